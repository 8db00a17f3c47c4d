"""The squeeze-excitation gate of include/ktf_se.h in numpy fp64, one utterance at a time and straight from the header's formulas, with
the bound of every output.

Bounds (the form of tests/_attn_ref.py). E = 2^-24 * 1.01 is one fp32 rounding of a value v (E |v|); an fp64 chain whose absolute terms sum
to S is off by at most F(S) = 2^-36 S + 2^-149 (generous against the 2^-53 per operation, so the order of the MFMA's four terms and its
unrounded products are covered). With d(.) the bound of a quantity:
  mu   d = F(sum_t |x| / len)
  a    (pre-activation) d = F(|b1| + sum_c |mu| |W1|) + sum_c d(mu_c) |W1[c,j]|;  h = relu(a): d(h) = d(a)  (the mask needs |a| > d(a):
       tests/test_se_cpu.py holds every case to |a| >= 2^-20 of its absolute-term sum)
  z    d = F(|b2| + sum_j |h| |W2|) + sum_j d(h_j) |W2[j,c]|
  s    = fl32(sigmoid(z)): d = E s + d(z) / 4 + F(1)            (|sigmoid'| <= 1/4; exp and the division)
  y    = fl32(fl32(x s) + r): d = |x| d(s) + E |x s| + E |x s + r| + 2^-149
  ds   d = F(sum_t |g x|)
  dz2  = ds s (1 - s): d = d(ds) / 4 + |ds| d(s) + F(|dz2|)    (|d/ds s(1-s)| <= 1; the kernel uses its own saved gate)
  dh   d = sum_c d(dz2_c) |W2[j,c]| + F(sum_c |dz2| |W2|)
  dmu  d = sum_j d(dh_j) |W1[c,j]| + F(sum_j |dh| |W1|)
  dx   = fl32(g s + dmu / len): d = |g| d(s) + d(dmu) / len + F(|g s| + |dmu| / len) + E |dx| + 2^-149
  dW2  = fl32(sum_b hid dz2): d = sum_b (d(h) |dz2| + |hid| d(dz2)) + F(sum_b |hid dz2|) + E |dW2|; dW1, db2, db1 likewise."""

import numpy as np

E = 2.0 ** -24 * 1.01


def F(S):
    return 2.0 ** -36 * S + 2.0 ** -149


def canon_sum(v):
    """Rule 2's order: rows t -> group t mod 64 ascending from +0; ((g + g+16) + g+32) + g+48 for g = 0..15, then ascending g."""
    n, C = v.shape
    k = -(-n // 64)
    vp = np.zeros((k * 64, C))
    vp[:n] = v
    G = np.zeros((64, C))
    for blk in vp.reshape(k, 64, C):
        G = G + blk
    s = np.zeros(C)
    for g in range(16):
        s = s + (((G[g] + G[g + 16]) + G[g + 32]) + G[g + 48])
    return s


def forward(x, r, w1, b1, w2, b2, round_gate=True):
    """x (n, C) and r (n, C) or None fp32, weights fp32 -> dict of fp64 values and bounds (n = 0: mu, h, s are +0). round_gate=False
    keeps the gate in fp64: the form tests/test_se_cpu.py compares with fp64 autograd."""
    n, C = x.shape
    H = w1.shape[1]
    x64, W1, W2 = x.astype(np.float64), w1.astype(np.float64), w2.astype(np.float64)
    B1 = np.zeros(H) if b1 is None else b1.astype(np.float64)
    B2 = np.zeros(C) if b2 is None else b2.astype(np.float64)
    o = {}
    if n == 0:
        z = np.zeros
        o.update(mean=z(C), a=z(H), a_abs=z(H), hid=z(H), gate=z(C, np.float32), y=z((0, C)), d_mean=z(C), d_hid=z(H), d_gate=z(C), d_y=z((0, C)))
        return o
    mu = canon_sum(x64) / n
    d_mu = F(np.abs(x64).sum(0) / n)
    a = B1.copy()
    for c in range(C):
        a = a + mu[c] * W1[c]
    a_abs = np.abs(B1) + np.abs(mu) @ np.abs(W1)
    d_a = F(a_abs) + d_mu @ np.abs(W1)
    h = np.where(a < 0, 0.0, a)
    z = B2.copy()
    for j in range(H):
        z = z + h[j] * W2[j]
    d_z = F(np.abs(B2) + np.abs(h) @ np.abs(W2)) + d_a @ np.abs(W2)
    s = 1.0 / (1.0 + np.exp(-z))
    s = s.astype(np.float32) if round_gate else s
    d_s = E * s + d_z / 4 + F(1.0)
    xs = x64 * s.astype(np.float64)
    y = xs + (0.0 if r is None else r.astype(np.float64))
    d_y = np.abs(x64) * d_s + E * np.abs(xs) + (0.0 if r is None else E * np.abs(y)) + 2.0 ** -149
    o.update(mean=mu, a=a, a_abs=a_abs, hid=h, gate=s, y=y, d_mean=d_mu, d_hid=d_a, d_gate=d_s, d_y=d_y)
    return o


def backward(g, x, w1, w2, f):
    """g (n, C) fp32 and the forward's dict f -> dx, the per-utterance terms of the parameter gradients, and their bounds."""
    n, C = x.shape
    H = w1.shape[1]
    W1, W2 = w1.astype(np.float64), w2.astype(np.float64)
    zc, zh = np.zeros(C), np.zeros(H)
    if n == 0:
        return dict(dx=np.zeros((0, C)), d_dx=np.zeros((0, C)), dz2=zc, d_dz2=zc, dh=zh, d_dh=zh)
    g64, x64, s = g.astype(np.float64), x.astype(np.float64), f["gate"].astype(np.float64)
    ds = canon_sum(g64 * x64)
    d_ds = F(np.abs(g64 * x64).sum(0))
    dz2 = ds * (s * (1.0 - s))
    d_dz2 = d_ds / 4 + np.abs(ds) * f["d_gate"] + F(np.abs(dz2))
    dh = np.zeros(H)
    for c in range(C):
        dh = dh + dz2[c] * W2[:, c]
    live = f["hid"] > 0
    dh = np.where(live, dh, 0.0)
    d_dh = np.where(live, d_dz2 @ np.abs(W2).T + F(np.abs(dz2) @ np.abs(W2).T), 0.0)
    dmu = np.zeros(C)
    for j in range(H):
        dmu = dmu + dh[j] * W1[:, j]
    d_dmu = d_dh @ np.abs(W1).T + F(np.abs(dh) @ np.abs(W1).T)
    dx = g64 * s + dmu / n
    d_dx = np.abs(g64) * f["d_gate"] + d_dmu / n + F(np.abs(g64 * s) + np.abs(dmu) / n) + E * np.abs(dx) + 2.0 ** -149
    return dict(dx=dx, d_dx=d_dx, dz2=dz2, d_dz2=d_dz2, dh=dh, d_dh=d_dh)


def param_grads(fs, bs):
    """The forward / backward dicts of a batch's utterances -> {name: (value, bound)} of dW1, db1, dW2, db2, sums in ascending b."""
    C, H = fs[0]["mean"].shape[0], fs[0]["hid"].shape[0]
    acc = {k: [np.zeros(sh), np.zeros(sh), np.zeros(sh)] for k, sh in (("dw1", (C, H)), ("db1", (H,)), ("dw2", (H, C)), ("db2", (C,)))}
    for f, b in zip(fs, bs):
        for k, u, du, v, dv in (("dw1", f["mean"][:, None], f["d_mean"][:, None], b["dh"][None], b["d_dh"][None]),
                                ("dw2", f["hid"][:, None], f["d_hid"][:, None], b["dz2"][None], b["d_dz2"][None]),
                                ("db1", 1.0, 0.0, b["dh"], b["d_dh"]), ("db2", 1.0, 0.0, b["dz2"], b["d_dz2"])):
            acc[k][0] = acc[k][0] + u * v
            acc[k][1] = acc[k][1] + np.abs(u * v)
            acc[k][2] = acc[k][2] + du * np.abs(v) + np.abs(u) * dv + du * dv
    return {k: (v, prop + F(S) + E * np.abs(v)) for k, (v, S, prop) in acc.items()}


def case(C, H, lens, T, seed, bias=True):
    """Seeded inputs of one batch: x, r, g (B, T, C) fp32 and the weights."""
    rng = np.random.default_rng(seed)
    B = len(lens)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)      # noqa: E731
    x, r, g = f(B, T, C), f(B, T, C), f(B, T, C)
    x += np.float32(0.5)                                             # (a mean away from zero: the squeeze has something to carry)
    w1, w2 = f(C, H) / np.float32(np.sqrt(C)), f(H, C) / np.float32(np.sqrt(H))
    return dict(x=x, r=r, g=g, w1=w1, w2=w2, b1=f(H) if bias else None, b2=f(C) if bias else None, lens=list(lens))


# (C, H, B) of tests/test_gpu_se.py: every value of each parameter with the extremes of the others
GRID = [(4, 1, 1), (4, 128, 17), (516, 1, 17), (516, 128, 1), (20, 17, 16), (64, 17, 17), (516, 128, 17), (4, 1, 17), (64, 128, 16), (20, 1, 1),
        (516, 17, 16), (64, 1, 17)]
LENGTHS = [0, 1, 2, 63, 64, 65, 129, 1025]


def grid_case(i):
    """Case i of GRID: one batch holding all the lengths (B = 1: one of them), and the variant it runs in."""
    C, H, B = GRID[i]
    lens = [LENGTHS[(k + i) % 8] for k in range(B)] if B > 1 else [LENGTHS[1 + i % 7]]
    # (offset, in floats, of the base behind a 256-byte boundary: 4 = 16 bytes, still float4 accesses; 1: the scalar accesses)
    var = dict(residual=i % 2 == 0, bias=i % 3 != 1, pad=4 * (i % 2), offset=1 if i in (5, 6) else 4 * ((i // 2) % 2), use_lens=i % 5 != 4)
    T = max(lens) + 3 if var["use_lens"] else 70
    if not var["use_lens"]:
        lens = [T] * B
    return case(C, H, lens, T, 1000 + i, var["bias"]), var
