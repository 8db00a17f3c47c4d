"""The gradient of the global-context attention logits (include/ktf_gcgrad.h) restated in fp64 NumPy, one utterance at a time.

Every output comes with S, the same expression over absolute values, which the bound k u S of rule 9 uses. Two places add what the
plain expression over absolute values does not see: dz = dh d with d = 1 - h^2 takes the sensitivity of d to h's own error in
(|dh| 2 |h| S_z), and a relu unit whose |z| is below 2^-18 S_z may switch either way, so its S is scaled to cover |dh| itself."""

import numpy as np

import _gctx_ref as G

K = dict(h=5, dz=8, coef=9, dw1c=9, db1=9, dx=10)      # rounded stages per output (rule 9)
U = {"f32": 2.0 ** -24, "bf16x3": (3 + 2.0 ** -6) * 2.0 ** -16}


def utterance(x, n, w1, b1, w2, de, act="tanh", eps=1e-10, dx_in=None):
    """x (T, >= D) and de (T, >= H), their first n rows; W1 (3 D, A), b1 (A,), W2 (A, H) -> a dict of (value, S) pairs: h, dz (n, A), coef
    (2, D), dx (n, D), and this utterance's terms of dw1x (D, A), dw1c (2 D, A), db1 (A,), dw2 (A, H), db2 (H,)."""
    D, A, H = w1.shape[0] // 3, w1.shape[1], w2.shape[1]
    f = lambda a: np.asarray(a, np.float64)      # noqa: E731
    w1x, w1c, w2 = f(w1[:D]), f(w1[D:]), f(w2)
    if n == 0:
        z = lambda *s: (np.zeros(s), np.zeros(s))      # noqa: E731
        return dict(h=z(0, A), dz=z(0, A), coef=z(2, D), dx=z(0, D), dw1x=z(D, A), dw1c=z(2 * D, A), db1=z(A), dw2=z(A, H), db2=z(H))
    xv, dev = f(np.asarray(x)[:n, :D]), f(np.asarray(de)[:n, :H])
    st = G.stats(np.asarray(x)[:, :D], n, eps)
    mu, sigma = st["mu"], st["sigma"]
    g, Sg = G.bias(mu, sigma, w1c, f(b1))
    z, Sz = xv @ w1x + g, np.abs(xv) @ np.abs(w1x) + Sg
    if act == "tanh":
        h = np.tanh(z)
        d = 1.0 - h * h
    else:
        h, d = np.maximum(z, 0.0), (z > 0).astype(np.float64)
    Sh = Sz + np.abs(h)
    dh, Sdh = dev @ w2.T, np.abs(dev) @ np.abs(w2).T
    dz = dh * d
    Sdz = Sdh * np.abs(d) + (np.abs(dh) * 2 * np.abs(h) * Sz if act == "tanh" else np.where(np.abs(z) < 2.0 ** -18 * Sz, 2.0 ** 24 * Sdh, 0.0))
    dg, Sdg = dz.sum(0), Sdz.sum(0)
    ctx = np.concatenate([mu, sigma])
    dctx, Sdctx = w1c @ dg, np.abs(w1c) @ Sdg
    live = sigma * sigma > float(np.float32(eps))
    c0, Sc0 = dctx[:D] / n, Sdctx[:D] / n
    c1, Sc1 = np.where(live, dctx[D:] / (n * sigma), 0.0), np.where(live, Sdctx[D:] / (n * sigma), 0.0)
    dx, Sdx = dz @ w1x.T + c0 + c1 * (xv - mu), Sdz @ np.abs(w1x).T + Sc0 + Sc1 * (np.abs(xv) + np.abs(mu))
    if dx_in is not None:
        dx, Sdx = dx + f(dx_in[:n, :D]), Sdx + np.abs(f(dx_in[:n, :D]))
    return dict(h=(h, Sh), dz=(dz, Sdz), coef=(np.stack([c0, c1]), np.stack([Sc0, Sc1])), dx=(dx, Sdx), dw1x=(xv.T @ dz, np.abs(xv).T @ Sdz),
                dw1c=(np.outer(ctx, dg), np.outer(np.abs(ctx), Sdg)), db1=(dg, Sdg), dw2=(h.T @ dev, Sh.T @ np.abs(dev)),
                db2=(dev.sum(0), np.abs(dev).sum(0)))


def case(D, A, H, T, lens, seed=0):
    """Random operands of unit-order hidden units; channel 0 of x is constant (s_c = 0)."""
    rng = np.random.default_rng(1000 * D + 10 * A + H + T + seed)
    r = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
    x = r(len(lens), T, D) + np.float32(0.5)
    x[:, :, 0] = np.float32(0.7)
    w1 = r(3 * D, A) / np.float32(np.sqrt(3 * D))
    return dict(x=x, w1=w1, b1=np.float32(0.1) * r(A), w2=r(A, H) / np.float32(np.sqrt(A)), de=r(len(lens), T, H), dx_in=r(len(lens), T, D))
