"""Attentive statistics pooling (include/ktf_attn.h, rules 1 to 12) restated in fp64 NumPy, one utterance at a time, with the
magnitudes its error bounds are made of, and the tables of cases test_gpu_attn.py runs and test_attn_cpu.py checks on the CPU.

U = 2^-24. An fp32 output v whose value is a sum with absolute terms S may deviate by
    |err| <= 1.01 U |v| + 2^-36 S + 2^-149
(the form test_gpu_loss.py uses): one rounding to fp32, and 2^-36 S for what the fp64 sums of the kernel and of this restatement may
differ by, (n + a few) 2^-53 S each with n <= 2^15 terms, amplified where a difference cancels. What S is made of, per output:

  mean    S = sum_t w |x|                                         (= mu_abs)
  std     through the concave square root, sqrt(v + d) - sqrt(v) <= d / (2 sqrt(v)): 2^-36 (q + mu^2) / (2 std) in place of 2^-36 S
          (q + mu^2 is what cancels in var = q - mu^2, and std >= sqrt(eps))
  dx      a_c + 2 b_c x = gmu + gsig (x - mu) / sigma. sigma carries the relative error of var, kappa = (q + mu^2) / (2 (var + eps))
          units of 2^-36, so S = w (|gmu| + (1 + kappa) |gsig| (mu_abs + |x|) / sigma). Every tested channel has var > 2^-20 q, which
          keeps kappa below 2^21, or is constant over its utterance: there x - mu is rounding noise of at most (n + 2) 2^-53 |x|
          whatever sigma is, kappa does not enter, and S = w (|gmu| + 2 |gsig| |x| / sqrt(eps)) holds for both values of `live`
          (var is +-noise there, so the kernel may take either; test_attn_cpu.py checks that both lie within the bound).
  de      S = w sum_{c in j} (a_abs (|x| + mu_abs) + b_abs (x^2 + q)) with a_abs = |gmu| + (1 + kappa) |gsig| mu_abs / sigma and
          b_abs = (1 + kappa) |gsig| / (2 sigma); for a constant channel a_abs = |gmu| + |gsig| |x| / sqrt(eps),
          b_abs = |gsig| / (2 sqrt(eps)).
"""

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
NAN = float("nan")


def bound(v, S):
    return 1.01 * U * np.abs(v) + 2.0 ** -36 * S + TINY


def clamp_len(n, T):
    return T if n is None else max(0, min(int(n), T))


def _eps(eps):
    return float(np.float32(eps))           # (the library takes eps as a float)


def forward(x, e, n, include_std=True, eps=1e-10):
    """x (T, ldx >= D) and e (T, lde >= H) fp32, of which only the first n rows are read -> a dict: out (D or 2 D) and out_bound, the
    side outputs m, Z (H), mu, q (D), and mu_abs, var, const (D). n = 0: out is NaN (0 / 0), bound 0."""
    x, e = np.asarray(x), np.asarray(e)
    D, H = x.shape[1], e.shape[1]
    assert 1 <= H <= D and D % H == 0
    od = 2 * D if include_std else D
    if n == 0:
        return dict(out=np.full(od, NAN), out_bound=np.zeros(od), m=np.full(H, -np.inf), Z=np.zeros(H), mu=np.full(D, NAN),
                    q=np.full(D, NAN), n=0)
    xv, ev = x[:n].astype(np.float64), e[:n].astype(np.float64)
    m = ev.max(0)
    p = np.exp(ev - m)
    Z = p.sum(0)
    pc, Zc = np.repeat(p, D // H, axis=1), np.repeat(Z, D // H)
    mu = (pc * xv).sum(0) / Zc
    q = (pc * (xv * xv)).sum(0) / Zc
    mu_abs = (pc * np.abs(xv)).sum(0) / Zc
    var = q - mu * mu
    const = (xv == xv[0]).all(0)
    out, ob = mu, bound(mu, mu_abs)
    if include_std:
        std = np.sqrt(np.maximum(var, 0.0) + _eps(eps))
        with np.errstate(divide="ignore", invalid="ignore"):
            sb = np.where(std > 0, 1.01 * U * std + 2.0 ** -36 * (q + mu * mu) / (2 * std) + TINY, 0.0)
        out, ob = np.concatenate([mu, std]), np.concatenate([ob, sb])
    return dict(out=out, out_bound=ob, m=m, Z=Z, mu=mu, q=q, mu_abs=mu_abs, var=var, const=const, n=n, w=p / Z)


def backward(x, e, n, gout, fwd, include_std=True, eps=1e-10, live=None):
    """The gradients of rule 12 for one utterance: dx (T, D), de (T, H) with zero rows from n on, and their bounds. `fwd` is
    forward()'s answer; `live` (None or a bool) overrides rule 12's `var > 0` on the constant channels, where it is undecided."""
    x, e = np.asarray(x), np.asarray(e)
    T, D, H = x.shape[0], x.shape[1], e.shape[1]
    dh = D // H
    dx, de = np.zeros((T, D)), np.zeros((T, H))
    dxb, deb = np.zeros((T, D)), np.zeros((T, H))
    if n == 0:
        return dict(dx=dx, de=de, dx_bound=dxb, de_bound=deb)
    g = np.asarray(gout).astype(np.float64)
    xv = x[:n].astype(np.float64)
    mu, q, var, const, mu_abs = fwd["mu"], fwd["q"], fwd["var"], fwd["const"], fwd["mu_abs"]
    gmu = g[:D]
    a, b = gmu.copy(), np.zeros(D)
    a_abs, b_abs = np.abs(gmu), np.zeros(D)
    ax = np.abs(xv)
    sx = np.abs(gmu)[None, :] * np.ones_like(xv)                 # S of dx / w
    if include_std:
        gs = g[D:2 * D]
        on = var > 0
        if live is not None:
            on = np.where(const, live, on)
        sg = np.sqrt(np.maximum(var, 0.0) + _eps(eps))
        a = np.where(on, gmu - (gs * mu) / sg, gmu)
        b = np.where(on, gs / (2 * sg), 0.0)
        kappa = (q + mu * mu) / (2 * (np.maximum(var, 0.0) + _eps(eps)))
        root = np.sqrt(_eps(eps)) if _eps(eps) > 0 else np.inf
        a_abs = np.where(const, np.abs(gmu) + np.abs(gs) * ax[0] / root, np.abs(gmu) + (1 + kappa) * np.abs(gs) * mu_abs / sg)
        b_abs = np.where(const, np.abs(gs) / (2 * root), (1 + kappa) * np.abs(gs) / (2 * sg))
        sx = np.where(const[None, :], np.abs(gmu) + 2 * np.abs(gs) * ax / root,
                      np.abs(gmu) + ((1 + kappa) * np.abs(gs) / sg)[None, :] * (mu_abs[None, :] + ax))
    w = fwd["w"]
    wc = np.repeat(w, dh, axis=1)
    dx[:n] = wc * (a + (2 * b) * xv)
    dxb[:n] = bound(dx[:n], wc * sx)
    S = (a * xv + b * (xv * xv)).reshape(n, H, dh).sum(2)
    K = (a * mu + b * q).reshape(H, dh).sum(1)
    de[:n] = w * (S - K)
    mag = (a_abs * (ax + mu_abs) + b_abs * (xv * xv + q)).reshape(n, H, dh).sum(2)
    deb[:n] = bound(de[:n], w * mag)
    return dict(dx=dx, de=de, dx_bound=dxb, de_bound=deb)


def pool(x, e, lens=None, include_std=True, eps=1e-10, gout=None, D=None, H=None):
    """The batch: x (B, T, ldx), e (B, T, lde) -> dict of stacked forward values and, with gout (B, >= D or 2 D), the gradients."""
    x, e = np.asarray(x), np.asarray(e)
    B, T = x.shape[:2]
    D = x.shape[2] if D is None else D
    H = e.shape[2] if H is None else H
    od = 2 * D if include_std else D
    res = dict(out=[], out_bound=[], dx=[], de=[], dx_bound=[], de_bound=[], fwd=[])
    for b in range(B):
        n = clamp_len(None if lens is None else lens[b], T)
        f = forward(x[b, :, :D], e[b, :, :H], n, include_std, eps)
        res["fwd"].append(f)
        res["out"].append(f["out"])
        res["out_bound"].append(f["out_bound"])
        if gout is not None:
            r = backward(x[b, :, :D], e[b, :, :H], n, np.asarray(gout)[b, :od], f, include_std, eps)
            for k in ("dx", "de", "dx_bound", "de_bound"):
                res[k].append(r[k])
    return {k: (np.stack(v) if k != "fwd" and v else v) for k, v in res.items()}


def ratio(got, want, bnd):
    """worst |got - want| / bound over the elements; NaN must sit exactly where the reference has it."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaN pattern"
    err = np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, want))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bnd)
    return float(r.max(initial=0.0))


# ----------------------------------------------------------------------------- the inputs of test_gpu_attn.py
DIMS = ((1, 1), (3, 1), (3, 3), (30, 5), (128, 1), (130, 2), (130, 130), (257, 1), (1500, 4))
LENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1025)
T_MAX = max(LENS) + 1
EPS = 1e-10


def kernel_data(D, H, seed=0, lens=LENS, T=T_MAX, const_channel=None):
    """x (B, T, D) with a per-channel offset of at most one standard deviation (var > q / 4), logits with a spread of a few units,
    gout (B, 2 D). `const_channel`: that channel is constant over every utterance."""
    rng = np.random.default_rng([seed, D, H])
    B = len(lens)
    x = (rng.standard_normal((B, T, D)) + rng.uniform(-1, 1, (1, 1, D))).astype(np.float32)
    # (an utterance of two rows has a variance too: they differ by more than one)
    x[:, 1] = x[:, 0] + (rng.choice((-1.0, 1.0), (B, D)) * (1.0 + np.abs(rng.standard_normal((B, D))))).astype(np.float32)
    e =(2.0 * rng.standard_normal((B, T, H)) + rng.uniform(-3, 3, (B, 1, H))).astype(np.float32)
    if const_channel is not None:
        x[:, :, const_channel] = rng.uniform(0.5, 2.0, (B, 1)).astype(np.float32)
    gout = rng.standard_normal((B, 2 * D)).astype(np.float32)
    return x, e, np.asarray(lens, np.int32), gout


def kernel_case(D, H, with_lens=True, const_channel=None):
    """The input of test_kernels_match_the_restatement: every length of LENS in one batch, or two utterances without `lens`."""
    x, e, lens, gout = kernel_data(D, H, const_channel=const_channel)
    if not with_lens:
        x, e, gout, lens = x[:2, :130], e[:2, :130], gout[:2], None
    return x, e, lens, gout


STRIDE_DIMS = ((3, 3), (130, 2), (257, 1))
STRIDE_LENS = (0, 1, 65, 129, 200)
INVARIANCE_CASES = ((1500, 4, 30, (300, 0, 1, 2, 63, 64, 65, 127, 128, 129)), (130, 130, 180, (65, 0, 1, 2, 63, 64)),
                    (30, 5, 12, (129, 1, 64, 200)))
SHIFT_DIMS = ((30, 5), (130, 130), (128, 1))
SHIFT_LENS = (129, 1, 64)
CONST_LOGIT_DIMS = ((30, 5), (257, 1), (130, 130))
CONST_LOGIT_LENS = (200, 1, 65, 2)
AUTOGRAD_DIMS = ((30, 5), (130, 130), (128, 1))
AUTOGRAD_LENS = (129, 1, 64, 0)
DOMINANT = (130, 2, 97, 40)        # D, H, T and the row whose logit stands 60 above the others


def stride_case(D, H):
    return kernel_data(D, H, seed=1, lens=STRIDE_LENS, T=max(STRIDE_LENS) + 1)


def invariance_case(D, H, B, lens):
    lens_b = [lens[b % len(lens)] for b in range(B)]
    return kernel_data(D, H, seed=2, lens=lens_b, T=max(lens) + 1)


def shift_case(D, H):
    """Logits that are multiples of 1/8 in [-8, 8], and the same moved by a multiple of 4096 per head (exactly)."""
    T = max(SHIFT_LENS) + 1
    x, _, lens, gout = kernel_data(D, H, seed=4, lens=SHIFT_LENS, T=T)
    e = (np.random.default_rng(5).integers(-64, 65, (len(lens), T, H)) / 8.0).astype(np.float32)
    move = 4096.0 * (1 + np.arange(H) % 3)
    shifted = (e.astype(np.float64) + move).astype(np.float32)
    assert np.array_equal(shifted.astype(np.float64) - move, e)
    return x, e, shifted, lens, gout


def dominant_case():
    D, H, T, row = DOMINANT
    x, e, _, _ = kernel_data(D, H, seed=6, lens=(T,), T=T)
    e = np.clip(e, -2, 2)
    e[0, row] += 60.0
    return x, e


def autograd_case(D, H):
    return kernel_data(D, H, seed=9, lens=AUTOGRAD_LENS, T=max(AUTOGRAD_LENS) + 1)


def const_logit_case(D, H):
    T = max(CONST_LOGIT_LENS) + 1
    x, _, lens, _ = kernel_data(D, H, seed=7, lens=CONST_LOGIT_LENS, T=T)
    e = np.repeat(np.random.default_rng(8).standard_normal((len(lens), 1, H)).astype(np.float32), T, axis=1)
    return x, e, lens


def gpu_inputs():
    """(tag, x, e, lens, gradients checked) of every input test_gpu_attn.py gives the kernels."""
    for D, H in DIMS:
        for with_lens in (True, False):
            x, e, lens, _ = kernel_case(D, H, with_lens)
            yield f"kernel {D} {H} {with_lens}", x, e, lens, True
    x, e, lens, _ = kernel_case(30, 5, True, 7)
    yield "constant channel", x, e, lens, True
    for D, H in STRIDE_DIMS:
        x, e, lens, _ = stride_case(D, H)
        yield f"stride {D} {H}", x, e, lens, True
    for D, H, B, lens in INVARIANCE_CASES:
        x, e, lens_b, _ = invariance_case(D, H, B, lens)
        yield f"invariance {D} {H}", x, e, lens_b, True
    for D, H in SHIFT_DIMS:
        x, e, shifted, lens, _ = shift_case(D, H)
        yield f"shift {D} {H}", x, e, lens, True
        yield f"shifted {D} {H}", x, shifted, lens, True
    for D, H in AUTOGRAD_DIMS:
        x, e, lens, _ = autograd_case(D, H)
        yield f"autograd {D} {H}", x, e, lens, True
    for D, H in CONST_LOGIT_DIMS:
        x, e, lens = const_logit_case(D, H)
        yield f"constant logits {D} {H}", x, e, lens, False
    x, e = dominant_case()
    yield "dominant", x, e, None, False


def check_inputs(x, e, lens, fwds, gradients=True):
    """What the bounds assume of a test input (the docstring above): |e - m| <= 64, and -- where gradients are compared: the bounds
    of the forward do not need it -- every channel of every utterance either has var > 2^-20 q or is constant over the utterance's
    rows."""
    for b, f in enumerate(fwds):
        n = f["n"]
        if n == 0:
            continue
        assert (np.abs(np.asarray(e)[b, :n, :f["m"].shape[0]].astype(np.float64) - f["m"]) <= 64).all(), b
        if gradients:
            ok = (f["var"] > 2.0 ** -20 * f["q"]) | f["const"]
            assert ok.all(), (b, np.flatnonzero(~ok))
