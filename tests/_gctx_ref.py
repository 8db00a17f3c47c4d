"""Global-context attention (include/ktf_gctx.h) restated in fp64 NumPy, one utterance at a time, and the cases of test_gpu_gctx.py.

ctx. `stats` adds the rows in the canonical order (ktf_attn.h rule 8), so its sums have the kernel's bits (x * x is exact in fp64). What
may differ is one unit in the last place, u = 2^-52, per later operation: d mu <= u |mu|, d q <= u q, d (mu mu) <= 3 u mu^2, so
d var <= u (q + 3 mu^2 + |var|), and through the concave square root, sqrt(v + d) - sqrt(v) <= d / (2 sqrt(v)) with v >= eps:
    mu_bound = u |mu|,      sigma_bound = u (2 sigma + (q + 3 mu^2 + |var|) / (2 sigma)).
Every tested channel has var > 2^-20 q, which keeps the second term below 2^-31 sigma, or is constant over its utterance.
g = b1 + sum_k ctx_k W1c[k] is an fp32 output whose value is a sum with absolute terms S = |b1| + sum_k |ctx_k W1c[k]|; it may deviate by
1.01 * 2^-24 |g| + 2^-36 S + 2^-149 (_attn_ref.py: one rounding to fp32, 2^-36 S for two fp64 sums of at most 2^15 terms in different orders)."""

import numpy as np

U64 = 2.0 ** -52
EXACT_SHAPES = [(1, 1, 1), (33, 17, 5), (96, 128, 130), (130, 256, 33)]      # (D, A, H)
STATS_LENS = [0, 1, 2, 63, 64, 65, 129]


def canon_sum(v):
    """The sum over the rows of v (n, D) fp64 in the order of ktf_attn.h rule 8."""
    groups, s = np.zeros((64,) + v.shape[1:]), np.zeros(v.shape[1:])
    for k in range(0, v.shape[0], 64):
        groups[:len(v[k:k + 64])] += v[k:k + 64]
    for g in range(16):
        s = s + (((groups[g] + groups[g + 16]) + groups[g + 32]) + groups[g + 48])
    return s


def stats(x, n, eps):
    """x (T, D) fp32, its first n rows -> mu, sigma, their bounds, q and var (D,). n = 0: NaN."""
    xv = np.asarray(x[:n], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu, q = canon_sum(xv) / np.float64(n), canon_sum(xv * xv) / np.float64(n)
        var = q - mu * mu
        sigma = np.sqrt(np.where(var < 0, 0.0, var) + float(np.float32(eps)))
        sb = U64 * (2 * sigma + (q + 3 * mu * mu + np.abs(var)) / (2 * sigma))
    return dict(mu=mu, sigma=sigma, mu_bound=U64 * np.abs(mu), sigma_bound=sb, q=q, var=var)


def bias(mu, sigma, w1c, b1):
    """g = b1 + [mu ; sigma] W1c and S, the sum of its absolute terms."""
    c, w = np.concatenate([mu, sigma]), np.asarray(w1c, np.float64)
    return np.asarray(b1, np.float64) + c @ w, np.abs(b1) + np.abs(c) @ np.abs(w)


def logits(x, n, w1x, g, w2, b2, act):
    """h (n, A) and e (n, H) of the first n rows of x (T, D) for the per-utterance bias g (A,)."""
    z = np.asarray(x[:n], np.float64) @ np.asarray(w1x, np.float64) + np.asarray(g, np.float64)
    h = np.tanh(z) if act == "tanh" else np.maximum(z, 0.0)
    return h, h @ np.asarray(w2, np.float64) + np.asarray(b2, np.float64)


def utterance(x, n, w1, b1, w2, b2, act="tanh", eps=1e-10):
    """One utterance's attention for W1 (3 D, A), rows [x ; mu ; sigma] -> mu, sigma, g, S, h, e (and stats' other entries)."""
    D = w1.shape[0] // 3
    r = stats(np.asarray(x)[:, :D], n, eps)
    r["g"], r["S"] = bias(r["mu"], r["sigma"], w1[D:], b1)
    r["h"], r["e"] = logits(np.asarray(x)[:, :D], n, w1[:D], r["g"], w2, b2, act)
    return r


def exact_case(D, A, H, R):
    """Lengths around the row tile R and small integers: every partial sum of h = relu(x W1x + g) and of e = h W2 + b2 is an integer,
    below 2^16 in h (so h splits into two bf16 without loss) and below 2^24 in e."""
    lens, rng = [0, 1, 2, R - 1, R, R + 1, 2 * R + 1], np.random.default_rng(D + A + H)
    f = lambda lo, hi, *s: rng.integers(lo, hi + 1, s).astype(np.float32)      # noqa: E731
    return lens, dict(x=f(-3, 3, len(lens), max(lens), D), w1x=f(-2, 2, D, A), g=f(-8, 8, len(lens), A), w2=f(-2, 2, A, H), b2=f(-2, 2, H))


def stats_case(D, A):
    """Random rows of mean 0.5 and unit variance, channel 0 constant; W1c and b1 for the bias."""
    rng = np.random.default_rng(1 + D + A)
    x = (rng.standard_normal((len(STATS_LENS), max(STATS_LENS), D)) + 0.5).astype(np.float32)
    x[:, :, 0] = np.float32(0.7)
    return dict(x=x, w1c=(rng.standard_normal((2 * D, A)) / np.sqrt(2 * D)).astype(np.float32), b1=(0.1 * rng.standard_normal(A)).astype(np.float32))
