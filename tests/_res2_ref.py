"""The Res2Net dilated convolution (include/ktf_res2.h) restated in fp64 NumPy, one utterance at a time, straight from the header's
formulas, and the exactly representable inputs that tests/test_gpu_res2.py compares bit for bit (tests/test_res2_cpu.py checks that they
are: every intermediate and every partial sum's bound is a multiple of 2^-14 below 2^10, so fp32 holds every sum exactly in any order)."""

import numpy as np


def clamp_len(n, T):
    return int(min(max(int(n), 0), T))


def conv(x, s, d, W, bias=None, nscale=None, nshift=None, relu=True, trace=None):
    """x (n, C) -> y (n, C) fp64, n >= 1 valid rows. W (s-1, 3, w, w) as [g, k, in, out]; bias, nscale, nshift (s-1, w) or None.
    `trace`: a list that receives, per group, every intermediate and the bound sum |term| of the group's sums."""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    n, w = x.shape[0], x.shape[1] // s
    rows = np.clip(np.arange(n)[:, None] + (np.arange(3)[None, :] - 1) * d, 0, n - 1)            # (n, 3): t + (k - 1) d, edge row replicated
    Y = [x[:, :w]]
    for i in range(1, s):
        U = x[:, i * w:(i + 1) * w] + Y[-1] if i >= 2 else x[:, w:2 * w]
        b = np.zeros(w) if bias is None else np.asarray(bias[i - 1], np.float64)
        Z = b + np.einsum("nki,kio->no", U[rows], W[i - 1])
        A = np.maximum(Z, 0.0) if relu else Z
        Y.append(A if nscale is None else A * np.asarray(nscale[i - 1], np.float64) + np.asarray(nshift[i - 1], np.float64))
        if trace is not None:
            trace.append(dict(U=U, Z=Z, A=A, Y=Y[-1], bound=np.abs(b) + np.einsum("nki,kio->no", np.abs(U[rows]), np.abs(W[i - 1]))))
    return np.concatenate(Y, axis=1)


def batch(x, lens, s, d, W, **kw):
    """x (B, T, C), lens (B,) or None -> the list of conv() over every utterance's valid rows ((0, C) for an empty one)."""
    B, T, C = x.shape
    ns = [T if lens is None else clamp_len(lens[b], T) for b in range(B)]
    return [conv(x[b, :n], s, d, W, **kw) if n else np.zeros((0, C)) for b, n in enumerate(ns)]


def exact_case(w, s, d, lens, seed=0):
    """x (B, max(lens) + 3, s w) of integers in [-8, 8], W with four taps of +-1 per output channel, integer bias and nshift in
    [-3, 3], nscale = 2^-2: dict(x, W, bias, nscale, nshift), all fp32."""
    rng = np.random.default_rng(seed + 1000 * w + 100 * s + d)
    x = rng.integers(-8, 9, (len(lens), max(lens) + 3, s * w)).astype(np.float32)
    W = np.zeros((s - 1, 3 * w, w), np.float32)
    for g in range(s - 1):
        for o in range(w):
            W[g, rng.choice(3 * w, 4, replace=False), o] = rng.choice([-1.0, 1.0], 4)
    ints = lambda: rng.integers(-3, 4, (s - 1, w)).astype(np.float32)      # noqa: E731
    return dict(x=x, W=W.reshape(s - 1, 3, w, w), bias=ints(), nscale=np.full((s - 1, w), 0.25, np.float32), nshift=ints())


def exact_lens(s, d, R):
    return [0, 1, 2, d, d + 1, (s - 1) * d - 1, (s - 1) * d + 1, R - 1, R, R + 1, 2 * R + 1]
