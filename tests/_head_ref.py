"""fp64 NumPy oracle of include/ktf_head.h: the head's loss with sub-centres (H1), the inter-top-k penalty (H2) and label smoothing
(H3), forward and backward (H4), one row b at a time over its classes j, in the operation order the header writes down. Next to every
result it returns the magnitudes the tests' bounds are made of. psi is that of tests/_loss_ref.py. Inputs are taken as they are (fp32
arrays are converted exactly); nothing is rounded to fp32 here."""

import math

import numpy as np

from _loss_ref import psi

MAX_CENTERS, MAX_TOPK = 8, 64


def _prep(z, labels, inv_x, inv_w, K):
    z = np.asarray(z, dtype=np.float64)
    assert z.ndim == 2 and z.shape[1] % K == 0 and 1 <= K <= MAX_CENTERS
    labels = [int(v) for v in np.asarray(labels).reshape(-1)]
    assert (inv_x is None) == (inv_w is None) and (inv_x is not None or K == 1)
    if inv_x is not None:
        inv_x, inv_w = np.asarray(inv_x, dtype=np.float64), np.asarray(inv_w, dtype=np.float64)
    return z, labels, inv_x, inv_w


def class_cosines(z, b, inv_x, inv_w, K):
    """H1 for row b: (c (N,), kstar (N,) the lowest centre attaining it, ck (N, K) the centres' cosines)."""
    ck = z[b] if inv_x is None else (z[b] * inv_x[b]) * inv_w
    ck = ck.reshape(-1, K)
    kstar = np.argmax(ck, axis=1)                        # the first of equal maxima
    return ck[np.arange(ck.shape[0]), kstar], kstar, ck


def select(c, y, topk):
    """H2: the first min(topk, N - 1) classes j != y in the order "c_j descending, then j ascending" (+0 equals -0)."""
    if topk == 0:
        return []
    order = sorted((j for j in range(len(c)) if j != y), key=lambda j: (-float(c[j]), j))
    return order[:min(topk, len(c) - 1)]


def forward(z, labels, inv_x, inv_w, kind, margin, scale, K=1, topk=0, penalty=0.0, eps=0.0):
    """z (B, N * K) class-major (any columns beyond N * K already cut off). Returns a dict: loss, lse, ly (the target logit, 0 for an
    ignored row), lmean (the mean logit), pred, sub_y, valid (B,), hard (B, max(topk, 1)), c (B, N) the class cosines, kstar (B, N),
    l (B, N) the logits."""
    z, labels, inv_x, inv_w = _prep(z, labels, inv_x, inv_w, K)
    assert 0 <= topk <= MAX_TOPK and penalty >= 0.0 and (topk > 0 or penalty == 0.0) and 0.0 <= eps < 1.0
    assert inv_x is not None or topk == 0
    B, N = z.shape[0], z.shape[1] // K
    out = dict(loss=np.zeros(B), lse=np.zeros(B), ly=np.zeros(B), lmean=np.zeros(B), pred=np.zeros(B, dtype=np.int32),
               sub_y=np.full(B, -1, dtype=np.int32), valid=np.zeros(B, dtype=bool), hard=np.full((B, max(topk, 1)), -1, dtype=np.int32),
               c=np.zeros((B, N)), kstar=np.zeros((B, N), dtype=np.int64), l=np.zeros((B, N)))
    for b in range(B):
        c, kstar, _ = class_cosines(z, b, inv_x, inv_w, K)
        y = labels[b]
        valid = 0 <= y < N
        l = scale * c
        if valid:
            members = select(c, y, topk)
            for j in members:
                l[j] = scale * (c[j] + penalty)
            out["hard"][b, :len(members)] = members
            l[y] = scale * psi(c[y], kind, margin)[0]
            out["sub_y"][b] = kstar[y]
        M = float(np.max(l))
        lse = M + math.log(float(np.sum(np.exp(l - M))))
        out["c"][b], out["kstar"][b], out["l"][b], out["lse"][b], out["valid"][b] = c, kstar, l, lse, valid
        if valid:
            mean = float(np.sum(l)) / N
            out["ly"][b], out["lmean"][b] = l[y], mean
            out["loss"][b] = (lse - l[y]) + eps * (l[y] - mean) if eps != 0.0 else lse - l[y]
        out["pred"][b] = int(np.argmax(c))               # the first of equal maxima
    return out


def backward(z, labels, inv_x, inv_w, kind, margin, scale, K, topk, penalty, eps, lse, hard, gloss=None):
    """The gradient of sum_b gloss[b] * loss[b] (gloss None: ones; an ignored row's gloss is not looked at), with the forward call's
    lse and hard. Returns a dict: dz (B, N * K), dz_mag = |gloss scale psi' inv_x inv_w| (p_j + [j = y] + eps ([j = y] + 1 / N)) on the
    selected centres, dinv_x (B,), dinv_w (N * K,) (zeros for a plain head), dinv_x_abs / dinv_w_abs, the sums of the absolute
    values of their terms, and selected (N * K,) bool: the centres some valid row selected."""
    z, labels, inv_x, inv_w = _prep(z, labels, inv_x, inv_w, K)
    B, N = z.shape[0], z.shape[1] // K
    lse, hard = np.asarray(lse, dtype=np.float64), np.asarray(hard)
    out = dict(dz=np.zeros((B, N * K)), dz_mag=np.zeros((B, N * K)), dinv_x=np.zeros(B), dinv_x_abs=np.zeros(B), dinv_w=np.zeros(N * K),
               dinv_w_abs=np.zeros(N * K), selected=np.zeros(N * K, dtype=bool))
    for b in range(B):
        y = labels[b]
        if not 0 <= y < N:
            continue
        g = 1.0 if gloss is None else float(gloss[b])
        c, kstar, _ = class_cosines(z, b, inv_x, inv_w, K)
        cols = np.arange(N) * K + kstar
        l = scale * c
        if topk > 0:
            for j in hard[b]:
                if 0 <= j < N:
                    l[j] = scale * (c[j] + penalty)
        py, dpy = psi(c[y], kind, margin)
        l[y] = scale * py
        p = np.exp(l - lse[b])
        hot, slope = np.zeros(N), np.ones(N)
        hot[y], slope[y] = 1.0, dpy
        dc = ((g * scale) * ((p - hot) + eps * (hot - 1.0 / N))) * slope
        mag = np.abs(g * scale * slope) * (p + hot + eps * (hot + 1.0 / N))
        out["selected"][cols] = True
        if inv_x is None:
            out["dz"][b, cols], out["dz_mag"][b, cols] = dc, mag
            continue
        zs, iws = z[b, cols], inv_w[cols]
        out["dz"][b, cols] = (dc * inv_x[b]) * iws
        out["dz_mag"][b, cols] = mag * abs(inv_x[b]) * np.abs(iws)
        tx, tw = (dc * zs) * iws, (dc * zs) * inv_x[b]
        out["dinv_x"][b], out["dinv_x_abs"][b] = np.sum(tx), np.sum(np.abs(tx))
        out["dinv_w"][cols] += tw
        out["dinv_w_abs"][cols] += np.abs(tw)
    return out
