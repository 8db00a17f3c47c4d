"""fp64 NumPy oracle of include/ktf_loss.h: the inverse row norms and the (margin) softmax loss, forward and backward, one row b at a
time over its columns j, restating rules N1, N2 and 1 - 6. Next to every result it returns the magnitudes the tests' bounds are
made of. Inputs are taken as they are (fp32 arrays are converted exactly); nothing is rounded to fp32 here."""

import math

import numpy as np

SOFTMAX, AM, AAM = "softmax", "am", "aam"
SIN2_FLOOR = 2.0 ** -20


def psi(c, kind, margin):
    """(psi(c), psi'(c)) of rule 3 for one fp64 cosine."""
    c = float(c)
    if kind == SOFTMAX:
        return c, 1.0
    if kind == AM:
        return c - margin, 1.0
    assert kind == AAM, kind
    cm, sm = math.cos(margin), math.sin(margin)
    if c > -cm:
        s2 = 1.0 - c * c
        if s2 > SIN2_FLOOR:
            S = math.sqrt(s2)
            return c * cm - S * sm, cm + (sm * c) / S
        return c * cm - math.sqrt(SIN2_FLOOR) * sm, cm
    return c - margin * sm, 1.0


def inv_norm(x, eps):
    """x (rows, D) -> dict: inv (rows,) = 1 / max(|x[r]|, eps), clamped (rows,) bool = |x[r]| < eps."""
    x = np.asarray(x, dtype=np.float64)
    inv, clamped = np.zeros(x.shape[0]), np.zeros(x.shape[0], dtype=bool)
    for r in range(x.shape[0]):
        nrm = math.sqrt(float(np.sum(x[r] * x[r])))
        clamped[r] = nrm < eps
        inv[r] = 1.0 / max(nrm, eps)
    return dict(inv=inv, clamped=clamped)


def inv_norm_backward(x, eps, inv, ginv):
    """dx (rows, D) = -ginv[r] * inv[r]^3 * x[r, d], zero for a clamped row (whose ginv is not looked at). `inv` as the backward call
    gets it (the library's fp32 value, or inv_norm's)."""
    x = np.asarray(x, dtype=np.float64)
    inv, ginv = np.asarray(inv, dtype=np.float64), np.asarray(ginv, dtype=np.float64)
    clamped = inv_norm(x, eps)["clamped"]
    dx = np.zeros_like(x)
    for r in range(x.shape[0]):
        if not clamped[r]:
            dx[r] = (-ginv[r] * ((inv[r] * inv[r]) * inv[r])) * x[r]
    return dx


def _cos(z, b, inv_x, inv_w):
    return z[b] if inv_x is None else (z[b] * inv_x[b]) * inv_w


def _prep(z, labels, inv_x, inv_w):
    z = np.asarray(z, dtype=np.float64)
    labels = [int(v) for v in np.asarray(labels).reshape(-1)]
    assert (inv_x is None) == (inv_w is None)
    if inv_x is not None:
        inv_x, inv_w = np.asarray(inv_x, dtype=np.float64), np.asarray(inv_w, dtype=np.float64)
    return z, labels, inv_x, inv_w


def forward(z, labels, inv_x, inv_w, kind, margin, scale):
    """z (B, N) (any columns beyond N already cut off). Returns a dict: loss, lse, ly (the target logit, 0 for an ignored row), pred,
    valid (B,), c (B, N) the cosines, gap (B,) the relative distance of the two largest cosines of a row (inf for N = 1)."""
    z, labels, inv_x, inv_w = _prep(z, labels, inv_x, inv_w)
    B, N = z.shape
    out = dict(loss=np.zeros(B), lse=np.zeros(B), ly=np.zeros(B), pred=np.zeros(B, dtype=np.int32), valid=np.zeros(B, dtype=bool),
               c=np.zeros((B, N)), gap=np.full(B, np.inf))
    for b in range(B):
        c = _cos(z, b, inv_x, inv_w)
        y = labels[b]
        valid = 0 <= y < N
        l = scale * c
        if valid:
            l[y] = scale * psi(c[y], kind, margin)[0]
        M = float(np.max(l))
        lse = M + math.log(float(np.sum(np.exp(l - M))))
        out["c"][b], out["lse"][b], out["valid"][b] = c, lse, valid
        if valid:
            out["ly"][b] = l[y]
            out["loss"][b] = lse - l[y]
        out["pred"][b] = int(np.argmax(c))              # the first of equal maxima
        if N > 1:
            top = np.sort(c)[-2:]
            out["gap"][b] = (top[1] - top[0]) / max(abs(top[1]), 1e-300)
    return out


def backward(z, labels, inv_x, inv_w, kind, margin, scale, lse, gloss=None):
    """The gradient of sum_b gloss[b] * loss[b] (gloss None: ones; an ignored row's gloss is not looked at). Returns a dict: dz (B, N),
    dz_mag = |gloss * scale * psi' * inv_x * inv_w| * (p_j + [j = y]), dinv_x (B,), dinv_w (N,) (zeros for a plain head) and
    dinv_x_abs / dinv_w_abs, the sums of the absolute values of their terms."""
    z, labels, inv_x, inv_w = _prep(z, labels, inv_x, inv_w)
    B, N = z.shape
    lse = np.asarray(lse, dtype=np.float64)
    out = dict(dz=np.zeros((B, N)), dz_mag=np.zeros((B, N)), dinv_x=np.zeros(B), dinv_x_abs=np.zeros(B), dinv_w=np.zeros(N),
               dinv_w_abs=np.zeros(N))
    for b in range(B):
        y = labels[b]
        if not 0 <= y < N:
            continue
        g = 1.0 if gloss is None else float(gloss[b])
        c = _cos(z, b, inv_x, inv_w)
        l = scale * c
        py, dpy = psi(c[y], kind, margin)
        l[y] = scale * py
        p = np.exp(l - lse[b])
        hot, slope = np.zeros(N), np.ones(N)
        hot[y], slope[y] = 1.0, dpy
        dc = ((g * scale) * (p - hot)) * slope
        mag = np.abs(g * scale * slope) * (p + hot)
        if inv_x is None:
            out["dz"][b], out["dz_mag"][b] = dc, mag
            continue
        out["dz"][b] = (dc * inv_x[b]) * inv_w
        out["dz_mag"][b] = mag * abs(inv_x[b]) * np.abs(inv_w)
        tx, tw = (dc * z[b]) * inv_w, (dc * z[b]) * inv_x[b]
        out["dinv_x"][b], out["dinv_x_abs"][b] = np.sum(tx), np.sum(np.abs(tx))
        out["dinv_w"] += tw
        out["dinv_w_abs"] += np.abs(tw)
    return out
