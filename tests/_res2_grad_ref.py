"""The backward of the Res2Net dilated convolution (include/ktf_res2.h rules 8 - 12) in fp64 NumPy, one utterance at a time, straight
from the header's formulas, on the fp32 x, y, a the forward saved (the mask is never re-derived), with the sum of absolute terms of
every output; and the forward restated as torch conv1d on replicate-padded slices, for fp64 autograd."""

import numpy as np
import torch


def shifted(dZ, d):
    """S_0, S_1, S_2 of rule 10 for dZ (n, w)."""
    n = len(dZ)
    S0, S2 = np.zeros_like(dZ), np.zeros_like(dZ)
    S0[0] = dZ[:min(d, n - 1) + 1].sum(0)
    S2[n - 1] = dZ[max(n - 1 - d, 0):].sum(0)
    r = np.arange(1, n)
    S0[r[r + d < n]] = dZ[r[r + d < n] + d]
    r = np.arange(0, n - 1)
    S2[r[r - d >= 0]] = dZ[r[r - d >= 0] - d]
    return S0, dZ, S2


def grad(x, y, a, g, s, d, W, nscale=None, relu=True):
    """x, y, g (n, C), a (n, (s-1) w) or None, W (s-1, 3, w, w) as [g, k, in, out], nscale (s-1, w) or None ->
    (dict dx, dW, dbias, dnscale, dnshift, gt), (the same keys: sum of |terms|)."""
    x, y, g, W = (np.asarray(v, np.float64) for v in (x, y, g, W))
    n, w = x.shape[0], x.shape[1] // s
    rows = np.clip(np.arange(n)[:, None] + (np.arange(3)[None, :] - 1) * d, 0, n - 1)
    out = dict(dx=np.zeros_like(x), dW=np.zeros_like(W), dbias=np.zeros((s - 1, w)), dnscale=np.zeros((s - 1, w)), dnshift=np.zeros((s - 1, w)),
               gt=np.zeros((n, (s - 1) * w)))
    bnd = {k: np.zeros_like(v) for k, v in out.items()}
    out["dx"][:, :w], bnd["dx"][:, :w] = g[:, :w], np.abs(g[:, :w])
    dU, bU = 0.0, 0.0
    for i in range(s - 1, 0, -1):
        sl, sa = slice(i * w, (i + 1) * w), slice((i - 1) * w, i * w)
        Gt, bG = g[:, sl] + dU, np.abs(g[:, sl]) + bU
        A = y[:, sl] if nscale is None else np.asarray(a, np.float64)[:, sa]
        sc = 1.0 if nscale is None else np.asarray(nscale, np.float64)[i - 1]
        mask = (A > 0) if relu else 1.0
        dZ, bZ = Gt * sc * mask, bG * np.abs(sc) * mask
        U = x[:, sl] + y[:, sa] if i >= 2 else x[:, sl]
        for o, k, v in ((out, "gt", Gt), (bnd, "gt", bG)):
            o[k][:, sa] = v
        for o, Gv, Zv, Av, Uv, Wv in ((out, Gt, dZ, A, U, W[i - 1]), (bnd, bG, bZ, np.abs(A), np.abs(U), np.abs(W[i - 1]))):
            o["dnshift"][i - 1], o["dnscale"][i - 1], o["dbias"][i - 1] = Gv.sum(0), (Gv * Av).sum(0), Zv.sum(0)
            o["dW"][i - 1] = np.einsum("nki,no->kio", Uv[rows], Zv)
            o["dx"][:, sl] = sum(S @ Wv[k].T for k, S in enumerate(shifted(Zv, d)))
        dU, bU = out["dx"][:, sl], bnd["dx"][:, sl]
    return out, bnd


def restatement(x, W, bias, nsc, nsh, s, d, relu=True):
    """x (n, C), W (s-1, 3, w, w), bias / nsc / nsh (s-1, w) or None, fp64 torch -> y (n, C), a (n, (s-1) w)."""
    w = x.shape[1] // s
    ys, acts = [x[:, :w]], []
    for i in range(1, s):
        u = x[:, i * w:(i + 1) * w] + (ys[-1] if i >= 2 else 0.0)
        padded = torch.nn.functional.pad(u.T[None], (d, d), mode="replicate")
        z = torch.nn.functional.conv1d(padded, W[i - 1].permute(2, 1, 0), None if bias is None else bias[i - 1], dilation=d)[0].T
        acts.append(z.clamp(min=0) if relu else z)
        ys.append(acts[-1] if nsc is None else acts[-1] * nsc[i - 1] + nsh[i - 1])
    return torch.cat(ys, 1), torch.cat(acts, 1)
