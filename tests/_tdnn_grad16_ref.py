"""fp64 NumPy oracle and a-priori bounds of the 16-bit TDNN gradients (include/ktf_grad.h rules 6 - 9), on top of
_tdnn_grad_ref.tdnn_grads (the loops, the term counts n and magnitude sums S) and _tdnn16_ref (bf16 rounding, the split-operand term).

What the kernels are held to, u = 2^-24, per element, all from the reference's own terms:

  "bf16"    the operands are g^ = bf16(g), W^ = bf16(W), x^ = bf16(x) (round to nearest even); every product is exact in fp32, so a sum
            of n of them in any order and grouping, slots included, plus one final rounding is within (n + 2) u S of the fp64 value
            (S = sum of the |products|; _tdnn16_ref item 1). Rows 0 and len - 1 of dx take their clamped terms as a folded sum f of g^
            rows that enters the GEMM as hi = bf16(f), lo = bf16(f - hi): |f - hi - lo| <= 2^-16 |f| <= 2^-16 sum |g^|, which adds
            2^-16 S_fold, S_fold = sum |g^| |W^| over the clamped terms alone (the fp32 additions of the fold are among the n).
  "bf16x3"  the operands are the exact fp32 values; three products per term: (3 n + 2) u 1.02 S for the accumulation (item 1) and
            (3 + 2^-6) 2^-16 S for the hi / lo operands (item 2). A folded A operand is an fp32 sum of at most a handful of g rows: its
            roundings are among the 3 n.
  db        both modes: sums of the unrounded fp32 g, (n + 2) u S.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _tdnn_grad_ref as R  # noqa: E402
from _tdnn16_ref import X3_OPERANDS, bf16_rne  # noqa: E402

U32 = 2.0 ** -24
MODES = ("bf16", "bf16x3")


def operands(x, W, g, mode):
    """The (x, W, g) the products of `mode` are taken of, as float32."""
    if mode == "bf16":
        return bf16_rne(x), bf16_rne(W), bf16_rne(g)
    assert mode == "bf16x3", mode
    return tuple(np.asarray(a, np.float32) for a in (x, W, g))


def fold_magnitudes(W, g, lens, context, sub, padding, shape):
    """S_fold (B, T, D): sum |g| |W| over the (t, k) whose input row was clamped, at the row it was clamped to."""
    W, g = np.abs(np.asarray(W, np.float64)), np.abs(np.asarray(g, np.float64))
    valid = padding.upper() == "VALID"
    out = np.zeros(shape)
    for b in range(shape[0]):
        n = int(lens[b])
        ol, start = R.out_len(n, context, sub, valid)
        for t in range(ol):
            for k, off in enumerate(context):
                row = start + t * sub + off
                if row < 0 or row > n - 1:
                    out[b, min(max(row, 0), n - 1)] += g[b, t] @ W[:, k, :]
    return out


def tdnn_grads16(x, W, g, lens, context, sub=1, padding="SAME", mode="bf16"):
    """-> the dict of _tdnn_grad_ref.tdnn_grads on the operands of `mode`, with db / db_n / db_S from the UNROUNDED g, `dx_S_fold`
    (zeros for "bf16x3": its fold is an operand like any other) and `*_bound` for dx, dW and db."""
    xq, Wq, gq = operands(x, W, g, mode)
    r = R.tdnn_grads(xq, Wq, gq, lens, context, sub, padding)
    g64 = np.asarray(g, np.float32).astype(np.float64)
    valid = padding.upper() == "VALID"
    r["db"], r["db_S"], r["db_n"] = (np.zeros(g64.shape[2]) for _ in range(3))
    for b in range(g64.shape[0]):
        ol = R.out_len(int(lens[b]), context, sub, valid)[0]
        r["db"] += g64[b, :ol].sum(0)
        r["db_S"] += np.abs(g64[b, :ol]).sum(0)
        r["db_n"] += ol
    r["db_bound"] = (r["db_n"] + 2) * U32 * r["db_S"]
    if mode == "bf16":
        r["dx_S_fold"] = fold_magnitudes(Wq, gq, lens, context, sub, padding, r["dx"].shape)
        r["dx_bound"] = (r["dx_n"] + 2) * U32 * r["dx_S"] + 2.0 ** -16 * r["dx_S_fold"]
        r["dW_bound"] = (r["dW_n"] + 2) * U32 * r["dW_S"]
    else:
        r["dx_S_fold"] = np.zeros(r["dx"].shape)
        for k in ("dx", "dW"):
            r[k + "_bound"] = (3 * r[k + "_n"] + 2) * U32 * 1.02 * r[k + "_S"] + X3_OPERANDS * r[k + "_S"]
    return r
