"""fp64 reference and error bounds for the fp32 and bf16-pair TDNN kernels (csrc/tdnn_f32.hip, csrc/tdnn_pair.hip), on top of
tests/_tdnn16_ref.py (numpy only; no GPU, no torch): the same `case` dicts (those of tests/test_gpu_tdnn32_bits.py), the same Ref, the
same comparisons (`check`), the same epilogue terms; only the operands and the accumulation term are these families' own.

Operands: what the kernel sees. KTF_GEMM_F32 -- the fp32 x and W as they are. KTF_GEMM_BF16X4 -- the values the KTF_BF16P pairs hold,
hi + lo with hi = bf16(a), lo = bf16(a - hi), both round to nearest even (ops.pair_encode; an exact sum in fp64). The pair split itself
(|a - hi - lo| <= 2^-16 |a|) is therefore NOT part of the budget: tests/test_gpu_round4.py measures it against the exact operands.

The bound on the pre-activation value z, u = 2^-24, K = Ktot products, A = sum |x| |w| over them (from the reference's own terms):
  KTF_GEMM_F32: v_mfma_f32_32x32x2_f32 / 16x16x4_f32 and the row-vector kernel's fmaf chain add the K products in K order, one
    rounding per fused multiply-add: first-order error at most K u A, for the partial sums never exceed A. The bias is added in the
    epilogue (one more rounding of a value of at most A + |bias|), and (1 + u)^(K + 1) - 1 < (K + 2) u for K u < 0.01 pays the second
    order:  dz = (K + 2) u (A + |bias|).
  KTF_GEMM_BF16X4: the four partial products of a pair of pairs are exact in fp32 (8 + 8 significand bits) and v_mfma_f32_16x16x32_bf16
    adds 32 of them to an fp32 accumulator per instruction: K / 8 instructions into two accumulators, one addition of the two, one of the
    bias. Their magnitudes sum to A' = sum (|xh| + |xl|) (|wh| + |wl|) >= A. The same (K + 2) u, now of A' + |bias|, allows a rounding per
    VALUE of K where the instruction count alone would ask for K / 8 + 2: the hardware's order inside an instruction is not documented,
    and this leaves it eight roundings per instruction.
Epilogue (activation, the device's expf / tanhf allowance ACT_ULPS, the BatchNorm affine, the bf16 rounding of bf16 rows, the pooled
sums in fp64): items 3 and 4 and the comparisons of tests/_tdnn16_ref.py, unchanged -- the fp32 kernels skip the affine without scale
(exact) and tdnn_x4s_kernel's pooled form adds fp64 values, which the bound for the fp32 pivot sums there covers.

KTF_BF16P rows (`ydt` "pair"): an fp32-sized slot holds hi = bf16(y) in its low half and lo = bf16(y - hi) in its high half. hi is
compared as a bf16 row; |hi + lo - want| <= dy + 2^-16 |want| and |lo| <= half a bf16 ulp of hi, as for the hi / lo planes there.
"""

import numpy as np

import _tdnn16_ref as R

X4 = "x4"
PAIR = "pair"


def pair_values(a):
    """fp32 -> (hi, lo) of its KTF_BF16P pair, as fp32."""
    a = np.ascontiguousarray(a, np.float32)
    hi = R.bf16_rne(a)
    return hi, R.bf16_rne(a - hi)


def dz32(A, b, ktot):
    return (ktot + 2) * R.U32 * (A + b)


def reference(c, x, W, bias, scale=None, shift=None):
    if c["gemm"] != X4:
        return R.reference_on(c, x, W, bias, scale, shift, dz32)
    (xh, xl), (wh, wl) = ((h.astype(np.float64), l.astype(np.float64)) for h, l in (pair_values(x), pair_values(W)))
    return R.reference_on(c, xh + xl, wh + wl, bias, scale, shift, dz32, mag=(np.abs(xh) + np.abs(xl), np.abs(wh) + np.abs(wl)))


def check(c, ref, raw, finalized=None, eps=1e-10):
    """As _tdnn16_ref.check; a KTF_BF16P buffer comes as its float32 words."""
    if c["ydt"] != PAIR or c["mode"] in R.POOLED_MODES:
        return R.check(c, ref, raw, finalized, eps)
    res = R.Result()
    assert raw.dtype == np.float32 and raw.shape == (ref.want.shape[0], ref.Tout, c["ldy"]), (raw.dtype, raw.shape)
    R._untouched(res, "y", raw, c, ref)
    m = R._valid(ref)
    want, bound = ref.want[m], ref.bound[m]
    bits = np.ascontiguousarray(raw[:, :, :c["units"]][m]).view(np.uint32)
    hi = R.bf16_from_bits((bits & 0xFFFF).astype(np.uint16)).astype(np.float64)
    lo = R.bf16_from_bits((bits >> 16).astype(np.uint16)).astype(np.float64)
    res.close("pair rows, hi", hi, want, bound + R.half_ulp_bf16(np.maximum(np.abs(hi), np.abs(want))))
    res.close("pair rows, hi + lo", hi + lo, want, bound + 2.0 ** -16 * np.abs(want))
    res.true("|lo| <= half a bf16 ulp of hi", np.abs(lo) <= R.half_ulp_bf16(hi))
    return res
