/*
 * ktf_res2.h -- the hierarchical, grouped, dilated convolution of a Res2Net block (Gao et al. 2019; the frame-level core of the
 * ECAPA / Res2Net-TDNN family) as ONE launch, inference only. Entry points of libktf_hip.so next to those of ktf_hip.h, whose
 * conventions and error codes hold here too (kernel: csrc/res2_conv.hip).
 *
 * x is fp32 (B, T, ldx) with C = scale * wd channels: `scale` groups of width wd, 2 <= scale <= 8, wd % 16 == 0, 16 <= wd <= 128.
 * `dilation` d is 1 .. 8. `lens` is B int32 on the device or NULL; len_b = lens ? clamp(lens[b], 0, T) : T. X_i = x[..., i wd : (i+1) wd].
 *     Y_0 = X_0, copied bit for bit.
 *     U_1 = X_1; U_i = X_i + Y_{i-1} for i >= 2: one fp32 add, rounded once.
 *     Z_i[t] = bias_i + sum_{k in 0,1,2} U_i[clamp(t + (k-1) d, 0, len_b - 1)] W_i[k],  W_i[k] of shape (wd, wd) as [c_in][c_out], i = 1 .. scale-1
 *              (the edge rule of a TDNN layer with SAME padding: the edge row is replicated).
 *     Y_i = act(Z_i) * nscale_i + nshift_i: act is ReLU (v < 0 ? 0 : v, NaN stays NaN) or none; nscale / nshift are the folded inference
 *              BatchNorm, one fp32 multiply then one fp32 add (no fused multiply-add), not applied at all when both are NULL.
 *     y = concat(Y_0 .. Y_{scale-1}), fp32 (B, T, ldy).
 * w is (scale-1, 3 wd, wd) fp32: [g][k wd + c_in][c_out] with g = i - 1; bias, nscale, nshift are (scale-1, wd) fp32.
 *
 *   1. Rows t >= len_b of x and the columns [C, ldx) are never read. They may hold NaN.
 *   2. Rows t >= len_b of y and the columns [C, ldy) are left untouched.
 *   3. Modes. `gemm` is KTF_GEMM_F32, KTF_GEMM_BF16 or KTF_GEMM_BF16X3. The reduction index q = k wd + c_in (0 .. 3 wd - 1, padded with
 *      zero products to a multiple of 32) is cut into chunks of 32 taken in ascending order; an element's accumulator starts from +0
 *      and the bias is added to the finished sum. F32: a chunk is eight v_mfma_f32_16x16x4_f32, step s = 0 .. 7 multiplying the four
 *      q = 32 chunk + 8 h + s, h = 0 .. 3 -- exact fp32 products, fp32 accumulation. BF16: U and W are rounded to bf16 (nearest even) in
 *      registers and a chunk is one v_mfma_f32_16x16x32_bf16. BF16X3: each is split into hi = bf16(a), lo = bf16(a - hi) in registers
 *      and a chunk is three of them: U_hi W_hi, U_lo W_hi, U_hi W_lo, accumulated in fp32 in that order. No 16-bit copy of an operand
 *      exists in memory. This order is every element's: it does not depend on where the element's row lies in a tile or its halo, on
 *      B, on the position of the utterance in the batch, on T beyond len_b, on ldx, ldy or the alignment of any pointer. An utterance
 *      alone and in a batch gives the same bits.
 *   4. No atomics. The same call twice gives the same bits.
 *   5. len_b = 0: nothing of that utterance is read or written. B = 0 or T = 0: nothing is launched.
 *   6. Refused (KTF_EINVAL, before any launch, no GPU needed): a null x, y or w with B T > 0; scale outside 2 .. 8, C % scale != 0,
 *      wd = C / scale not a multiple of 16 in 16 .. 128, dilation outside 1 .. 8; ldx < C, ldy < C, ldx % 4 or ldy % 4; only one of
 *      nscale / nshift; an act other than KTF_ACT_NONE / KTF_ACT_RELU; a gemm other than the three of rule 3; B above
 *      KTF_RES2_MAX_BATCH, T above KTF_RES2_MAX_ROWS, a negative size, a leading dimension at or beyond 2^31; y (the whole of its rows,
 *      pad columns included) overlapping x. Elements are addressed in 64 bits.
 */
#ifndef KTF_RES2_H_
#define KTF_RES2_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_RES2_MAX_BATCH 65535          /* utterances per call */
#define KTF_RES2_MAX_ROWS 1073741824      /* 2^30: frames per utterance */

int ktf_res2_conv(const float* x, int64_t B, int64_t T, int32_t C, int64_t ldx, const int32_t* lens, int32_t scale, int32_t dilation,
                  const float* w, const float* bias, const float* nscale, const float* nshift, int32_t act, int32_t gemm, float* y,
                  int64_t ldy, void* stream);

/* Output rows per workgroup (R) that ktf_res2_conv uses for this width, scale and dilation: the largest multiple of 16 up to 128
 * whose two row buffers, halo included, fit the LDS. A negative KTF_* code on arguments rule 6 refuses. */
int32_t ktf_res2_row_tile(int32_t width, int32_t scale, int32_t dilation, int32_t gemm);

#ifdef __cplusplus
}
#endif
#endif
