/*
 * ktf_agg.h -- multi-layer feature aggregation (Desplanques et al. 2020, ECAPA-TDNN): the 1 x 1 convolution over the channel-wise
 * concatenation of S frame-level tensors as ONE launch that never forms the concatenation. Entry points of libktf_hip.so next to those
 * of ktf_hip.h, whose conventions and error codes hold here too (kernel: csrc/agg_conv.hip, DESIGN.md
 * section 7).
 *
 *     z[b,t,u] = sum_{s<S} sum_{c<C_s} x_s[b,t,c] * w[u, off_s + c]       off_s = C_0 + ... + C_{s-1},  K = off_S
 *     y[b,t,u] = act(z + bias[u]) * nscale[u] + nshift[u]                 t < len_b, u < units
 *
 * x_s is fp32 (B, T, ldx_s): every source has its own base pointer and leading dimension, 2 <= S <= 4. w is fp32 (units, ldw),
 * row-major with ldw >= K, read as it stands in memory: the layout of a Conv1d(K, units, 1) weight. bias, nscale, nshift hold `units`
 * floats each or are NULL, nscale and nshift both or neither (the folded inference BatchNorm). act is KTF_ACT_NONE or KTF_ACT_RELU
 * (v < 0 ? 0 : v, NaN stays NaN). y is fp32 (B, T, ldy). `lens` is B int32 on the device or NULL; len_b = lens ? clamp(lens[b], 0, T) : T.
 * The source table -- xs, widths, ldxs -- is three host arrays of length S, read at call time; they travel as kernel arguments and
 * there is no device-side table.
 *
 *   1. Rows t >= len_b and the pad columns [C_s, ldx_s) of every source, and the columns [K, ldw) of w, are never read. They may hold
 *      NaN.
 *   2. Rows t >= len_b and the columns [units, ldy) of y are left untouched.
 *   3. len_b = 0: nothing of that utterance is read or written. B T = 0: nothing is launched.
 *   4. Order of the sum: rule 3 of ktf_res2.h, taken over. The reduction index q = off_s + c runs in concatenation order, cut into
 *      chunks of 32 taken ascending; an element's accumulator starts from +0; the bias is added to the finished sum; then act, one
 *      fp32 multiply and one fp32 add (no fused multiply-add; neither with both norm pointers NULL). `gemm` is KTF_GEMM_F32 (a chunk
 *      is eight v_mfma_f32_16x16x4_f32, step e = 0 .. 7 multiplying the four q = 32 chunk + 8 h + e, h = 0 .. 3), KTF_GEMM_BF16 (x
 *      and w rounded to bf16, nearest even, in registers; a chunk is one v_mfma_f32_16x16x32_bf16) or KTF_GEMM_BF16X3 (each split
 *      into hi = bf16(a), lo = bf16(a - hi) in registers; a chunk is three of them: x_hi w_hi, x_lo w_hi, x_hi w_lo, in that order).
 *      No 16-bit copy of an operand exists in memory.
 *   5. Independence. The order is every element's own: it does not depend on the tile, on B, on the position of the utterance in the
 *      batch, on T beyond len_b, on any leading dimension or pointer alignment, or on how K is divided among the sources. Because
 *      C_s % 32 == 0 a chunk never straddles two sources.
 *   6. No atomics. The same call twice gives the same bits. An utterance alone and in a batch gives the same bits.
 *   7. Refused (KTF_EINVAL, before any launch, no GPU needed): S outside 2 .. KTF_AGG_MAX_SOURCES; a C_s that is not a multiple of 32 in
 *      32 .. KTF_AGG_MAX_WIDTH; units outside 1 .. KTF_AGG_MAX_UNITS; a leading dimension (ldx_s, ldw, ldy) below its width, not a
 *      multiple of 4 or at 2^31; a null x_s, w or y (or source table) with B T > 0; one of nscale / nshift alone; an act other than
 *      KTF_ACT_NONE / KTF_ACT_RELU; a gemm other than the three of rule 4; B above KTF_AGG_MAX_BATCH, T above KTF_AGG_MAX_ROWS, a
 *      negative size; y (the whole of its rows, pad columns included) overlapping any source. Elements are addressed in 64 bits.
 */
#ifndef KTF_AGG_H_
#define KTF_AGG_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_AGG_MAX_SOURCES 4
#define KTF_AGG_MAX_WIDTH 4096           /* channels of one source */
#define KTF_AGG_MAX_UNITS 8192
#define KTF_AGG_MAX_BATCH 65535          /* utterances per call */
#define KTF_AGG_MAX_ROWS 1073741824      /* 2^30: frames per utterance */

int ktf_agg_conv(const float* const* xs, const int32_t* widths, const int64_t* ldxs, int32_t S, int64_t B, int64_t T, const int32_t* lens,
                 const float* w, int64_t ldw, const float* bias, const float* nscale, const float* nshift, int32_t units, int32_t act,
                 int32_t gemm, float* y, int64_t ldy, void* stream);

/* Output rows per workgroup (R) that ktf_agg_conv uses for `units` outputs over K = sum C_s concatenated channels (a multiple of 32
 * in 64 .. KTF_AGG_MAX_SOURCES * KTF_AGG_MAX_WIDTH). A negative KTF_* code on arguments rule 7 refuses. */
int32_t ktf_agg_row_tile(int32_t units, int32_t K, int32_t gemm);

#ifdef __cplusplus
}
#endif
#endif
