/*
 * ktf_gctx.h -- global-context attention for attentive statistics pooling (Desplanques et al. 2020, ECAPA-TDNN): the attention reads
 * the frame concatenated with its utterance's mean and standard deviation, [x_t ; mu_b ; sigma_b]. Entry points of libktf_hip.so next
 * to those of ktf_hip.h, whose conventions and error codes hold here too (kernels: csrc/attn_ctx.hip,
 * DESIGN.md section 7). The context part of the first affine is constant over an utterance,
 *
 *     W1^T [x_t ; mu_b ; sigma_b] + b1  =  W1x^T x_t + g_b,      g_b = b1 + W1c[0:D]^T mu_b + W1c[D:2D]^T sigma_b,
 *     e[b,t,:] = W2^T act(W1x^T x[b,t,:] + g_b) + b2,            t < len_b,
 *
 * so no (B, T, 3 D) tensor is formed: ktf_gctx_stats writes mu and sigma, ktf_gctx_bias the per-utterance bias g, ktf_gctx_logits the
 * logits in one launch whose hidden tile never leaves the compute unit. The pooling of ktf_attn.h takes e from there.
 *
 * x is fp32 (B, T, ldx) with D channels. W1x is fp32 (D, A) and W1c fp32 (2 D, A), both row-major with a leading dimension (the rows
 * [0, D) and [D, 3 D) of one (3 D, A) matrix will do); W2 is fp32 (A, H) row-major with a leading dimension; b1 holds A floats, b2 H
 * floats (either may be NULL: zeros). ctx is fp64 (B, 2, D) dense, g fp32 (B, ldg), e fp32 (B, T, lde). `lens` is B int32 on the device
 * or NULL; len_b = lens ? clamp(lens[b], 0, T) : T.
 *
 *   1. Rows t >= len_b of x, its pad columns [D, ldx), and the pad columns of W1x, W1c, W2 and g are never read. They may hold NaN.
 *   2. ktf_gctx_stats, with n = len_b, in fp64, every operation rounded on its own (no fused multiply-add):
 *      mu_c = (sum_t x[t,c]) / n, q_c = (sum_t x[t,c] * x[t,c]) / n (the square is exact), sigma_c = sqrt(max(q_c - mu_c * mu_c, 0) + (double)eps);
 *      a NaN variance stays NaN. ctx[b,0,c] = mu_c, ctx[b,1,c] = sigma_c. This sigma is rule 6 of ktf_attn.h under uniform weights.
 *   3. Every sum over t of rule 2 is formed in the order of ktf_attn.h rule 8 (csrc/canon_sum.h): it does not depend on B, on the position of
 *      the utterance in the batch, on T beyond len_b, on ldx, on the alignment of x or on the launch shape.
 *   4. len_b = 0: mu and sigma are 0 / 0 (NaN), the row of g is NaN, and no row of e is written.
 *   5. ktf_gctx_bias: g[b,a] = (float)(b1[a] + sum_{k < 2 D} ctx[b,k] * W1c[k,a]) in fp64 on v_mfma_f64_16x16x4_f64, a tile of 16
 *      utterances per wave: the accumulator starts from b1[a] and takes the terms in ascending k, four per instruction. One order, no
 *      atomics, one rounding to fp32. Columns [A, ldg) of g are left untouched.
 *   6. ktf_gctx_logits: a workgroup owns the rows [t0, t0 + R) of ONE utterance, t0 a multiple of R = ktf_gctx_row_tile(), and every
 *      unit and head of them. h[r,a] = act(sum_{c < D} x[r,c] * W1x[c,a] + g[b,a]) is formed in fp32 and kept in LDS; it is never
 *      written to memory. e[r,j] = sum_{a < A} h[r,a] * W2[a,j] + b2[j]. Either sum runs over chunks of 32 taken ascending, the
 *      accumulator starting from +0; g and b2 are added to the finished sums. act is KTF_ACT_TANH (tanhf) or KTF_ACT_RELU (v < 0 ? 0 : v).
 *   7. `gemm` of ktf_gctx_logits is KTF_GEMM_F32 (a chunk is eight v_mfma_f32_16x16x4_f32, step s = 0 .. 7 multiplying the four
 *      k = 32 chunk + 8 i + s, i = 0 .. 3) or KTF_GEMM_BF16X3 (either operand split into hi = bf16(a), lo = bf16(a - hi) in registers; a
 *      chunk is three v_mfma_f32_16x16x32_bf16: l_hi r_hi, l_lo r_hi, l_hi r_lo, in that order, l the rows, r the weights; lo lo is
 *      dropped). The activated h is split again, from its fp32 value, for the second product. No 16-bit copy of anything exists in
 *      memory. One-pass bf16 is refused: e goes through exp.
 *   8. Rows t >= len_b of e and its columns [H, lde) are left untouched.
 *   9. Independence. The bits of an utterance's ctx, g and e do not depend on B, on its position in the batch, on T beyond len_b, on any
 *      leading dimension or on the alignment of any pointer (operands on 16-byte boundaries with leading dimensions that are multiples
 *      of 4 are fed by LDS-DMA, all others by scalar loads into the same LDS image). No atomics; the same call twice gives the same bits.
 *  10. Refused (KTF_EINVAL, before any launch, no GPU needed): B < 0, T < 0, B above KTF_GCTX_MAX_BATCH, T above KTF_GCTX_MAX_ROWS; D
 *      outside 1 .. KTF_GCTX_MAX_DIM; A outside 1 .. KTF_GCTX_MAX_UNITS; H outside 1 .. KTF_GCTX_MAX_DIM; ldx < D, ldw1 < A, ldw < A,
 *      ldg < A, ldw2 < H, lde < H, or a leading dimension at 2^31; eps negative or not finite; an act other than KTF_ACT_TANH /
 *      KTF_ACT_RELU; a gemm other than KTF_GEMM_F32 / KTF_GEMM_BF16X3; a null ctx (stats); a null x with B T > 0 (stats, logits); a null
 *      ctx, W1c or g with B > 0 (bias); a null W1x, g, W2 or e with B T > 0 (logits). Elements are addressed in 64 bits.
 */
#ifndef KTF_GCTX_H_
#define KTF_GCTX_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_GCTX_MAX_UNITS 256            /* A: the hidden tile of a workgroup holds every unit */
#define KTF_GCTX_MAX_BATCH 65535          /* utterances per call   (KTF_ATTN_MAX_BATCH) */
#define KTF_GCTX_MAX_ROWS 1073741824      /* 2^30: frames per utterance   (KTF_ATTN_MAX_ROWS) */
#define KTF_GCTX_MAX_DIM 1048576          /* 2^20: channels, heads   (KTF_ATTN_MAX_DIM) */

/* Rules 1 - 4. B = 0: nothing is launched. */
int ktf_gctx_stats(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const int32_t* lens, float eps, double* ctx, void* stream);

/* Rule 5. B = 0: nothing is launched. */
int ktf_gctx_bias(const double* ctx, int64_t B, int32_t D, const float* w1c, int64_t ldw, const float* b1, int32_t A, float* g, int64_t ldg,
                  void* stream);

/* Rules 6 - 9. B T = 0: nothing is launched. */
int ktf_gctx_logits(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const int32_t* lens, const float* w1x, int64_t ldw1,
                    const float* g, int64_t ldg, int32_t A, int32_t act, const float* w2, int64_t ldw2, const float* b2, int32_t H,
                    int32_t gemm, float* e, int64_t lde, void* stream);

/* Rows per workgroup (R of rule 6) that ktf_gctx_logits uses for A units and H heads. A negative KTF_* code on arguments rule 10 refuses. */
int32_t ktf_gctx_row_tile(int32_t A, int32_t H, int32_t gemm);

#ifdef __cplusplus
}
#endif
#endif
