/*
 * ktf_res2.h -- the hierarchical, grouped, dilated convolution of a Res2Net block (Gao et al. 2019; the frame-level core of the
 * ECAPA / Res2Net-TDNN family) as ONE launch, and its backward (rules 7 - 13) as three. Entry points of libktf_hip.so next to those of
 * ktf_hip.h, whose conventions and error codes hold here too (kernels: csrc/res2_conv.hip and
 * csrc/res2_grad.hip).
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
 *
 * Training (kernels: csrc/res2_grad.hip). A_i = act(Z_i), G_i = dL/dY_i = columns i wd .. of g, walked i = scale-1 .. 1:
 *   7. The training forward takes the forward's arguments and `a`, fp32 (B, T, lda) of (scale-1) wd columns (group i at (i-1) wd):
 *      A_i, the value after the activation and before the norm. a is required exactly when nscale is given and is NULL otherwise;
 *      its rows t >= len_b and columns beyond (scale-1) wd are left untouched. y has the bits of the inference call.
 *   8. Gt_i = G_i + dU_{i+1} (one fp32 add), Gt_{scale-1} = G_{scale-1}. dnshift_i = sum_{b,t} Gt_i, dnscale_i = sum_{b,t} Gt_i A_i.
 *   9. dZ_i = Gt_i nscale_i [A_i > 0]: one fp32 multiply (none without the norm pair), then the mask (1 without ReLU). A_i and the mask
 *      are what the forward saved, never recomputed: a with the norm pair, else Y_i of y. dbias_i = sum_{b,t} dZ_i.
 *  10. dU_i[r] = sum_k S_k[r] W_i[k]^T with S_1[r] = dZ_i[r]; S_0[r] = dZ_i[r+d] for r > 0 and r+d < len; S_0[0] = sum_{t=0}^{min(d,len-1)}
 *      dZ_i[t]; S_2[r] = dZ_i[r-d] for r < len-1 and r-d >= 0; S_2[len-1] = sum_{t=max(len-1-d,0)}^{len-1} dZ_i[t]; every other S row is
 *      zero. The two folded rows are fp32 sums in ascending t (len = 1: both are dZ_i[0]). The product runs as rule 3 with the
 *      reduction index q = k wd + c_out. dX_i = dU_i for i >= 1; dX_0 = G_0 copied bit for bit. Rows t >= len_b of dx are written
 *      as zero in [0, C); its pad columns are left untouched. dx of an utterance has the same bits alone or in a batch, at any
 *      leading dimension or alignment.
 *  11. The data-gradient call also writes `gt`, fp32 (B, T, ldgt) of (scale-1) wd columns: Gt_i, NOT dZ_i, each tile its own rows
 *      (rows t >= len_b untouched). The weights call forms dZ_i from gt, the saved activation and nscale as rule 9 does, so the two
 *      see the same bits, and takes dnscale / dnshift from gt itself.
 *  12. dW_i[k][c_in][c_out] = sum_{b, t < len_b} U_i[b, clamp(t+(k-1)d)][c_in] dZ_i[b,t][c_out], U_i recomputed as the forward's single
 *      fp32 add of x and y. The frames of an utterance are cut into chunks of 32 (the reduction chunk of rule 3; in F32 step s takes
 *      frames 8 h + s); chunks, counted over the batch, are dealt to slots in contiguous runs; a slot accumulates its chunks in
 *      ascending order into a region of its own and a second kernel adds the slots in ascending order. dbias, dnscale and dnshift are
 *      fp32 sums of unrounded values over the same chunks, rows ascending, then slots ascending. The slot count is
 *      min(B ceil(T / 32), clamp(ceil(768 / (3 (scale-1))), 32, 64)): a function of (B, T, wd, scale), never of lens.
 *  13. No atomics; the same call twice gives the same bits. Rows t >= len_b and pad columns of every input are never read. An empty
 *      utterance contributes nothing. B T = 0: only the zero fill of dw, dbias, dnscale, dnshift is launched. Refused (KTF_EINVAL,
 *      before any launch): what rule 6 refuses; a missing or misplaced a; a leading dimension below its width, not a multiple of 4
 *      or at 2^31; dnscale / dnshift without nscale; scratch below the float count the query gives; an output overlapping an input.
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

/* The forward for training (rule 7). */
int ktf_res2_conv_train(const float* x, int64_t B, int64_t T, int32_t C, int64_t ldx, const int32_t* lens, int32_t scale, int32_t dilation,
                        const float* w, const float* bias, const float* nscale, const float* nshift, int32_t act, int32_t gemm, float* y,
                        int64_t ldy, float* a, int64_t lda, void* stream);

/* Rows of dx per workgroup of the data gradient: the largest multiple of 16 up to 128 whose two row buffers, halo included, and three
 * edge rows fit the LDS. */
int32_t ktf_res2_grad_row_tile(int32_t width, int32_t scale, int32_t dilation, int32_t gemm);

/* Slots of the weights call (rule 12), and the floats of scratch it takes: slots * (scale-1) * 3 * wd * (wd + 1). */
int32_t ktf_res2_grad_slots(int64_t B, int64_t T, int32_t width, int32_t scale);
int32_t ktf_res2_grad_scratch_floats(int64_t B, int64_t T, int32_t width, int32_t scale);

/* g (B, T, ldg) -> dx (B, T, lddx) and gt (B, T, ldgt), one launch (rules 8 - 11). y and a are the training forward's. */
int ktf_res2_grad_data(const float* g, int64_t B, int64_t T, int32_t C, int64_t ldg, const int32_t* lens, int32_t scale, int32_t dilation,
                       const float* w, const float* nscale, const float* y, int64_t ldy, const float* a, int64_t lda, int32_t act,
                       int32_t gemm, float* dx, int64_t lddx, float* gt, int64_t ldgt, void* stream);

/* dw (scale-1, 3 wd, wd), dbias, dnscale, dnshift (scale-1, wd; each may be NULL) from x, y, a and the gt of the data call (rule 12). */
int ktf_res2_grad_weights(const float* x, int64_t B, int64_t T, int32_t C, int64_t ldx, const int32_t* lens, int32_t scale,
                          int32_t dilation, const float* nscale, const float* y, int64_t ldy, const float* a, int64_t lda,
                          const float* gt, int64_t ldgt, int32_t act, int32_t gemm, float* dw, float* dbias, float* dnscale,
                          float* dnshift, float* scratch, int64_t scratch_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif
