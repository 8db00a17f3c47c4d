/*
 * ktf_attn.h -- attentive statistics pooling (Okabe et al. 2018) in its single-head, multi-head and channel-wise forms, forward and
 * backward, on the GPU. Entry points of libktf_hip.so next to those of ktf_hip.h, whose conventions and error codes hold here too
 * (kernels: csrc/attn_pool.hip). The attention logits are an input: the two affines
 * that produce them are ktf_tdnn calls.
 *
 * x is fp32 (B, T, ldx) with D channels, e is fp32 (B, T, lde) with H heads of attention logits, 1 <= H <= D and D % H == 0. Channel c
 * belongs to head j(c) = c / (D / H): H = 1 is one weight per frame, H = D one per frame and channel. `lens` is B int32 on the device
 * or NULL; len_b = lens ? clamp(lens[b], 0, T) : T. All arithmetic is fp64 on the fp32 inputs, every operation rounded on its own (no
 * fused multiply-add), every fp32 output rounded once.
 *   1. Rows t >= len_b of x and e, and the columns [D, ldx) and [H, lde), are never read. They may hold NaN.
 *   2. m[b,j] = max_{t < len_b} e[b,t,j] (-inf when len_b = 0).
 *   3. p[t,j] = exp((double)e[b,t,j] - m[b,j]), Z[b,j] = sum_t p[t,j]. The backward uses w[t,j] = p[t,j] * (1 / Z[b,j]).
 *   4. mu_c = (sum_t p[t,j(c)] * x[t,c]) / Z_j, q_c = (sum_t p[t,j(c)] * (x[t,c] * x[t,c])) / Z_j (the square is exact in fp64).
 *   5. out[b,c] = (float)mu_c.
 *   6. With include_std, out[b,D+c] = (float)sqrt(max(q_c - mu_c * mu_c, 0) + (double)eps); a NaN variance stays NaN.
 *   7. Columns of out beyond D (or 2 D) are left untouched.
 *   8. Every sum over t is formed in one order and association: row t goes to group t mod 64, a group adds its rows in ascending
 *      order starting from +0, the 64 groups are combined as ((g + g+16) + g+32) + g+48 for g = 0..15 and these sixteen are added in
 *      ascending g. This does not depend on B, on the position of the utterance in the batch, on T beyond len_b, on the strides, on
 *      the alignment of any pointer or on the launch shape the library picks (it has two and chooses by the size of the grid).
 *   9. No floating-point atomics. The same call twice gives the same bits; an utterance alone and in a batch gives the same bits.
 *  10. len_b = 0: Z = 0, and the row of out is 0 / 0 through rules 5 and 6, which is what ktf_stats_pool writes for such an
 *      utterance. Its rows of dx and de are zero.
 *  11. Side outputs of the forward: norm (B, H, 2) fp64 holding m, Z (required: the x pass reads it), stats (B, 2, D) fp64 holding
 *      mu, q (may be NULL for inference; the backward needs it).
 *  12. Backward, given gout (B, ld_gout) = the gradient of out: var_c = q_c - mu_c * mu_c, sigma_c = sqrt(max(var_c, 0) + eps),
 *      live_c = include_std && var_c > 0; with gmu = gout[b,c], gsig = gout[b,D+c]:
 *        a_c = live ? gmu - (gsig * mu_c) / sigma_c : gmu,   b_c = live ? gsig / (2 * sigma_c) : 0,
 *        dx[b,t,c] = (float)(w[t,j(c)] * (a_c + (2 * b_c) * x[t,c])),
 *        de[b,t,j] = (float)(w[t,j] * (S[t,j] - K[b,j])),  S[t,j] = sum_{c in j} (a_c * x[t,c] + b_c * (x[t,c] * x[t,c])),
 *        K[b,j] = sum_{c in j} (a_c * mu_c + b_c * q_c).
 *      K is the softmax's sum_t w * dL/dw in closed form: the backward has no sum over t and is one pass over x and e. Both sums over
 *      the channels of a head are formed in one order: slot l of 64 adds the head's channels l, l + 64, ... in ascending order
 *      starting from +0, and the 64 slots are added by a butterfly over the distances 32, 16, 8, 4, 2, 1. Rows t in [len_b, T) of dx
 *      and de and the pad columns [D, ld_dx) and [H, ld_de) of every row are written as zero. norm and stats must be those the
 *      forward wrote for the same x, e, lens, include_std and eps. dx and de must not overlap x or e.
 *  13. Refused (KTF_EINVAL, before any launch, no GPU needed): a null out or norm, a null x or e unless T = 0 (forward); a null x, e,
 *      norm, stats, gout, dx, de or workspace (backward); D < 1, H < 1, H > D or D % H != 0; ldx < D or lde < H; ld_out or ld_gout
 *      below D (2 D with include_std); ld_dx < D or ld_de < H; eps negative or not finite; B < 0, T < 0, B above KTF_ATTN_MAX_BATCH,
 *      T above KTF_ATTN_MAX_ROWS, D above KTF_ATTN_MAX_DIM (what the grids index); a workspace below
 *      ktf_attn_pool_backward_workspace_bytes or not 256-byte aligned. Elements are addressed in 64 bits.
 */
#ifndef KTF_ATTN_H_
#define KTF_ATTN_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_ATTN_MAX_BATCH 65535          /* utterances per call */
#define KTF_ATTN_MAX_ROWS 1073741824      /* 2^30: frames per utterance */
#define KTF_ATTN_MAX_DIM 1048576          /* 2^20: channels */

/* Rules 1 - 11. B = 0: nothing is launched. */
int ktf_attn_pool(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const float* e, int32_t H, int64_t lde, const int32_t* lens,
                  int32_t include_std, float eps, float* out, int64_t ld_out, double* norm, double* stats, void* stream);

/* Bytes of the workspace the backward call takes: al256(max(B, 1) * 2 * D * 8) for a, b plus al256(max(B, 1) * H * 8) for K (al256:
 * rounded up to a multiple of 256). Never 0; a negative KTF_* code on bad sizes. */
int64_t ktf_attn_pool_backward_workspace_bytes(int64_t B, int32_t D, int32_t H);

/* Rule 12. B = 0 or T = 0: nothing is launched. */
int ktf_attn_pool_backward(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const float* e, int32_t H, int64_t lde,
                           const int32_t* lens, int32_t include_std, float eps, const double* norm, const double* stats, const float* gout,
                           int64_t ld_gout, float* dx, int64_t ld_dx, float* de, int64_t ld_de, void* workspace, size_t workspace_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
