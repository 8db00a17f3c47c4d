/*
 * ktf_loss.h -- the speaker classification head's loss in training: the inverse row norms of a cosine head and the (margin) softmax
 * cross entropy over its logits, forward and backward, on the GPU. Entry points of libktf_hip.so next to those of ktf_hip.h, whose
 * conventions and error codes hold here too (kernels: csrc/loss_train.hip). The GEMM
 * of the head is ktf_tdnn / ktf_grad_tdnn*: these calls are what stands around it.
 *
 * Inverse norms. x is fp32 (rows, ldx), ldx >= D; inv, ginv are `rows` floats.
 *   N1. ktf_loss_row_inv_norm: s = sum_d x[r,d]^2 in fp64 (the squares are exact there), inv[r] = (float)(1 / max(sqrt(s), eps)):
 *       rounded once. Lane l of the row's wave adds the columns l, l + 64, ... in ascending order; the 64 lanes are then added by a
 *       butterfly over the lane distances 32, 16, 8, 4, 2, 1.
 *   N2. ktf_loss_row_inv_norm_backward: dx[r,d] = (float)((-(double)ginv[r] * inv[r]^3) * x[r,d]) with inv[r]^3 = (inv * inv) * inv in
 *       fp64, rounded once; a row whose forward was clamped (sqrt(s) < eps, s summed again as in N1) gets dx = 0 and its ginv is not
 *       read into any result. Columns [D, lddx) of dx are written as zero; columns [D, ldx) of x are never read. dx must not overlap x.
 *
 * Loss. z is fp32 (B, ldz), ldz >= N: the raw dot products x_b . w_j of the affine. `labels` is B int32 on the device. inv_x (B floats)
 * and inv_w (N floats) are both given (cosine head) or both NULL (plain head). kind is one of KTF_LOSS_*. All arithmetic is fp64 on the
 * fp32 inputs, every operation rounded on its own (no fused multiply-add), every output rounded once.
 *   1. Cosine. c_j = ((double)z_j * inv_x[b]) * inv_w[j] for a cosine head, c_j = z_j for a plain one.
 *   2. Valid rows. A row is valid when 0 <= labels[b] < N; any other label marks an ignored row: loss[b] = 0, a zero row of dz, no
 *      contribution to dinv_x (its element is zero) or dinv_w. gloss[b] of an ignored row is not read into any result.
 *   3. Target function psi on the target column y = labels[b] of a valid row. SOFTMAX: psi(c) = c (margin must be 0). AM:
 *      psi(c) = c - m. AAM: with cm = cos m, sm = sin m evaluated once on the host in double and
 *      S(c) = sqrt(max(1 - c * c, KTF_LOSS_SIN2_FLOOR)): psi(c) = c * cm - S(c) * sm where c > -cm, psi(c) = c - m * sm otherwise
 *      (the non-"easy-margin" fallback beyond theta = pi - m). psi' is the derivative of exactly this function: 1 for SOFTMAX and AM
 *      and on the fallback branch, cm + sm * c / S(c) where 1 - c * c > KTF_LOSS_SIN2_FLOOR, cm where the floor holds. The floor also
 *      absorbs |c| marginally above 1: c is not clipped.
 *   4. Logits. l_j = scale * c_j for j != y, l_y = scale * psi(c_y); an ignored row uses scale * c_j throughout.
 *      lse[b] = M + log(sum_j exp(l_j - M)), M = max_j l_j, written as fp64 (B doubles) for every row; loss[b] = (float)(lse[b] - l_y).
 *   5. Prediction. pred[b] (int32) = the lowest index attaining max_j c_j (the cosine without margin), for ignored rows too. pred may
 *      be NULL.
 *   6. Backward. p_j = exp(l_j - lse[b]); gloss is B floats, NULL = all ones.
 *      dc_j = (((double)gloss[b] * scale) * (p_j - [j = y])) * (j = y ? psi'(c_y) : 1);
 *      dz[b,j] = (float)((dc_j * inv_x[b]) * inv_w[j]), or (float)dc_j for a plain head;
 *      dinv_x[b] = (float) sum_j (dc_j * z_j) * inv_w[j];  dinv_w[j] = (float) sum_b (dc_j * z_j) * inv_x[b]:
 *      the partial derivatives of sum_b gloss[b] * loss[b] with respect to z, inv_x and inv_w. dinv_x and dinv_w are both given for a
 *      cosine head and both NULL for a plain one. dz may be exactly z (same pointer and leading dimension): the gradient then
 *      overwrites the logits; any other overlap of dz with z is refused. Columns [N, lddz) of dz are written as zero; columns
 *      [N, ldz) of z are never read (NaN allowed). lse, labels, inv_x, inv_w, kind, margin and scale must be those of the forward call.
 *   7. No floating-point atomics. A workgroup has KTF_LOSS_CHUNK_COLS threads; thread t of the forward call takes the columns
 *      t, t + 256, ... of its row in ascending order, the 64 lanes of a wave are added by a butterfly over the lane distances
 *      32, 16, 8, 4, 2, 1 and the four waves in ascending order. The backward call cuts the columns into chunks of
 *      KTF_LOSS_CHUNK_COLS and the rows into blocks of ktf_loss_slot_rows(): a row's sum for dinv_x is formed per chunk (butterfly,
 *      then the four waves in ascending order; columns at and beyond N add +0) and the chunks are added in ascending order; a
 *      column's sum for dinv_w adds the valid rows of a block in ascending order into a workspace slot of the block's own, and the
 *      slots are added in ascending order. The same call twice gives the same bits.
 *   8. Alignment. There is one path: every row is read and written four bytes per lane, consecutive lanes on consecutive columns
 *      (256 contiguous bytes per wave and instruction), whatever the base pointer and the leading dimension, so a contiguous
 *      (B, N) tensor with odd N runs as fast as a padded one and the values do not depend on the alignment.
 *   9. Degenerate cases. B = 0: nothing is launched and dinv_w (if given) is written as zero. N = 1: loss = 0 and dz = 0 exactly.
 *  10. Refused (KTF_EINVAL, before any launch, no GPU needed): a null z, labels, loss, lse or workspace (forward), a null z, labels,
 *      lse, dz or workspace (backward), a null x, inv, ginv or dx; exactly one of inv_x / inv_w; exactly one of dinv_x / dinv_w, or
 *      one that does not go with the head; AM or AAM on a plain head; a non-zero margin with SOFTMAX; scale <= 0 or not finite;
 *      margin not finite, < 0, or >= pi / 2 for AAM; an unknown kind; B < 0, rows < 0, N < 1, D < 1; a leading dimension below N
 *      (or D); eps <= 0 or not finite; a workspace below ktf_loss_workspace_bytes or not 256-byte aligned; dz overlapping z other
 *      than exactly, dx overlapping x; B, rows, N, D or a leading dimension at or beyond 2^31, or
 *      ceil(B / slot_rows) * ceil(ld / KTF_LOSS_CHUNK_COLS) at or beyond 2^31 (the backward grid, ld = lddz; N in
 *      ktf_loss_workspace_bytes and the forward call). Elements are addressed in 64 bits.
 */
#ifndef KTF_LOSS_H_
#define KTF_LOSS_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_LOSS_SOFTMAX 0        /* psi(c) = c */
#define KTF_LOSS_AM 1             /* additive margin (CosFace) */
#define KTF_LOSS_AAM 2            /* additive angular margin (ArcFace) */
#define KTF_LOSS_SIN2_FLOOR 9.5367431640625e-07   /* 2^-20: the floor of 1 - c^2 under the square root (rule 3) */
#define KTF_LOSS_SLOT_ROWS 8      /* batch rows per slot of partial sums of dinv_w (rule 7) */
#define KTF_LOSS_CHUNK_COLS 256   /* columns per workgroup of the backward call (rule 7) */

/* KTF_LOSS_SLOT_ROWS, for callers that do not read the header. */
int32_t ktf_loss_slot_rows(void);

/* Bytes of the workspace either loss call takes for a (B, N) batch: al256(max(ceil(B / KTF_LOSS_SLOT_ROWS), 1) * N * 8) for the slots
 * plus al256(ceil(N / KTF_LOSS_CHUNK_COLS) * max(B, 1) * 8) for the rows' sums per chunk (al256: rounded up to a multiple of 256).
 * Never 0; a negative KTF_* code on bad arguments (B < 0, N < 1, the limits of rule 10). The forward call checks the workspace and
 * leaves it untouched; both calls may share one on one stream. */
int64_t ktf_loss_workspace_bytes(int64_t B, int64_t N);

/* Rule N1. */
int ktf_loss_row_inv_norm(const float* x, int64_t ldx, int64_t rows, int64_t D, double eps, float* inv, void* stream);

/* Rule N2. */
int ktf_loss_row_inv_norm_backward(const float* x, int64_t ldx, int64_t rows, int64_t D, double eps, const float* inv, const float* ginv,
                                   float* dx, int64_t lddx, void* stream);

/* Rules 1 - 5. */
int ktf_loss_margin_softmax_forward(const float* z, int64_t ldz, int64_t B, int64_t N, const int32_t* labels, const float* inv_x,
                                    const float* inv_w, int32_t kind, double margin, double scale, float* loss, int32_t* pred, double* lse,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* Rule 6. */
int ktf_loss_margin_softmax_backward(const float* z, int64_t ldz, int64_t B, int64_t N, const int32_t* labels, const float* inv_x,
                                     const float* inv_w, int32_t kind, double margin, double scale, const double* lse, const float* gloss,
                                     float* dz, int64_t lddz, float* dinv_x, float* dinv_w, void* workspace, size_t workspace_bytes,
                                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
