/*
 * ktf_head.h -- the classification head's loss with sub-centres, an inter-top-k penalty and label smoothing: a second family of loss
 * calls next to ktf_loss.h, whose rules (cited below as "ktf_loss.h, rule n"), conventions and error codes hold here unless a rule says
 * otherwise (kernels: csrc/loss_train.hip). The inverse norms are those of
 * ktf_loss.h, rules N1 and N2; the GEMM of the head is the affine's. All arithmetic is fp64 on the fp32 inputs, every operation rounded
 * on its own (no fused multiply-add), every output rounded once; no floating-point atomics.
 *
 * z is fp32 (B, ldz), labels B int32, inv_x B floats and inv_w N * K floats, both given (cosine head) or both NULL (plain head). kind,
 * margin and scale are those of ktf_loss.h, rule 3 (KTF_LOSS_SOFTMAX / _AM / _AAM = 0 / 1 / 2).
 *  H1. Sub-centres. ldz >= N * K; column j * K + k is centre k of class j (class-major: K = 1 is the layout of ktf_loss.h).
 *      c_{j,k} = ((double)z[b, jK+k] * inv_x[b]) * inv_w[jK+k] (z itself for a plain head); c_j = max_k c_{j,k} and k*_j the lowest k that
 *      attains it (k ascending, replaced only by a strictly larger value). Everything in ktf_loss.h, rules 1 - 6 (psi, psi', logits,
 *      lse, pred) applies to the N class cosines c_j: lse and pred run over N classes, not over N * K columns. sub_y[b] (int32, may be
 *      NULL) = k*_y of a valid row, -1 of an ignored one. 1 <= K <= KTF_HEAD_MAX_CENTERS; K > 1 needs a cosine head.
 *  H2. Inter-top-k, 0 <= topk <= KTF_HEAD_MAX_TOPK. H_b = the first min(topk, N - 1) classes j != y of valid row b in the order
 *      "c_j descending, then j ascending". The order compares the fp64 c_j themselves, so it is total: there are no ties to break by
 *      rounding, and +0 equals -0. A NaN cosine is never a member. l_j = scale * (c_j + penalty) for j in H_b; the penalty is additive,
 *      so the derivative with respect to c_j stays `scale`. The forward call writes `hard`, int32 (B, max(topk, 1)): the members of H_b
 *      in that order, -1 beyond them, -1 throughout an ignored row (`hard` may be NULL when topk = 0). The backward call reads `hard`
 *      and selects nothing: a class listed there takes the penalty, except the target, whose logit is always scale * psi(c_y); entries
 *      outside [0, N) are skipped. topk > 0 needs a cosine head; penalty >= 0, and 0 when topk = 0. Ignored rows take no penalty.
 *  H3. Label smoothing, 0 <= smoothing = e < 1, plain and cosine heads alike. With l_j the logits after margin and penalties and
 *      mean = (sum_j l_j) / N (the sum in the order of H5):
 *        loss[b] = (float)((lse[b] - l_y) + e * (l_y - mean)),            which is lse - ((1 - e) l_y + e mean) in this exact order;
 *        dc_j = (((double)gloss[b] * scale) * ((p_j - [j = y]) + e * ([j = y] - 1 / (double)N))) * (j = y ? psi'(c_y) : 1),
 *      p_j = exp(l_j - lse[b]). With e = 0 both are the values of ktf_loss.h, rules 4 and 6, bit for bit (the sum is then not formed).
 *  H4. Backward. dz[b, jK+k] = (float)((dc_j * inv_x[b]) * inv_w[jK+k]) for k = k*_j, found again from z ((float)dc_j for a plain
 *      head), exactly +0 for the other centres of the class; columns [N * K, lddz) are written as zero and columns [N * K, ldz) of z
 *      are never read. dinv_x[b] = (float) sum_j (dc_j * z[b, jK+k*]) * inv_w[jK+k*]; dinv_w[jK+k] = (float) of the sum of
 *      (dc_j * z[b, jK+k]) * inv_x[b] over the valid rows b with k*_{b,j} = k, zero for a centre no row selected. Ignored rows behave as
 *      in ktf_loss.h, rule 2 (sub_y = -1, a row of -1 in `hard`). dz may be exactly z (same pointer and leading dimension); any other
 *      overlap is refused. lse, hard and every input must be those of the forward call.
 *  H5. Order of sums: ktf_loss.h, rule 7 with "column" read as "class". A workgroup has KTF_HEAD_CHUNK_CLASSES threads; thread t of
 *      the forward call takes the classes t, t + 256, ... of its row in ascending order (sum_j exp(l_j - M) and sum_j l_j alike), the
 *      64 lanes of a wave are added by a butterfly over the lane distances 32, 16, 8, 4, 2, 1 and the four waves in ascending order.
 *      The backward call cuts the classes into chunks of KTF_HEAD_CHUNK_CLASSES and the rows into blocks of ktf_head_slot_rows(): a
 *      row's sum for dinv_x is formed per chunk and the chunks are added in ascending order; a centre's sum for dinv_w adds the valid
 *      rows of a block in ascending order into a workspace slot of the block's own, and the slots are added in ascending order.
 *      Hence: the same call twice gives the same bits; ld = N * K and ld = N * K + 4 give the same bits (one access path, four bytes
 *      per lane and access, whatever the base pointer and the leading dimension); with K = 1, topk = 0 and smoothing = 0 every
 *      output equals that of the corresponding call of ktf_loss.h bit for bit.
 *  H6. Degenerate cases. B = 0: nothing is launched and dinv_w (if given) is written as zero. N = 1: loss = 0 and dz = 0 exactly, H_b
 *      empty. topk >= N - 1 penalises every class but the target.
 *  H7. Refused (KTF_EINVAL, before any launch, no GPU needed): everything of ktf_loss.h, rule 10 that applies to these arguments (null
 *      z, labels, loss, lse or workspace (forward), z, labels, lse, dz or workspace (backward); one of inv_x / inv_w without the
 *      other; dinv_x / dinv_w that do not go with the head; a margin kind on a plain head; a non-zero margin with SOFTMAX; scale <= 0
 *      or not finite; margin not finite, < 0, or >= pi / 2 for AAM; an unknown kind; B < 0; N < 1; a leading dimension below N * K; dz
 *      overlapping z other than exactly); K outside [1, KTF_HEAD_MAX_CENTERS]; K > 1 or topk > 0 on a plain head; topk outside
 *      [0, KTF_HEAD_MAX_TOPK]; a penalty that is not finite, negative, or non-zero with topk = 0; smoothing not finite or outside
 *      [0, 1); a null `hard` with topk > 0; B, N * K or a leading dimension at or beyond 2^31, or a grid of 2^31 workgroups; a workspace
 *      below ktf_head_workspace_bytes or not 256-byte aligned. Elements are addressed in 64 bits.
 */
#ifndef KTF_HEAD_H_
#define KTF_HEAD_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_HEAD_MAX_CENTERS 8        /* sub-centres per class (rule H1) */
#define KTF_HEAD_MAX_TOPK 64          /* penalised classes per row (rule H2) */
#define KTF_HEAD_SLOT_ROWS 8          /* batch rows per slot of partial sums of dinv_w (rule H5) */
#define KTF_HEAD_CHUNK_CLASSES 256    /* classes per workgroup of the backward call (rule H5) */

/* KTF_HEAD_SLOT_ROWS, for callers that do not read the header. */
int32_t ktf_head_slot_rows(void);

/* Bytes of the workspace either call takes: al256(max(ceil(B / KTF_HEAD_SLOT_ROWS), 1) * N * K * 8) for the slots plus
 * al256(ceil(N / KTF_HEAD_CHUNK_CLASSES) * max(B, 1) * 8) for the rows' sums per chunk (al256: rounded up to a multiple of 256).
 * Never 0; a negative KTF_* code on bad arguments. The forward call checks the workspace and leaves it untouched. */
int64_t ktf_head_workspace_bytes(int64_t B, int64_t N, int64_t K);

/* Rules H1 - H3: loss (B floats), pred (B int32 or NULL), lse (B doubles), hard (B x max(topk, 1) int32; NULL allowed when
 * topk = 0), sub_y (B int32 or NULL). */
int ktf_head_forward(const float* z, int64_t ldz, int64_t B, int64_t N, int64_t K, const int32_t* labels, const float* inv_x,
                     const float* inv_w, int32_t kind, double margin, double scale, int32_t topk, double penalty, double smoothing,
                     float* loss, int32_t* pred, double* lse, int32_t* hard, int32_t* sub_y, void* workspace, size_t workspace_bytes,
                     void* stream);

/* Rule H4. gloss is B floats, NULL = all ones. */
int ktf_head_backward(const float* z, int64_t ldz, int64_t B, int64_t N, int64_t K, const int32_t* labels, const float* inv_x,
                      const float* inv_w, int32_t kind, double margin, double scale, int32_t topk, double penalty, double smoothing,
                      const double* lse, const int32_t* hard, const float* gloss, float* dz, int64_t lddz, float* dinv_x, float* dinv_w,
                      void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
