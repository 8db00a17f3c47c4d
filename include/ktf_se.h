/*
 * ktf_se.h -- the squeeze-excitation gate (Hu et al. 2018) of an SE-Res2Block with the block's skip connection fused into it, forward
 * (three launches) and backward (four). Entry points of libktf_hip.so next to those of ktf_hip.h, whose conventions and error codes
 * hold here too (kernels: csrc/se_gate.hip).
 *
 *     y = x * sigmoid(W2^T relu(W1^T mean_t(x) + b1) + b2) + r
 *
 * x is fp32 (B, T, ldx) with C channels, r an optional residual fp32 (B, T, ldr), y fp32 (B, T, ldy). `lens` is B int32 on the device
 * or NULL; len_b = lens ? clamp(lens[b], 0, T) : T. W1 is fp32 (C, H) as [c][h], b1 (H), W2 fp32 (H, C) as [h][c], b2 (C); both biases
 * may be NULL. There is one arithmetic: the call has no `gemm` mode.
 *   1. Rows t >= len_b and the pad columns of x and r are never read; they may hold NaN. Rows t >= len_b and the pad columns of y are
 *      left untouched.
 *   2. Squeeze. mu[b,c] = (sum_{t < len_b} (double)x[b,t,c]) / len_b in fp64. The sum has the one order and association of ktf_attn.h
 *      rule 8: row t goes to group t mod 64, a group adds its rows in ascending order starting from +0, the 64 groups are combined as
 *      ((g + g+16) + g+32) + g+48 for g = 0..15 and these sixteen are added in ascending g. This does not depend on B, on the position
 *      of the utterance in the batch, on T beyond len_b, on the strides, on the alignment of any pointer or on the launch shape the
 *      library picks (it has two -- 16 row groups of 64 lanes or 64 row groups of 16 lanes per workgroup -- and chooses by the grid).
 *   3. Excite. fp64, sums in ascending index starting from the bias (or +0), on v_mfma_f64_16x16x4_f64: an element's accumulator takes
 *      its terms four per instruction in ascending order; a count that is no multiple of four is padded with +0 * +0 terms.
 *        h[b,j] = relu(b1[j] + sum_c mu[b,c] W1[c,j])            (v < 0 ? 0 : v)
 *        z[b,c] = b2[c] + sum_j h[b,j] W2[j,c]
 *        s[b,c] = (float)(1 / (1 + exp(-z[b,c])))                 rounded to fp32 once
 *   4. Scale. y = fl32(x * s): one fp32 multiply; with r it is followed by one fp32 add of r; no fused multiply-add.
 *   5. len_b = 0: mu, h and s of that utterance are written as +0, nothing of its x, r, y is touched and it contributes nothing to any
 *      parameter gradient. B = 0 or T = 0: nothing is launched (backward: only the zero fill of the parameter gradients).
 *   6. Side outputs of the training forward: mean (B, C) fp64, hid (B, H) fp64, gate (B, C) fp32, all dense. The inference call takes
 *      `gate` only, as caller-provided workspace of KTF_SE_GATE_FLOATS(B, C) floats: the gate in the first B C of them, the fp64 means
 *      behind it. y has the same bits in both calls.
 *   7. Backward, given g (B, T, ldg) = dL/dy. All fp64, every operation rounded on its own, each fp32 output rounded once:
 *        ds[b,c]  = sum_{t < len_b} (double)g[b,t,c] * (double)x[b,t,c]     (the product is exact; the sum in the order of rule 2)
 *        dz2      = ds * (s * (1 - s)), s the saved fp32 gate widened
 *        dh[b,j]  = (sum_c dz2[b,c] W2[j,c]) * [hid[b,j] > 0], ascending c as in rule 3
 *        dmu[b,c] = sum_j dh[b,j] W1[c,j], ascending j
 *        dx[b,t,c] = (float)((double)g[b,t,c] * (double)s[b,c] + dmu[b,c] / len_b)
 *      Rows t >= len_b of dx are written as zero in [0, C); its pad columns are left untouched.
 *        dW2[j,c] = (float)sum_b hid[b,j] dz2[b,c],  dW1[c,j] = (float)sum_b mean[b,c] dh[b,j],
 *        db2[c]   = (float)sum_b dz2[b,c],           db1[j]   = (float)sum_b dh[b,j]
 *      each in ascending b from +0 (four per MFMA, db as products with 1); each of the four may be NULL. The gradient of r is g
 *      itself: no kernel writes it.
 *   8. No atomics. The same call twice gives the same bits. An utterance alone and in a batch gives the same bits of y, gate and dx.
 *   9. Refused (KTF_EINVAL, before any launch, no GPU needed): a null x, y, W1, W2 or gate (training: mean, hid; backward: g, x, W1,
 *      W2, mean, hid, gate, dx) with B T > 0; C < 4, C % 4 != 0 or C > KTF_SE_MAX_DIM; H < 1 or H > KTF_SE_MAX_HIDDEN; a leading
 *      dimension below C, not a multiple of 4 or at 2^31; B above KTF_SE_MAX_BATCH, T above KTF_SE_MAX_ROWS, a negative size; gate
 *      (inference: workspace) or the backward's workspace not 256-byte aligned, the latter below
 *      ktf_se_gate_backward_workspace_bytes; mean or hid not 8-byte aligned; y overlapping x; y overlapping r in any way but y being
 *      r itself with ldy = ldr (the add is elementwise: the block's input may be overwritten by its output); dx overlapping g, x or
 *      gate. Elements are addressed in 64 bits.
 */
#ifndef KTF_SE_H_
#define KTF_SE_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_SE_MAX_BATCH 65535          /* utterances per call */
#define KTF_SE_MAX_ROWS 1073741824      /* 2^30: frames per utterance */
#define KTF_SE_MAX_DIM 4096             /* channels */
#define KTF_SE_MAX_HIDDEN 1024          /* bottleneck units */

/* Floats of the inference call's `gate` workspace (rule 6): B C for the gate, rounded up to 64, and 2 B C for the fp64 means. */
#define KTF_SE_GATE_FLOATS(B, C) ((((int64_t)(B) * (C) + 63) / 64) * 64 + 2 * (int64_t)(B) * (C))

/* Rules 1 - 6, inference. r may be NULL. */
int ktf_se_gate(const float* x, int64_t B, int64_t T, int32_t C, int64_t ldx, const float* r, int64_t ldr, const int32_t* lens,
                const float* w1, const float* b1, const float* w2, const float* b2, int32_t H, float* y, int64_t ldy, float* gate,
                void* stream);

/* The forward for training: also writes mean (B, C) fp64, hid (B, H) fp64 and gate (B, C) fp32 (rule 6). */
int ktf_se_gate_train(const float* x, int64_t B, int64_t T, int32_t C, int64_t ldx, const float* r, int64_t ldr, const int32_t* lens,
                      const float* w1, const float* b1, const float* w2, const float* b2, int32_t H, float* y, int64_t ldy, double* mean,
                      double* hid, float* gate, void* stream);

/* Bytes of the workspace the backward call takes: 3 al256(max(B, 1) C 8) for ds, dz2 and dmu / len plus al256(max(B, 1) H 8) for dh
 * (al256: rounded up to a multiple of 256). Never 0; a negative KTF_* code on bad sizes. */
int64_t ktf_se_gate_backward_workspace_bytes(int64_t B, int32_t C, int32_t H);

/* Rule 7. mean, hid and gate are the training forward's for the same x, lens and weights. */
int ktf_se_gate_backward(const float* g, int64_t B, int64_t T, int32_t C, int64_t ldg, const float* x, int64_t ldx, const int32_t* lens,
                         const float* w1, const float* w2, int32_t H, const double* mean, const double* hid, const float* gate, float* dx,
                         int64_t lddx, float* dw1, float* db1, float* dw2, float* db2, void* workspace, size_t workspace_bytes,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
