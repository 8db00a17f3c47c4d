/*
 * ktf_norm.h -- the block between two GEMMs of the x-vector network in training: ReLU followed by batch normalisation, forward and
 * backward, on the GPU. Entry points of libktf_hip.so next to those of ktf_hip.h, whose conventions and error codes hold here too
 * (kernels: csrc/norm_train.hip).
 *
 * z, y, gy and dz are fp32 (B, T, ld) with ld >= D, `lens` (B int32 on the device) may be NULL: len_b = lens ? clip(lens[b], 0, T) : T.
 * A (N, D) input behind the pooling is the case B = 1, T = N. Per feature c < D, with a = relu ? max(z, 0) : z and n = sum_b len_b:
 *     y[b,t,c] = gamma[c] * (a[b,t,c] - mean[c]) * invstd[c],  invstd = 1 / sqrt(var + eps)               for t < len_b
 * (no beta, as in the project's BatchNorm). gamma, moving_mean, moving_var and dgamma are D floats; `saved` is (2, D) fp64: mean, invstd.
 *
 *   1. Forward, training = 1. S1 = sum a and S2 = sum a * a per feature over the valid rows (b, t < len_b), in fp64 (the square of an
 *      fp32 number is exact there). mean = S1 / n, var = max(S2 / n - mean * mean, 0), in fp64, every operation rounded on its own.
 *      moving <- (float)((double)moving * momentum + batch * (1 - momentum)) in place, for moving_mean (batch = mean) and moving_var
 *      (batch = var): evaluated in fp64 and rounded once.
 *   2. Forward, training = 0. mean = moving_mean, var = moving_var (converted to fp64); nothing is reduced, nothing is updated,
 *      momentum is not looked at beyond rule 8. `saved` is written in both modes: the backward call reads it.
 *   3. y = (float)((((double)a - mean) * gamma) * invstd): fp64, rounded once. Rows at and beyond len_b and columns [D, ldy) of y are
 *      written as zero.
 *   4. Backward. With ahat = (a - mean) * invstd from z and `saved`: s1 = sum gy and s2 = sum gy * ahat in fp64 over the valid rows;
 *      dgamma = (float)s2 (dgamma may be NULL). training = 1: dz = (float)((gamma * invstd) * ((gy - s1 / n) - ahat * (s2 / n)));
 *      training = 0: dz = (float)((gamma * invstd) * gy). With relu, dz = 0 where z <= 0 (-0.0 included: torch.relu's gradient at 0).
 *      Rows at and beyond len_b and columns [D, ld_dz) of dz are written as zero. The backward call reads z again, not y: y must not
 *      have overwritten z (rule 8), and `saved`, gamma, lens, relu and training must be those of the forward call.
 *   5. No floating-point atomics. The flat row space b * T + t is cut into blocks of ktf_norm_slot_rows() rows; every block adds its
 *      valid rows in a fixed order (row j of the block goes to group j mod 8 in ascending j, the groups are added as
 *      ((((((0 + 1) + 2) + 3) + 4) + 5) + 6) + 7) and writes its fp64 partial sums into a slot of its own in the workspace; the slots
 *      are added in ascending order. The same call twice gives the same bits, whatever the alignment path taken (rule 9).
 *   6. Rows of z and gy at or beyond len_b are never read and the columns [D, ld) never enter a result: both may hold anything, NaN
 *      included.
 *   7. n = 0 (every length 0, or B * T = 0): y, dz and dgamma are zero, `saved` is written as (0, 0), the moving statistics are
 *      untouched, no NaN is produced. n = 1: var = 0 and invstd = 1 / sqrt(eps).
 *   8. Refused (KTF_EINVAL, before any launch, no GPU needed): a null z, gamma, moving_mean, moving_var, y, saved or workspace
 *      (forward), a null gy, z, gamma, saved, dz or workspace (backward); B < 0 or T < 0; D < 1; a leading dimension below D;
 *      eps <= 0 or not finite; momentum outside [0, 1]; a workspace below ktf_norm_workspace_bytes or not 256-byte aligned;
 *      B * T >= 2^31 (or a batch whose workgroup count does not fit the grid); y overlapping z; dz overlapping z or gy.
 *   9. Rows are read and written 16 bytes per lane where every leading dimension of the call is a multiple of 4 and every base
 *      pointer is 16-byte aligned, element by element otherwise. The values are the same.
 */
#ifndef KTF_NORM_H_
#define KTF_NORM_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_NORM_SLOT_ROWS 128    /* flat rows b * T + t per slot of partial sums (rule 5) */

/* The constant above, for callers that do not read the header. */
int32_t ktf_norm_slot_rows(void);

/* Bytes of the workspace either call takes for a (B, T, D) batch: al256(max(ceil(B * T / slot_rows), 1) * 2 * D * 8) for the slots
 * plus al256((2 * D + 1) * 8) for the totals (al256: rounded up to a multiple of 256). Never 0; a negative KTF_* code on bad
 * arguments (B < 0, T < 0, D < 1, B * T >= 2^31). The forward and the backward call may share one workspace on one stream. */
int64_t ktf_norm_workspace_bytes(int64_t B, int64_t T, int32_t D);

/* Rules 1 - 3. */
int ktf_norm_relu_bn_forward(const float* z, int64_t ldz, int64_t B, int64_t T, int32_t D, const int32_t* lens, int32_t relu,
                             int32_t training, const float* gamma, float* moving_mean, float* moving_var, double momentum, double eps,
                             float* y, int64_t ldy, double* saved, void* workspace, size_t workspace_bytes, void* stream);

/* Rule 4. */
int ktf_norm_relu_bn_backward(const float* gy, int64_t ldg, const float* z, int64_t ldz, int64_t B, int64_t T, int32_t D,
                              const int32_t* lens, int32_t relu, int32_t training, const float* gamma, const double* saved, float* dz,
                              int64_t ld_dz, float* dgamma, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
