/*
 * ktf_grad.h -- gradients of the x-vector network's hot path on the GPU: the irregular-context convolution (ktf_tdnn) and the reducing
 * statistics pooling (ktf_stats_pool). Entry points of libktf_hip.so next to those of ktf_hip.h, whose conventions and error codes hold
 * here too (kernels: csrc/tdnn_grad.hip and csrc/tdnn_grad16.hip).
 *
 * The forward pass these differentiate is ktf_tdnn with KTF_GEMM_F32, act = KTF_ACT_NONE, scale = shift = NULL on fp32 x / W / y:
 *     z[b,t,u] = bias[u] + sum_k sum_d x[b, row(t,k), d] * W[u, k * din_pad + d]           for t < out_len_b
 *     row(t,k) = clip(start + t * subsampling + ctx[k], 0, len_b - 1),  len_b = lens ? lens[b] : T,  out_len_b = ktf_tdnn_out_len of (len_b, d)
 * W is the forward operand (units_pad, nctx * din_pad), units_pad = units rounded up to 256, zero in the pad region.
 * g[b,t,u] = dL/dz[b,t,u] is fp32 (B, T_out, ldg) with T_out = ktf_tdnn_out_len of (T, d) and ldg >= units.
 *
 *   1. Arithmetic. Every product and its accumulation run on the fp32 MFMA (v_mfma_f32_32x32x2_f32: an fmaf chain, one rounding per
 *      term). Sums that no product enters (dbias, the folded rows of rule 3, the slots of rule 2) are fp32 additions in a fixed order.
 *   2. No floating-point atomics. The row axis (b, t) of dW / dbias is cut into blocks of ktf_grad_tdnn_slot_rows() rows of the flat
 *      space b * T_out + t; every block writes its partial sums into a slot of its own in the workspace, and the slots are added in
 *      ascending order. The same call twice gives the same bits.
 *   3. Clamped rows. With SAME padding several (t, k) send their x row to 0 or len_b - 1. For dx their g rows are first added up, per
 *      (b, edge, k) in ascending t, and enter the GEMM as part of the A operand of row 0 / len_b - 1.
 *   4. Rows of g at or beyond out_len_b and rows of x at or beyond len_b are never read: they may hold anything, NaN included.
 *      Columns [units, ldg) of g and [din_pad, ldx) of x are not read either; columns [din, din_pad) of x must be finite (as for ktf_tdnn).
 *   5. Refused (KTF_EINVAL, before any launch, no GPU needed): null pointers; gemm != KTF_GEMM_F32; act != KTF_ACT_NONE; dtypes other than
 *      KTF_F32; a descriptor ktf_tdnn refuses (unsorted context, nctx outside [1, 16], din_pad not a multiple of 32, subsampling < 1);
 *      ldx < din_pad or ldx % 4 != 0; ldg < units; x, w, dx or dw not 16-byte aligned; a workspace below
 *      ktf_grad_tdnn_workspace_bytes or not 256-byte aligned; B > 65535; B * T_out >= 2^31.
 *
 * The ktf_grad_tdnn16_* calls compute the same two gradients on the 16-bit MFMA (v_mfma_f32_32x32x16_bf16) from the same fp32 g, W and
 * x: the backward half of mixed-precision training with fp32 master copies. Rules 2 - 5 hold for them unchanged (their workspace size is
 * ktf_grad_tdnn16_workspace_bytes'); rule 1 is replaced by rules 6 - 8. Write g^ = bf16(g), W^ = bf16(W), x^ = bf16(x), rounded to
 * nearest even in registers.
 *
 *   6. gemm = KTF_GEMM_BF16. Every product is g^ * W^ (data) or g^ * x^ (weights), exact in fp32; accumulation is fp32, on the MFMA
 *      and over the slots. The folded rows of rule 3 are fp32 sums of the ROUNDED g^ rows, per (b, edge, k) in ascending t; such a sum
 *      is not a bf16 number and enters the GEMM as the pair hi = bf16(f), lo = bf16(f - hi), in K-steps of their own that only the
 *      tiles holding row 0 or len_b - 1 run. It is never rounded to one bf16.
 *   7. gemm = KTF_GEMM_BF16X3. Every fp32 operand a is split into hi = bf16(a), lo = bf16(a - hi), and the three products hi * hi,
 *      lo * hi, hi * lo are accumulated in fp32 (the forward's KTF_GEMM_BF16X3). The folded rows are the fp32 sums of the fp32 g of rule
 *      3, added to the row's own g in fp32 as the fp32 kernel does; that A operand is split like any other.
 *   8. dbias, both modes: sums of the UNROUNDED fp32 g rows in a fixed order (per slot: per group of 16 rows of every 32-row step in
 *      ascending row order, the two groups added, the slots in ascending order).
 *   9. Refused as in rule 5, plus: a `gemm` argument other than KTF_GEMM_BF16 / KTF_GEMM_BF16X3 (KTF_GEMM_F32 has the calls above).
 *      The descriptor is the one of the fp32 calls: it describes the trainable forward (d->gemm == KTF_GEMM_F32, fp32 dtypes).
 */
#ifndef KTF_GRAD_H_
#define KTF_GRAD_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_GRAD_ROW_TILE 64      /* rows of dx per workgroup of the data gradient (ktf_grad_tdnn_weights reduces its rows 16 at a time) */
#define KTF_GRAD_SLOT_ROWS 512    /* flat rows b * T_out + t per dW / dbias slot (rule 2) */

/* The two constants above, for callers that do not read the header. */
int32_t ktf_grad_tdnn_row_tile(void);
int32_t ktf_grad_tdnn_slot_rows(void);

/* Bytes of the workspace both TDNN gradient calls of a (B, T) batch of layer `d` take (the folded rows of rule 3 and the slots of rule
 * 2; the two calls use disjoint parts). Never 0; a negative KTF_* code on bad arguments. */
int64_t ktf_grad_tdnn_workspace_bytes(int64_t B, int64_t T, const KtfTdnnDesc* d);

/* Data gradient: dx[b,r,d] = sum over (t,k) with row(t,k) = r, t < out_len_b, and over u, of g[b,t,u] * W[u, k * din_pad + d] for
 * r < len_b, d < din. dx is (B, T, ldx) fp32; rows r >= len_b and columns [din, ldx) are written as zero. */
int ktf_grad_tdnn_data(const float* g, int64_t ldg, int64_t B, int64_t T, const int32_t* lens, const KtfTdnnDesc* d, const float* w,
                       float* dx, int64_t ldx, void* workspace, size_t workspace_bytes, void* stream);

/* Weight and bias gradient: dw[u, k * din_pad + d] = sum_b sum_{t < out_len_b} g[b,t,u] * x[b, row(t,k), d] in the forward operand's
 * layout (units_pad, nctx * din_pad), zero where u >= units or d >= din; dbias[u] = sum_b sum_{t < out_len_b} g[b,t,u], `units`
 * floats (dbias may be NULL). */
int ktf_grad_tdnn_weights(const float* x, int64_t B, int64_t T, int64_t ldx, const int32_t* lens, const KtfTdnnDesc* d, const float* g,
                          int64_t ldg, float* dw, float* dbias, void* workspace, size_t workspace_bytes, void* stream);

/* The 16-bit counterparts (rules 6 - 9): the arguments of the three calls above, then the mode. Outputs, layouts, strides, alignment
 * and the zero-filled regions are those of the fp32 calls; B == 0, T == 0 or T_out == 0 launch no GEMM. */
int64_t ktf_grad_tdnn16_workspace_bytes(int64_t B, int64_t T, const KtfTdnnDesc* d, int32_t gemm);
int ktf_grad_tdnn16_data(const float* g, int64_t ldg, int64_t B, int64_t T, const int32_t* lens, const KtfTdnnDesc* d, const float* w,
                         float* dx, int64_t ldx, void* workspace, size_t workspace_bytes, int32_t gemm, void* stream);
int ktf_grad_tdnn16_weights(const float* x, int64_t B, int64_t T, int64_t ldx, const int32_t* lens, const KtfTdnnDesc* d, const float* g,
                            int64_t ldg, float* dw, float* dbias, void* workspace, size_t workspace_bytes, int32_t gemm, void* stream);

/* Gradient of ktf_stats_pool on fp32 x (B, T, ldx): with n_b the rows 0, input_period, ... < len_b, mean and var = E[x^2] - mean^2 from
 * fp64 column sums over them and std = sqrt(max(var, 0) + eps),
 *     dx[b,t,c] = gout[b,c] / n_b + gout[b,D + c] * (x[b,t,c] - mean) / (n_b * std)
 * on those rows, evaluated in fp64 and rounded once; the second term is absent without include_std and where var <= 0 (the clipped
 * relu). Every other row below T and the columns [D, ld_dx) are written as zero. gout is (B, ld_gout) fp32, ld_gout >= D or 2 D. */
int ktf_grad_stats_pool(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const int32_t* lens, int32_t input_period,
                        int32_t include_std, float eps, const float* gout, int64_t ld_gout, float* dx, int64_t ld_dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif
