/*
 * ktf_gcgrad.h -- the gradient of the global-context attention logits of ktf_gctx.h, for training attentive statistics pooling with
 * global context (ECAPA-TDNN). Entry points of libktf_hip.so next to those of ktf_hip.h, whose conventions and error codes hold here
 * too (kernels: csrc/attn_ctx_grad.hip). The forward is ktf_gctx.h unchanged:
 *
 *     g_b = b1 + W1c^T [mu_b ; sigma_b],      z[b,t] = W1x^T x[b,t] + g_b,      h = act(z),      e = W2^T h + b2,      t < len_b = n.
 *
 * Given de = dL/de (B, T, H) -- from the pooling backward of ktf_attn.h -- three calls produce, for rows t < len_b,
 *
 *     dh = de W2^T                 dz = dh * act'(z)        (tanh: 1 - h^2;  relu: z > 0 ? 1 : 0)
 *     dg_b = sum_t dz[b,t]         db1 = sum_b dg_b         dW1c = sum_b ctx_b^T dg_b         dctx_b = W1c dg_b = (dmu_b, dsig_b)
 *     dx[b,t,c] += (dz[b,t] W1x^T)_c + dmu_c / n + s_c (x[b,t,c] - mu_c),      s_c = sigma_c^2 > eps ? dsig_c / (n sigma_c) : 0
 *
 * (s_c is the derivative of sqrt(max(q - mu^2, 0) + eps) through q and mu). dW1x = sum x^T dz, dW2 = sum h^T de and db2 = sum de are
 * ordinary weight gradients over (x, dz) and (h, de): the context-[0] calls of ktf_grad.h take them, no kernel of this header.
 *
 * x, W1x, W1c, W2, g, ctx and lens are the operands of ktf_gctx.h. de is fp32 (B, T, lde) with H heads; dz and h are fp32 (B, T, ldz)
 * with A units; dx is fp32 (B, T, lddx) with D channels; dW1c is fp32 (2 D, lddw) with A columns, db1 A floats; coef is fp64 (B, 2, D)
 * dense. The workspace is 256-byte aligned, of ktf_gcgrad_workspace_bytes(B, A) bytes.
 *
 *   1. Rows t >= len_b of x and de, their pad columns, and the pad columns of W1x, W1c, W2, g and dz are never read: they may hold NaN.
 *   2. ktf_gcgrad_hidden: a workgroup owns the rows [t0, t0 + R) of ONE utterance, t0 a multiple of R = ktf_gcgrad_row_tile(), and
 *      every unit of them. z and h are recomputed exactly as rule 6 of ktf_gctx.h forms them (chunks of 32 ascending from +0, g added
 *      to the finished sum, the same act); h stays in LDS and is never read back from the forward. dh[r,a] = sum_{j < H} de[r,j] *
 *      W2[a,j] runs over chunks of 32 heads taken ascending, the accumulator starting from +0; dz = dh * d in fp32 with d = 1 - h * h
 *      (tanh; each operation rounded on its own) or d = h > 0 ? 1 : 0 (relu; h > 0 exactly when z > 0).
 *   3. `gemm` is KTF_GEMM_F32 or KTF_GEMM_BF16X3 with the chunk arithmetic of rule 7 of ktf_gctx.h in every product of this header: the
 *      rows (x, de, dz) are the left operand, the weights the right one, either split in registers. One-pass bf16 is refused.
 *   4. ktf_gcgrad_hidden writes dz[b,t,a] and h[b,t,a] for every t < T and a < A: the values for t < len_b, +0 for t >= len_b (an empty
 *      utterance: all zero). Columns [A, ldz) are left untouched.
 *   5. ktf_gcgrad_context, in fp64: dg[b,a] = sum_{t < len_b} dz[b,t,a] in the order of ktf_attn.h rule 8 (csrc/canon_sum.h), kept in
 *      the workspace. dctx[b,k] = sum_{a < A} dg[b,a] * W1c[k,a] (ascending a from +0) and dW1c[k,a] = sum_b ctx[b,k] * dg[b,a],
 *      db1[a] = sum_b dg[b,a] (ascending b from +0) on v_mfma_f64_16x16x4_f64, four terms per instruction, padded with zeros where the
 *      shape is no multiple of the instruction's; dW1c and db1 are rounded once to fp32. An utterance with len_b = 0 enters every sum
 *      as zero (its ctx, NaN by rule 4 of ktf_gctx.h, is not used). No atomics.
 *   6. coef[b,0,c] = dmu_c / n and coef[b,1,c] = sigma_c * sigma_c > (double)eps ? dsig_c / (n * sigma_c) : 0, sigma_c = ctx[b,1,c], each
 *      operation rounded on its own; both are 0 when len_b = 0. dW1c (with lddw) and db1 may be NULL: not computed.
 *   7. ktf_gcgrad_data: the row tiles of rule 2. acc[r,c] = sum_{a < A} dz[r,a] * W1x[c,a] in fp32 (rule 3; chunks of 32 units ascending
 *      from +0, the dz tile kept in LDS, the channels looped in blocks of 256); then, in fp64 and in this order,
 *      dx[b,t,c] = (float)((((double)acc + (double)dx_in) + coef[b,0,c]) + coef[b,1,c] * ((double)x[b,t,c] - ctx[b,0,c])),
 *      dx_in the value dx held (accumulate != 0) or +0 (accumulate == 0: dx is not read). Each element is read and written by one
 *      thread, once. Rows t >= len_b of dx and its columns [D, lddx) are left untouched.
 *   8. Independence. The bits of an utterance's dz, h, coef and dx do not depend on B, on its position in the batch, on T beyond len_b,
 *      on any leading dimension or on the alignment of any pointer (LDS-DMA for 16-byte aligned operands with leading dimensions that
 *      are multiples of 4, scalar loads into the same LDS image otherwise). dW1c and db1 sum over b in ascending order. No atomics
 *      anywhere; the same call twice gives the same bits.
 *   9. Error. With u the unit of `gemm` (2^-24; split operands: (3 + 2^-6) 2^-16 as for ktf_grad.h) and S the value's own expression
 *      over absolute values, |value - exact| <= k u S with k the rounded stages of its chain: h: 5 (product, g's rounding, the add, two
 *      for tanhf); dz: 8 (h's five, two for 1 - h h, the product with dh; S takes the sensitivity 2 |h| S_z |dh| of d in); coef, dW1c
 *      and db1: 9 (dz's eight, one rounding of the fp64 result -- for coef the division); dx: 10 (dz's eight, the product, the final
 *      rounding). With relu an element whose |z| is below 2^-18 S_z may fall on either side of the switch and is not bounded.
 *  10. Refused (KTF_EINVAL, before any launch, no GPU needed): the sizes, leading dimensions, eps, act and gemm that rule 10 of
 *      ktf_gctx.h refuses (ldz < A, lddx < D and lddw < A included); a null x, W1x, g, W2, de, dz or h with B T > 0 (hidden); a null
 *      dz, ctx, W1c, coef or workspace with B > 0, a workspace below ktf_gcgrad_workspace_bytes or not 256-byte aligned (context); a
 *      null dz, W1x, x, ctx, coef or dx with B T > 0 (data). Elements are addressed in 64 bits.
 */
#ifndef KTF_GCGRAD_H_
#define KTF_GCGRAD_H_

#include "ktf_gctx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rules 2 - 4. B T = 0: nothing is launched. */
int ktf_gcgrad_hidden(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const int32_t* lens, const float* w1x, int64_t ldw1,
                      const float* g, int64_t ldg, int32_t A, int32_t act, const float* w2, int64_t ldw2, int32_t H, int32_t gemm,
                      const float* de, int64_t lde, float* dz, float* h, int64_t ldz, void* stream);

/* Rules 5 and 6. B = 0: nothing is launched. */
int ktf_gcgrad_context(const float* dz, int64_t B, int64_t T, int32_t A, int64_t ldz, const int32_t* lens, const double* ctx, int32_t D,
                       const float* w1c, int64_t ldw, float eps, float* dw1c, int64_t lddw, float* db1, double* coef, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Rule 7. B T = 0: nothing is launched. */
int ktf_gcgrad_data(const float* dz, int64_t B, int64_t T, int32_t A, int64_t ldz, const int32_t* lens, const float* w1x, int64_t ldw1,
                    int32_t D, const float* x, int64_t ldx, const double* ctx, const double* coef, int32_t gemm, int32_t accumulate,
                    float* dx, int64_t lddx, void* stream);

/* Rows per workgroup (R of rules 2 and 7) for A units and H heads. A negative KTF_* code on arguments rule 10 refuses. */
int32_t ktf_gcgrad_row_tile(int32_t A, int32_t H, int32_t gemm);

/* Bytes of the workspace of ktf_gcgrad_context (dg, fp64 (B, A)). A negative KTF_* code on arguments rule 10 refuses. */
int64_t ktf_gcgrad_workspace_bytes(int64_t B, int32_t A);

#ifdef __cplusplus
}
#endif
#endif
