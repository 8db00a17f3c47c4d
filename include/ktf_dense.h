/*
 * ktf_dense.h -- the dense affine of a classification head and its gradients on the GPU: a short, dense batch of M rows against a very
 * tall weight of N rows (classes x centres), with no context, no lengths, no clamped rows and no padded or copied operand. Entry points
 * of libktf_hip.so next to those of ktf_hip.h, whose conventions and error codes hold here too (kernels:
 * csrc/dense_affine.hip).
 *
 * All operands are fp32, row-major with dense rows and an explicit leading dimension: x (M, ldx >= D), w (N, ldw >= D) -- the weight
 * as it stands in memory --, g (M, ldg >= N), bias and dbias N floats.
 *     ktf_dense_forward        z[m,n]  = bias[n] + sum_d x[m,d] * w[n,d]       (bias may be NULL)
 *     ktf_dense_grad_data      dx[m,d] = sum_n g[m,n] * w[n,d]
 *     ktf_dense_grad_weights   dw[n,d] = sum_m g[m,n] * x[m,d],  dbias[n] = sum_m g[m,n]      (dbias may be NULL)
 *
 *   1. Modes. `gemm` is KTF_GEMM_F32, KTF_GEMM_BF16 or KTF_GEMM_BF16X3 with the meaning of ktf_grad.h rules 6 - 9. F32: every product
 *      and its accumulation run on v_mfma_f32_32x32x2_f32, an fmaf chain over the reduction index in ascending order (the forward's
 *      chain starts from bias[n]). BF16: both operands are rounded to bf16, to nearest even, in registers between LDS and the matrix
 *      instruction v_mfma_f32_32x32x16_bf16; products are exact in fp32 and accumulation is fp32. BF16X3: every operand a is split
 *      into hi = bf16(a), lo = bf16(a - hi) and hi * hi, lo * hi, hi * lo are accumulated in fp32. No 16-bit copy of an operand exists
 *      in global memory in any mode.
 *   2. Reductions. The forward reduces over D and the weight gradient over M, each whole, in ascending steps of 32, inside one
 *      workgroup. The data gradient cuts the N columns of g into slots of KTF_DENSE_SLOT_COLS; every slot is reduced by a workgroup of
 *      its own into an fp32 partial tile in the workspace, and a second kernel adds the slots in ascending order. With one slot
 *      (N <= KTF_DENSE_SLOT_COLS) the partial is the result and is written to dx directly.
 *   3. dbias[n] is the sum over m ascending of the UNROUNDED fp32 g[m,n] in fp64, rounded once, in every mode.
 *   4. No floating-point atomics. The bits of every result are a function of (M, N, D, gemm) and the operands' values alone: not of
 *      the leading dimensions, of the alignment of any pointer or of the tile the library picks (it has two, 32 x 32 and 64 x 64
 *      outputs per workgroup, and takes the larger one when that still gives 512 workgroups). The same call twice gives the same bits.
 *   5. Alignment. Any M >= 0, N >= 1, D >= 1, any leading dimension at or above the row length, any 4-byte-aligned base. There is one
 *      path: operands are read four bytes per lane, consecutive lanes on consecutive addresses.
 *   6. Pad columns. The columns [N, ldz), [D, lddx), [D, lddw) of the outputs are written as zero. The columns [D, ldx), [D, ldw),
 *      [N, ldg) of the inputs are never read: they may hold NaN. Rows, columns and reduction elements beyond M, N, D enter the tiles
 *      as 0.0f and are never loaded.
 *   7. Degenerate cases. M = 0: the forward and the data gradient launch nothing; dw and dbias are written as zero.
 *   8. Refused (KTF_EINVAL, before any launch, no GPU needed): a null x, w, z (forward), g, w, dx, workspace (data gradient), g, x, dw
 *      (weight gradient); a `gemm` other than the three of rule 1; M < 0, N < 1, D < 1; a leading dimension below the row length; M,
 *      N, D or a leading dimension at or beyond 2^31; a grid dimension beyond the hardware's: ldz or N (weight gradient) above
 *      KTF_DENSE_MAX_COLS, M (data gradient) above KTF_DENSE_MAX_COLS, N (data gradient) above 65535 slots, M * lddx at or beyond
 *      2^38, or a workspace size that does not fit 63 bits; a workspace below ktf_dense_workspace_bytes or not 256-byte aligned; an
 *      output overlapping an input or another output (the whole of its rows, pad columns included). Elements are addressed in 64
 *      bits.
 */
#ifndef KTF_DENSE_H_
#define KTF_DENSE_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_DENSE_SLOT_COLS 256       /* columns of g per partial sum of the data gradient (rule 2) */
#define KTF_DENSE_MAX_COLS 2097120    /* 65535 * 32: the widest grid of 32-wide tiles (rule 8) */

/* KTF_DENSE_SLOT_COLS, for callers that do not read the header. */
int32_t ktf_dense_slot_cols(void);

/* Bytes of the workspace the data gradient takes: al256(ceil(N / KTF_DENSE_SLOT_COLS) * max(M, 1) * D * 4), the slots' partial
 * (M, D) tiles (al256: rounded up to a multiple of 256). Never 0; a negative KTF_* code on bad arguments (rule 8). */
int64_t ktf_dense_workspace_bytes(int64_t M, int64_t N, int64_t D);

/* z (M, ldz >= N). */
int ktf_dense_forward(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, int64_t M, int64_t N, int64_t D,
                      int32_t gemm, float* z, int64_t ldz, void* stream);

/* dx (M, lddx >= D). */
int ktf_dense_grad_data(const float* g, int64_t ldg, const float* w, int64_t ldw, int64_t M, int64_t N, int64_t D, int32_t gemm, float* dx,
                        int64_t lddx, void* workspace, size_t workspace_bytes, void* stream);

/* dw (N, lddw >= D), dbias N floats or NULL. */
int ktf_dense_grad_weights(const float* g, int64_t ldg, const float* x, int64_t ldx, int64_t M, int64_t N, int64_t D, int32_t gemm, float* dw,
                           int64_t lddw, float* dbias, void* stream);

#ifdef __cplusplus
}
#endif
#endif
