// C (M x N, ldc) = [C +] op(A) op(B) in fp64 on v_mfma_f64_16x16x4_f64 (f64_mfma.h): no atomics, no split of K.
#include "f64_mfma.h"

namespace {

constexpr int MF_MT = 2;            // 16-row MFMA tiles per wave
constexpr int MF_NT = 4;            // 16-column MFMA tiles per wave
constexpr int MF_WAVES = 4;         // waves per workgroup: stacked along M it owns 128 x 64 of C, side by side along N 32 x 256

// Lane l holds op(A)[row l & 15][k = l >> 4] and op(B)[k = l >> 4][col l & 15]; result reg r of lane l is C[row (l >> 4) + 4 r]
// [col l & 15]. A_KM: A is stored (K x M), else (M x K). B_KN: B is stored (K x N), else (N x K). FROM_C: the accumulators start
// from C, else from zero. ALONG_M: the workgroup's waves are stacked along M, else side by side along N. k runs upwards four at a time.
template <bool A_KM, bool B_KN, bool FROM_C, bool ALONG_M>
__global__ void __launch_bounds__(64 * MF_WAVES) f64_mfma_kernel(const double* __restrict__ A, int64_t lda, const double* __restrict__ Bm,
                                                                 int64_t ldb, double* __restrict__ Cm, int64_t ldc, int64_t M, int64_t N,
                                                                 int64_t K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const int64_t m0 = (ALONG_M ? (int64_t)blockIdx.y * MF_WAVES + wave : (int64_t)blockIdx.y) * (16 * MF_MT);
    const int64_t n0 = (ALONG_M ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * MF_WAVES + wave) * (16 * MF_NT);
    if (ALONG_M ? m0 >= M : n0 >= N) return;
    f64x4 acc[MF_MT][MF_NT];
#pragma unroll
    for (int i = 0; i < MF_MT; ++i)
#pragma unroll
        for (int j = 0; j < MF_NT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + 16 * i + lk + 4 * r, col = n0 + 16 * j + lc;
                acc[i][j][r] = (FROM_C && row < M && col < N) ? Cm[row * ldc + col] : 0.0;
            }
    for (int64_t k0 = 0; k0 < K; k0 += 4) {
        const int64_t k = k0 + lk;
        double a[MF_MT], bv[MF_NT];
#pragma unroll
        for (int i = 0; i < MF_MT; ++i) {
            const int64_t m = m0 + 16 * i + lc;
            a[i] = (k < K && m < M) ? (A_KM ? A[k * lda + m] : A[m * lda + k]) : 0.0;
        }
#pragma unroll
        for (int j = 0; j < MF_NT; ++j) {
            const int64_t c = n0 + 16 * j + lc;
            bv[j] = (k < K && c < N) ? (B_KN ? Bm[k * ldb + c] : Bm[c * ldb + k]) : 0.0;
        }
#pragma unroll
        for (int i = 0; i < MF_MT; ++i)
#pragma unroll
            for (int j = 0; j < MF_NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bv[j], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < MF_MT; ++i)
#pragma unroll
        for (int j = 0; j < MF_NT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + 16 * i + lk + 4 * r, col = n0 + 16 * j + lc;
                if (row < M && col < N) Cm[row * ldc + col] = acc[i][j][r];
            }
}

}  // namespace

int f64_atb(const char* who, const double* A, int64_t lda, const double* Bm, int64_t ldb, double* Cm, int64_t ldc, int64_t M, int64_t N,
            int64_t K, hipStream_t st) {
    hipLaunchKernelGGL((f64_mfma_kernel<true, true, true, true>), dim3(ktf_cdiv(N, 16 * MF_NT), ktf_cdiv(M, 16 * MF_MT * MF_WAVES)),
                       dim3(64 * MF_WAVES), 0, st, A, lda, Bm, ldb, Cm, ldc, M, N, K);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

int f64_nt(const char* who, const double* A, int64_t lda, const double* Bm, int64_t ldb, double* Cm, int64_t ldc, int64_t M, int64_t N,
           int64_t K, hipStream_t st) {
    hipLaunchKernelGGL((f64_mfma_kernel<false, false, false, false>), dim3(ktf_cdiv(N, 16 * MF_NT * MF_WAVES), ktf_cdiv(M, 16 * MF_MT)),
                       dim3(64 * MF_WAVES), 0, st, A, lda, Bm, ldb, Cm, ldc, M, N, K);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
