// i-vector extractor training statistics: Kaldi's `ivector-extractor-acc-stats` (IvectorExtractorStats::AccStatsForUtterance with
// update_variances, no ivector-dependent weights), batched over the utterances of one call and accumulated in place into fp64 device
// totals. Stages (b) - (d) of the extraction (ivector_stages.h) leave gamma, F, the linear term and the Cholesky factor L of
// Q = I + sum_i gamma_i U_i in the workspace; from there
//
//   ivcov_kernel     (ivector_stages.hip) per utterance (one workgroup): sum_j log L_jj, X = L^-1 in place (blocked, 32 x 32 tiles
//                    in LDS), z = X lin', w = X^T z (the posterior mean, the prior offset kept), W = X^T X + w w^T as a packed lower
//                    triangle, and the scalar lin'^T w / 2 - sum_j log L_jj - offset^2 / 2 of the marginal likelihood. An utterance
//                    with no frames gets zeros and the flag 0.
//   f64_atb          (f64_mfma.hip) C += A^T B in fp64 on v_mfma_f64_16x16x4_f64: A (K x M) and B (K x N) row-major, K = the
//                    utterances of the chunk, ascending inside every output element; no atomics, no split of K. One kernel for R
//                    (A = gamma, B = W), Y (A = F, B = w), gamma, the prior's sum and scatter and the two scalar totals (A = the flags).
//   sec_acc_kernel   second-order statistics Ssec_i += sum_t p'_ti x_t x_t^T: the (frame, slot) pairs are bucketed by Gaussian with the
//                    STABLE counting sort of gmm_bucket.hip, so a bucket lists its pairs in ascending pair id and its fp64 sum,
//                    taken row after row, has the same bits on every run.
#include "ivector_stages.h"
#include "f64_mfma.h"
#include "gmm_bucket.h"

namespace {

constexpr int SEC_RB = 16;          // bucket rows staged in LDS per step

struct TrLayout {
    int64_t ext, scat, w, tail, total;
};

TrLayout tr_layout(int64_t B, int64_t I, int64_t D, int64_t S) {
    TrLayout t;
    const int64_t P = S * (S + 1) / 2;
    t.ext = 0;
    int64_t at = iv_layout(B, I, D, S).total;
    t.scat = at; at += al256(B * P * 8);
    t.w = at;    at += al256(B * S * 8);
    t.tail = at; at += al256(B * 2 * 8);
    t.total = at;
    return t;
}

// ---------------------------------------------------------------- second-order statistics (the bucketing: gmm_bucket.hip)
// Ssec[g] (D x D) += sum over the bucket's rows, in bucket order, of p' x x^T: one workgroup per Gaussian, thread (ty, tx) owns
// elements (ty + 16 a, tx + 16 c). x_i x_j is exact in fp64 (fp32 inputs), so the result is symmetric bit for bit.
__global__ void __launch_bounds__(256) sec_acc_kernel(const float* __restrict__ x, int D, int64_t ldx, const float* __restrict__ post, int n,
                                                       float post_scale, const int* __restrict__ start, const int* __restrict__ pairs,
                                                       double* __restrict__ Ssec) {
    __shared__ double xs[SEC_RB][KTF_IVECTOR_MAX_FEAT_DIM];
    __shared__ double wr[SEC_RB];
    const int g = blockIdx.x, tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int r0 = start[g], r1 = start[g + 1];
    if (r1 <= r0) return;
    constexpr int NA = KTF_IVECTOR_MAX_FEAT_DIM / 16;
    double acc[NA][NA];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int c = 0; c < NA; ++c) acc[a][c] = 0.0;
    for (int rb = r0; rb < r1; rb += SEC_RB) {
        const int nr = r1 - rb < SEC_RB ? r1 - rb : SEC_RB;
        for (int e = tid; e < nr * D; e += 256) {
            const int r = e / D, d = e - r * D;
            const int p = pairs[rb + r];
            xs[r][d] = (double)x[(int64_t)(p / n) * ldx + d];
        }
        if (tid < nr) wr[tid] = (double)(post[pairs[rb + tid]] * post_scale);
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            const double w = wr[r];
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                if (16 * a >= D) break;
                const int i = ty + 16 * a;
                const double xi = i < D ? xs[r][i] : 0.0;
#pragma unroll
                for (int c = 0; c < NA; ++c) {
                    if (16 * c >= D) break;
                    const int j = tx + 16 * c;
                    const double xj = j < D ? xs[r][j] : 0.0;
                    acc[a][c] = fma(xi * xj, w, acc[a][c]);
                }
            }
        }
        __syncthreads();
    }
    double* out = Ssec + (int64_t)g * D * D;
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int c = 0; c < NA; ++c) {
            const int i = ty + 16 * a, j = tx + 16 * c;
            if (i < D && j < D) out[(int64_t)i * D + j] += acc[a][c];
        }
}

}  // namespace

extern "C" int ktf_atb_f64(const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, int64_t M, int64_t N,
                           int64_t K, void* stream) {
    const char* who = "ktf_atb_f64";
    KTF_REQUIRE(M >= 1 && N >= 1 && K >= 0, "%s: M %lld, N %lld, K %lld out of range", who, (long long)M, (long long)N, (long long)K);
    KTF_REQUIRE(M <= ((int64_t)1 << 22) && N <= ((int64_t)1 << 21), "%s: M %lld > 2^22 or N %lld > 2^21", who, (long long)M, (long long)N);
    KTF_REQUIRE(lda >= M && ldb >= N && ldc >= N, "%s: lda %lld < M, ldb %lld < N or ldc %lld < N", who, (long long)lda, (long long)ldb,
                (long long)ldc);
    KTF_REQUIRE(C && (K == 0 || (A && B)), "%s: null argument", who);
    if (K == 0) return KTF_OK;
    return f64_atb(who, A, lda, B, ldb, C, ldc, M, N, K, (hipStream_t)stream);
}

extern "C" int64_t ktf_ivector_train_workspace_bytes(int32_t B, int32_t I, int32_t D, int32_t S) {
    const int64_t ext = ktf_ivector_workspace_bytes(B, I, D, S);
    if (ext < 0) return ext;
    return tr_layout(B, I, D, S).total;
}

extern "C" int ktf_ivector_acc_stats(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* offsets, int32_t B, const int32_t* gauss,
                                     const float* post, int32_t n, float posterior_scale, const double* sigma_inv_M, const double* U, int32_t I,
                                     int32_t S, double prior_offset, double* gamma, double* Y, double* R, double* ivector_sum,
                                     double* ivector_scatter, double* totals, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_ivector_acc_stats";
    const int64_t need = ktf_ivector_train_workspace_bytes(B, I, D, S);
    if (need < 0) return (int)need;
    KTF_REQUIRE(F >= 0 && F < ((int64_t)1 << 31), "%s: frame count %lld out of range", who, (long long)F);
    KTF_REQUIRE(ldx >= D, "%s: ldx %lld < D %d", who, (long long)ldx, (int)D);
    KTF_REQUIRE(n >= 1 && n <= KTF_IVECTOR_MAX_GSELECT, "%s: %d slots per frame outside 1 .. %d", who, (int)n, KTF_IVECTOR_MAX_GSELECT);
    KTF_REQUIRE(posterior_scale >= 0.f, "%s: posterior_scale must be >= 0", who);
    KTF_REQUIRE(offsets && sigma_inv_M && U && workspace, "%s: null argument", who);
    KTF_REQUIRE(gamma && Y && R && ivector_sum && ivector_scatter && totals, "%s: null accumulator", who);
    KTF_REQUIRE(F == 0 || (x && gauss && post), "%s: null frames / posteriors", who);
    if (ktf_check_workspace(who, workspace, workspace_bytes, need) != KTF_OK) return KTF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const IvLayout l = iv_layout(B, I, D, S);
    const TrLayout t = tr_layout(B, I, D, S);
    double* scat = (double*)(ws + t.scat);
    double* wv = (double*)(ws + t.w);
    double* tail = (double*)(ws + t.tail);
    int rc = iv_run_stages(who, x, F, (int)D, ldx, offsets, (int)B, gauss, post, (int)n, posterior_scale, 1.f, 0.f, sigma_inv_M, U, (int)I,
                           (int)S, prior_offset, wv, 8, ws, st);
    if (rc != KTF_OK) return rc;
    rc = iv_cov(who, (const double*)(ws + l.lin), offsets, (int)B, F, (int)S, prior_offset, (double*)(ws + l.L), scat, wv, tail, st);
    if (rc != KTF_OK) return rc;
    const int64_t P = (int64_t)S * (S + 1) / 2, ID = (int64_t)I * D;
    const double* gam = (const double*)(ws + l.gamma);
    const double* Fst = (const double*)(ws + l.F);
    if ((rc = f64_atb(who, gam, I, scat, P, R, P, I, P, B, st)) != KTF_OK) return rc;             // R_i += gamma_ui W_u
    if ((rc = f64_atb(who, Fst, ID, wv, S, Y, S, ID, S, B, st)) != KTF_OK) return rc;             // Y_i += F_ui w_u^T
    if ((rc = f64_atb(who, gam, I, tail, 2, gamma, 1, I, 1, B, st)) != KTF_OK) return rc;         // gamma += gamma_u (counted utterances)
    if ((rc = f64_atb(who, tail, 2, wv, S, ivector_sum, S, 1, S, B, st)) != KTF_OK) return rc;
    if ((rc = f64_atb(who, tail, 2, scat, P, ivector_scatter, P, 1, P, B, st)) != KTF_OK) return rc;
    return f64_atb(who, tail, 2, tail, 2, totals, 2, 1, 2, B, st);                                // (num_ivectors, sum of the scalars)
}

extern "C" int64_t ktf_ivector_acc2_workspace_bytes(int64_t F, int32_t I, int32_t n) {
    const int rc = bucket_check_pairs("ktf_ivector_acc2_workspace_bytes", F, I, n);
    if (rc != KTF_OK) return rc;
    return sec_layout(F > 0 ? F : 1, I, n, true).bytes;
}

extern "C" int ktf_ivector_acc_second_order(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* gauss, const float* post,
                                            int32_t n, float posterior_scale, int32_t I, double* Ssec, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    const char* who = "ktf_ivector_acc_second_order";
    const int64_t need = ktf_ivector_acc2_workspace_bytes(F, I, n);
    if (need < 0) return (int)need;
    KTF_REQUIRE(D >= 1 && D <= KTF_IVECTOR_MAX_FEAT_DIM, "%s: feature dim %d outside 1 .. %d", who, (int)D, KTF_IVECTOR_MAX_FEAT_DIM);
    KTF_REQUIRE(ldx >= D, "%s: ldx %lld < D %d", who, (long long)ldx, (int)D);
    KTF_REQUIRE(posterior_scale >= 0.f, "%s: posterior_scale must be >= 0", who);
    KTF_REQUIRE(Ssec && workspace, "%s: null argument", who);
    KTF_REQUIRE(F == 0 || (x && gauss && post), "%s: null frames / posteriors", who);
    if (ktf_check_workspace(who, workspace, workspace_bytes, need) != KTF_OK) return KTF_EINVAL;
    if (F == 0) return KTF_OK;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const SecLayout l = sec_layout(F, I, n, true);
    const int64_t np = F * n;
    const int* start = (const int*)(ws + l.start);
    const int* pairs = (const int*)(ws + l.pairs);
    const int rc = sec_bucket(who, gauss, np, (int)I, l, ws, st);
    if (rc != KTF_OK) return rc;
    hipLaunchKernelGGL(sec_acc_kernel, dim3(I), dim3(256), 0, st, x, (int)D, ldx, post, (int)n, posterior_scale, start, pairs, Ssec);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
