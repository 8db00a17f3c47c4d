// VB-HMM resegmentation (vb_common.h): the speakers' soft statistics, their update and the block log-likelihoods.
//
//   vb_stats_kernel   N_sc, F_sc: one workgroup per (Gaussian, recording) walks that recording's share of the Gaussian's bucket
//                     (the stable bucketing of gmm_bucket.h) in ascending pair order; thread e owns elements (s, column): no atomics.
//   update            lin = F B and Q = N U (iv_gemm), the blocked Cholesky (iv_solve), C, a and W = C + a a^T (iv_cov),
//   vb_kl_kernel      kl and the triangle weights of g; f64_nt: C = A B^T on v_mfma_f64_16x16x4_f64 for h = a B^T and
//                     g = W' U^T (k ascending, four per MFMA: the bits depend on the operands alone).
//   vb_lls_kernel     one wave per block: lane (s, part) takes a quarter of the D terms of speaker s, frames then slots in order.
#include "vb_common.h"
#include "ivector_stages.h"
#include "f64_mfma.h"
#include "gmm_bucket.h"

namespace {

constexpr int VST_ROWS = 16;        // bucket rows staged in LDS per step
constexpr int VST_ACC = (FBK * (KTF_IVECTOR_MAX_FEAT_DIM + 1) + 255) / 256;   // elements (s, column) per thread

// ---------------------------------------------------------------- soft statistics
// first index in [lo, hi) of the ascending list `pairs` whose value is >= v
__device__ __forceinline__ int vb_lower_bound(const int* __restrict__ pairs, int lo, int hi, int64_t v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)pairs[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Nst (N K, I), Fst (N K, I D): every element is written (zero for an empty share of a bucket)
__global__ void __launch_bounds__(256) vb_stats_kernel(const float* __restrict__ x, int64_t F, int D, int64_t ldx, const int* __restrict__ off,
                                                       const int* __restrict__ boff, int64_t TB, int d, const float* __restrict__ post,
                                                       int n, const int* __restrict__ start, const int* __restrict__ pairs,
                                                       const double* __restrict__ means, const double* __restrict__ q, int K, int I,
                                                       double* __restrict__ Nst, double* __restrict__ Fst) {
    __shared__ double xm[VST_ROWS][KTF_IVECTOR_MAX_FEAT_DIM];
    __shared__ double wq[VST_ROWS][FBK];
    const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    int64_t t0, t1;
    utt_rows(off, r, F, &t0, &t1);
    const int lo = vb_lower_bound(pairs, start[c], start[c + 1], t0 * n);
    const int hi = vb_lower_bound(pairs, lo, start[c + 1], t1 * n);
    const int ncol = D + 1, ne = K * ncol;
    double acc[VST_ACC];
    int es[VST_ACC], ec[VST_ACC];
#pragma unroll
    for (int u = 0; u < VST_ACC; ++u) {
        const int e = tid + 256 * u;
        acc[u] = 0.0;
        es[u] = e < ne ? e / ncol : 0;
        ec[u] = e < ne ? e - es[u] * ncol : 0;
    }
    const int64_t qb0 = boff[r];
    for (int rb = lo; rb < hi; rb += VST_ROWS) {
        const int nr = hi - rb < VST_ROWS ? hi - rb : VST_ROWS;
        for (int e = tid; e < nr * D; e += 256) {
            const int rr = e / D, dd = e - rr * D;
            const int64_t t = pairs[rb + rr] / n;
            xm[rr][dd] = (double)x[t * ldx + dd] - means[(int64_t)c * D + dd];
        }
        for (int e = tid; e < nr * K; e += 256) {
            const int rr = e / K, s = e - rr * K;
            const int p = pairs[rb + rr];
            int64_t qb = qb0 + ((int64_t)(p / n) - t0) / d;
            qb = qb < 0 ? 0 : (qb >= TB ? TB - 1 : qb);
            wq[rr][s] = q[qb * K + s] * (double)post[p];
        }
        __syncthreads();
        for (int rr = 0; rr < nr; ++rr) {
#pragma unroll
            for (int u = 0; u < VST_ACC; ++u)
                if (tid + 256 * u < ne) acc[u] = fma(wq[rr][es[u]], ec[u] < D ? xm[rr][ec[u]] : 1.0, acc[u]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < VST_ACC; ++u)
        if (tid + 256 * u < ne) {
            const int64_t b = (int64_t)r * K + es[u];
            if (ec[u] < D) Fst[(b * I + c) * D + ec[u]] = acc[u];
            else Nst[b * I + c] = acc[u];
        }
}

// ---------------------------------------------------------------- speaker update
__global__ void vb_iota_kernel(int* __restrict__ o, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) o[e] = e;
}

// per speaker row b: kl = (R - tr W) / 2 + sum_j log X_jj (X = L^-1), and Wd = the triangle weights of g = tr(U W) / 2:
// half the diagonal, the off-diagonal entries whole (they count twice)
__global__ void __launch_bounds__(COV_THREADS) vb_kl_kernel(const double* __restrict__ Wp, const double* __restrict__ X, int R,
                                                             double* __restrict__ Wd, double* __restrict__ kl) {
    __shared__ double red[COV_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t P = (int64_t)R * (R + 1) / 2;
    const double* w = Wp + (int64_t)b * P;
    double* wd = Wd + (int64_t)b * P;
    const double* Xb = X + (int64_t)b * R * R;
    for (int64_t e = tid; e < P; e += COV_THREADS) wd[e] = w[e];
    double v = 0.0;
    for (int j = tid; j < R; j += COV_THREADS) v += log(Xb[(int64_t)j * R + j]) - 0.5 * w[(int64_t)j * (j + 1) / 2 + j];
    __syncthreads();
    for (int j = tid; j < R; j += COV_THREADS) wd[(int64_t)j * (j + 1) / 2 + j] = 0.5 * w[(int64_t)j * (j + 1) / 2 + j];
    const double tot = block_sum(v, red, tid);
    if (tid == 0) kl[b] = 0.5 * (double)R + tot;
}

struct UpLayout {
    int64_t lpart, lin, qpart, q, L, wd, tail, off, total;
    int nkl, nkq;
};

UpLayout up_layout(int64_t B, int64_t I, int64_t D, int64_t R) {
    UpLayout l;
    const int64_t P = R * (R + 1) / 2;
    l.nkl = (int)((I * D + GKC - 1) / GKC);
    l.nkq = (int)((I + GKC - 1) / GKC);
    int64_t at = 0;
    l.lpart = at; at += al256(l.nkl * B * R * 8);
    l.lin = at;   at += al256(B * R * 8);
    l.qpart = at; at += al256(l.nkq * B * P * 8);
    l.q = at;     at += al256(B * P * 8);
    l.L = at;     at += al256(B * R * R * 8);
    l.wd = at;    at += al256(B * P * 8);
    l.tail = at;  at += al256(B * 2 * 8);
    l.off = at;   at += al256((B + 1) * 4);
    l.total = at;
    return l;
}

// ---------------------------------------------------------------- block log-likelihood
__global__ void __launch_bounds__(256) vb_lls_kernel(const float* __restrict__ x, int64_t F, int D, int64_t ldx, const int* __restrict__ off,
                                                     const int* __restrict__ boff, int N, int64_t TB, int d, const int* __restrict__ gauss,
                                                     const float* __restrict__ post, int n, int I, const double* __restrict__ means,
                                                     const double* __restrict__ h, const double* __restrict__ g, int K,
                                                     double* __restrict__ lls) {
    const int lane = threadIdx.x & 63, s = lane >> 2, part = lane & 3;
    const int64_t gb = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gb >= TB) return;
    const int r = vb_owner(boff, N, gb);
    if (r < 0) return;
    int64_t t0, t1;
    utt_rows(off, r, F, &t0, &t1);
    const int64_t fa = t0 + (gb - boff[r]) * d;
    const int64_t fe = fa + d < t1 ? fa + d : t1;
    const int64_t row = (int64_t)r * K + (s < K ? s : 0);
    double acc = 0.0;
    for (int64_t t = fa; t < fe; ++t)
        for (int sl = 0; sl < n; ++sl) {
            const int c = gauss[t * n + sl];
            if (c < 0 || c >= I) continue;
            const double p = (double)post[t * n + sl];
            double dot = 0.0;
            if (s < K) {
                const double* hb = h + (row * I + c) * D;
                const double* mc = means + (int64_t)c * D;
                for (int dd = part; dd < D; dd += 4) dot = fma((double)x[t * ldx + dd] - mc[dd], hb[dd], dot);
            }
            dot += __shfl_xor(dot, 1, 64);
            dot += __shfl_xor(dot, 2, 64);
            if (s < K) acc += p * (dot - g[row * I + c]);
        }
    if (s < K && part == 0) lls[gb * K + s] = acc;
}

}  // namespace

extern "C" int ktf_vb_speaker_stats(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* offsets, const int32_t* boffsets, int32_t N,
                                    int64_t TB, int32_t downsample, const float* post, int32_t n, const int32_t* start, const int32_t* pairs,
                                    int32_t I, const double* means, const double* q, int32_t K, double* Nst, double* Fst, void* stream) {
    const char* who = "ktf_vb_speaker_stats";
    int rc = vb_check_tables(who, F, D, ldx, N, TB, downsample, K);
    if (rc != KTF_OK) return rc;
    if ((rc = bucket_check_pairs(who, F, I, n)) != KTF_OK) return rc;
    KTF_REQUIRE(offsets && boffsets && start && means && Nst && Fst, "%s: null argument", who);
    KTF_REQUIRE(F == 0 || (x && post && pairs && q), "%s: null frames / posteriors / q", who);
    if (F == 0 || TB == 0) {
        hipStream_t st0 = (hipStream_t)stream;
        KTF_CHECK_HIP(hipMemsetAsync(Nst, 0, (size_t)N * K * I * 8, st0), who, "hipMemsetAsync");
        KTF_CHECK_HIP(hipMemsetAsync(Fst, 0, (size_t)N * K * I * D * 8, st0), who, "hipMemsetAsync");
        return KTF_OK;
    }
    hipLaunchKernelGGL(vb_stats_kernel, dim3(I, N), dim3(256), 0, (hipStream_t)stream, x, F, (int)D, ldx, offsets, boffsets, TB, (int)downsample,
                       post, (int)n, start, pairs, means, q, (int)K, (int)I, Nst, Fst);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int64_t ktf_vb_update_workspace_bytes(int32_t B, int32_t I, int32_t D, int32_t R) {
    const char* who = "ktf_vb_update_workspace_bytes";
    KTF_REQUIRE(B >= 1 && B <= 65535, "%s: %d speaker rows outside 1 .. 65535", who, (int)B);
    KTF_REQUIRE(I >= 1 && I <= KTF_IVECTOR_MAX_GAUSS, "%s: %d Gaussians outside 1 .. %d", who, (int)I, KTF_IVECTOR_MAX_GAUSS);
    KTF_REQUIRE(D >= 1 && D <= KTF_IVECTOR_MAX_FEAT_DIM, "%s: feature dim %d outside 1 .. %d", who, (int)D, KTF_IVECTOR_MAX_FEAT_DIM);
    KTF_REQUIRE(R >= 1 && R <= KTF_IVECTOR_MAX_DIM, "%s: i-vector dim %d outside 1 .. %d", who, (int)R, KTF_IVECTOR_MAX_DIM);
    return up_layout(B, I, D, R).total;
}

extern "C" int ktf_vb_speaker_update(const double* Nst, const double* Fst, int32_t B, int32_t I, int32_t D, int32_t R, const double* Bm,
                                     const double* U, double* a, double* Wp, double* kl, double* h, double* g, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    const char* who = "ktf_vb_speaker_update";
    const int64_t need = ktf_vb_update_workspace_bytes(B, I, D, R);
    if (need < 0) return (int)need;
    KTF_REQUIRE(Nst && Fst && Bm && U && a && Wp && kl && h && g && workspace, "%s: null argument", who);
    if (ktf_check_workspace(who, workspace, workspace_bytes, need) != KTF_OK) return KTF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const UpLayout l = up_layout(B, I, D, R);
    const int64_t P = (int64_t)R * (R + 1) / 2, ID = (int64_t)I * D;
    double* lin = (double*)(ws + l.lin);
    double* Q = (double*)(ws + l.q);
    double* L = (double*)(ws + l.L);
    double* Wd = (double*)(ws + l.wd);
    double* tail = (double*)(ws + l.tail);
    int* off = (int*)(ws + l.off);
    hipLaunchKernelGGL(vb_iota_kernel, dim3(ktf_cdiv(B + 1, 256)), dim3(256), 0, st, off, (int)B + 1);   // every row "has frames"
    KTF_CHECK_LAUNCH(who);
    int rc = iv_gemm(who, Fst, ID, Bm, R, (double*)(ws + l.lpart), lin, l.nkl, B, R, ID, st);
    if (rc != KTF_OK) return rc;
    if ((rc = iv_gemm(who, Nst, I, U, P, (double*)(ws + l.qpart), Q, l.nkq, B, P, I, st)) != KTF_OK) return rc;
    if ((rc = iv_solve(who, Q, lin, off, (int)B, (int64_t)B, (int)R, 0.0, L, a, 8, st)) != KTF_OK) return rc;
    if ((rc = iv_cov(who, lin, off, (int)B, (int64_t)B, (int)R, 0.0, L, Wp, a, tail, st)) != KTF_OK) return rc;
    hipLaunchKernelGGL(vb_kl_kernel, dim3(B), dim3(COV_THREADS), 0, st, (const double*)Wp, (const double*)L, (int)R, Wd, kl);
    KTF_CHECK_LAUNCH(who);
    if ((rc = f64_nt(who, a, R, Bm, R, h, ID, B, ID, R, st)) != KTF_OK) return rc;                // h_sc = (B rows of c) a_s
    return f64_nt(who, Wd, P, U, P, g, I, B, I, P, st);                                           // g_sc = tr(U_c W_s) / 2
}

extern "C" int ktf_vb_block_loglike(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* offsets, const int32_t* boffsets, int32_t N,
                                    int64_t TB, int32_t downsample, const int32_t* gauss, const float* post, int32_t n, int32_t I,
                                    const double* means, const double* h, const double* g, int32_t K, double* lls, void* stream) {
    const char* who = "ktf_vb_block_loglike";
    int rc = vb_check_tables(who, F, D, ldx, N, TB, downsample, K);
    if (rc != KTF_OK) return rc;
    if ((rc = bucket_check_pairs(who, F, I, n)) != KTF_OK) return rc;
    KTF_REQUIRE(offsets && boffsets && means && h && g, "%s: null argument", who);
    KTF_REQUIRE(TB == 0 || (x && gauss && post && lls), "%s: null frames / posteriors / output", who);
    if (TB == 0) return KTF_OK;
    hipLaunchKernelGGL(vb_lls_kernel, dim3((unsigned)((TB + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, F, (int)D, ldx, offsets, boffsets, (int)N,
                       TB, (int)downsample, gauss, post, (int)n, (int)I, means, h, g, (int)K, lls);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
