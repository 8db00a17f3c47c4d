// Adaptive symmetric score normalisation (S-norm / AS-norm, Matejka et al. 2017): mean and standard deviation of the top_n largest
// entries of each row of a score block (ktf_topn_stats_*), and the same on the PLDA scores of R vectors against a cohort, formed
// row chunk by row chunk in a workspace the caller bounds (ktf_plda_cohort_stats_*).
//
// Selection, one 256-thread workgroup per row: every score maps to an unsigned key whose integer order is the order of the values
// (non-negatives get the sign bit set, negatives are inverted), and the top_n-th largest key is found by radix select from the most
// significant byte down (8 passes in fp64, 4 in fp32): a 256-bin LDS histogram of the byte among the keys that share the prefix
// found so far (integer LDS atomics only), then one wave scans the bins from 255 down, picks the bin that holds the wanted rank
// and leaves the rank within it. After the last pass the prefix is the threshold T itself and the remaining rank k is the number
// of copies of T the selection takes: the selected multiset is {x > T} and k times T, whatever the ties.
//   mean = T + sum_{x > T} (x - T) / N            (about the pivot T: an all-tied selection has mean T exactly, hence std 0 exactly)
//   std  = sqrt((sum_{x > T} (x - mean)^2 + k (T - mean)^2) / N)                  (centred, a second pass; population form)
// top_n >= C selects the whole row: no select, the pivot is the row's first value. Sums are fp64 whatever the dtype: thread t adds
// the terms of columns t, t + 256, ... in order, a fixed butterfly adds the lanes of a wave, the four wave sums are added in order.
// No floating-point atomics: a row's result depends on its values in order, C, top_n and the dtype alone.
// A row of at most TOPN_STAGE_BYTES is staged in LDS once; a longer one is read again from global memory in each pass (it is the
// workgroup's only traffic and stays in the L2). A NaN is a key like any other: the passes are counted, the bins masked.
#include "plda_common.h"

namespace {

constexpr int TOPN_STAGE_BYTES = 32 * 1024;

template <typename R> struct KeyOf;
template <> struct KeyOf<double> { typedef unsigned long long K; };
template <> struct KeyOf<float> { typedef unsigned int K; };

template <typename R>
__device__ __forceinline__ typename KeyOf<R>::K to_key(R v) {
    typedef typename KeyOf<R>::K K;
    constexpr K sign = (K)1 << (8 * sizeof(K) - 1);
    K b;
    __builtin_memcpy(&b, &v, sizeof(K));
    return (b & sign) ? ~b : (b | sign);
}
template <typename R>
__device__ __forceinline__ R from_key(typename KeyOf<R>::K k) {
    typedef typename KeyOf<R>::K K;
    constexpr K sign = (K)1 << (8 * sizeof(K) - 1);
    const K b = (k & sign) ? (k ^ sign) : ~k;
    R v;
    __builtin_memcpy(&v, &b, sizeof(K));
    return v;
}

// the workgroup's sum of v: wave butterflies, then the four wave sums in order (red: 4 doubles of LDS, free on entry of every thread
// once the barrier inside has been passed)
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

template <typename R, bool STAGED>
__global__ __launch_bounds__(256) void topn_stats_kernel(const R* __restrict__ x, int C, int64_t ld, int top_n,
                                                         double* __restrict__ mean, double* __restrict__ std_) {
    typedef typename KeyOf<R>::K K;
    constexpr int NB = (int)sizeof(K);
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];      // STAGED: the row
    __shared__ unsigned hist[256];
    __shared__ int pick[2];
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const R* row = x + (int64_t)blockIdx.x * ld;
    R* srow = reinterpret_cast<R*>(smraw);
    if (tid == 0) { pick[0] = 0; pick[1] = 1; }
    if constexpr (STAGED) {
        for (int i = tid; i < C; i += 256) srow[i] = row[i];
    }
    __syncthreads();
    auto at = [&](int i) -> R {
        if constexpr (STAGED) return srow[i];
        else return row[i];
    };
    const bool all = top_n >= C;
    const int N = all ? C : top_n;
    K tkey = 0;
    int k = N;                                                     // the rank wanted among the keys that share the prefix, 1 = largest
    if (!all) {
        for (int p = 0; p < NB; ++p) {
            const int shift = 8 * (NB - 1 - p);
            hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < C; i += 256) {
                const K key = to_key<R>(at(i));
                if (p == 0 || (key >> (shift + 8)) == (tkey >> (shift + 8))) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid < 64) {                                        // lane l owns bins 255 - 4 l down to 252 - 4 l
                unsigned h[4], s = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    h[q] = hist[255 - 4 * tid - q];
                    s += h[q];
                }
                unsigned inc = s;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned t = __shfl_up(inc, o, 64);
                    if (tid >= o) inc += t;
                }
                unsigned below = inc - s;                          // keys in the bins above this lane's
                if ((unsigned)k > below && (unsigned)k <= inc) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if ((unsigned)k > below && (unsigned)k <= below + h[q]) {
                            pick[0] = 255 - 4 * tid - q;
                            pick[1] = k - (int)below;
                        }
                        below += h[q];
                    }
                }
            }
            __syncthreads();
            tkey |= (K)(pick[0] & 255) << shift;
            k = pick[1];
        }
    }
    const double piv = (double)(all ? at(0) : from_key<R>(tkey));
    double s = 0.0;
    for (int i = tid; i < C; i += 256) {
        const R v = at(i);
        if (all || to_key<R>(v) > tkey) s += (double)v - piv;
    }
    s = block_sum_d(s, red);
    const double m = piv + s / (double)N;
    double q = 0.0;
    for (int i = tid; i < C; i += 256) {
        const R v = at(i);
        if (all || to_key<R>(v) > tkey) {
            const double d = (double)v - m;
            q += d * d;
        }
    }
    q = block_sum_d(q, red);
    if (!all) {
        const double d = piv - m;
        q += (double)k * (d * d);
    }
    if (tid == 0) {
        mean[blockIdx.x] = m;
        std_[blockIdx.x] = sqrt(q / (double)N);
    }
}

template <typename R>
static int topn_launch(const char* who, const R* x, int64_t R_, int64_t C, int64_t ld, int32_t top_n, double* mean, double* std_,
                       void* stream) {
    KTF_REQUIRE(R_ >= 0 && R_ < (1ll << 31), "%s: R = %lld outside 0..2^31 - 1", who, (long long)R_);
    KTF_REQUIRE(C >= 1 && C < (1ll << 31), "%s: C = %lld outside 1..2^31 - 1", who, (long long)C);
    KTF_REQUIRE(ld >= C, "%s: row stride %lld below C = %lld", who, (long long)ld, (long long)C);
    KTF_REQUIRE(top_n >= 1, "%s: top_n = %d, must be >= 1 (INT32_MAX: the whole row)", who, (int)top_n);
    if (R_ == 0) return KTF_OK;
    KTF_REQUIRE(x && mean && std_, "%s: null argument", who);
    hipStream_t st = (hipStream_t)stream;
    if (C * (int64_t)sizeof(R) <= TOPN_STAGE_BYTES)
        hipLaunchKernelGGL((topn_stats_kernel<R, true>), dim3((unsigned)R_), dim3(256), (size_t)C * sizeof(R), st, x, (int)C, ld,
                           (int)top_n, mean, std_);
    else
        hipLaunchKernelGGL((topn_stats_kernel<R, false>), dim3((unsigned)R_), dim3(256), 0, st, x, (int)C, ld, (int)top_n, mean, std_);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

// The score block of a cohort side, one 64 x 64 tile per workgroup (plda_score_tile: the bits of ktf_plda_score_* / _score_n_*).
// y: the vectors scored as tests, yc: the classes; SWAP: the block is stored with the class as its row.
template <typename R, bool PER_CLASS, bool SWAP>
__global__ __launch_bounds__(256) void cohort_score_kernel(const R* __restrict__ y, int64_t B, const R* __restrict__ yc, int64_t Bc,
                                                           int dim, const R* __restrict__ psi, const R* __restrict__ cnt,
                                                           R* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    plda_score_tile<R, PER_CLASS, SWAP>(y, B, yc, Bc, dim, psi, scores, (int64_t)blockIdx.y * PLDA_TILE, (int64_t)blockIdx.x * PLDA_TILE,
                                        smraw, cnt);
}

template <typename R, bool PER_CLASS, bool SWAP>
static void cohort_score_launch(const R* y, int64_t B, const R* yc, int64_t Bc, int dim, const R* psi, const R* cnt, R* scores,
                                hipStream_t st) {
    const size_t lds = PER_CLASS ? PLDA_N_LDS_BYTES(R) : PLDA_LDS_BYTES(R);
    dim3 grid((unsigned)ktf_cdiv(Bc, PLDA_TILE), (unsigned)ktf_cdiv(B, PLDA_TILE));
    KTF_LDS_ONCE((int)lds, cohort_score_kernel<R, PER_CLASS, SWAP>);
    hipLaunchKernelGGL((cohort_score_kernel<R, PER_CLASS, SWAP>), grid, dim3(256), lds, st, y, B, yc, Bc, dim, psi, cnt, scores);
}

template <typename R>
static int cohort_launch(const char* who, const R* rows, int64_t R_, const R* cohort, int64_t C, int32_t dim, const R* psi,
                         const R* counts, int32_t role, int32_t top_n, double* mean, double* std_, void* workspace,
                         size_t workspace_bytes, void* stream) {
    KTF_REQUIRE(role == 0 || role == 1, "%s: role %d (0: the rows are tests, 1: the rows are classes)", who, (int)role);
    KTF_REQUIRE(R_ >= 0 && R_ < (1ll << 31), "%s: R = %lld outside 0..2^31 - 1", who, (long long)R_);
    KTF_REQUIRE(C >= 1 && C < (1ll << 31) && dim > 0, "%s: bad sizes (1 <= C < 2^31, dim > 0)", who);
    KTF_REQUIRE(top_n >= 1, "%s: top_n = %d, must be >= 1 (INT32_MAX: the whole cohort)", who, (int)top_n);
    if (R_ == 0) return KTF_OK;
    KTF_REQUIRE(rows && cohort && psi && mean && std_ && workspace, "%s: null argument", who);
    // grid.y runs over the vectors scored as tests: the rows (role 0) or the cohort (role 1)
    KTF_REQUIRE(ktf_cdiv(role == 0 ? R_ : C, PLDA_TILE) < 65536, "%s: too many %s (chunk them)", who, role == 0 ? "rows" : "cohort vectors");
    const int rc = ktf_check_workspace(who, workspace, workspace_bytes, ktf_plda_cohort_workspace_bytes(R_, C, dim, (int32_t)sizeof(R)));
    if (rc != KTF_OK) return rc;
    R* scores = reinterpret_cast<R*>(workspace);                   // (R, C): the row entity's C scores side by side
    hipStream_t st = (hipStream_t)stream;
    if (role == 0) {
        if (counts) cohort_score_launch<R, true, false>(rows, R_, cohort, C, dim, psi, counts, scores, st);
        else cohort_score_launch<R, false, false>(rows, R_, cohort, C, dim, psi, counts, scores, st);
    } else {
        if (counts) cohort_score_launch<R, true, true>(cohort, C, rows, R_, dim, psi, counts, scores, st);
        else cohort_score_launch<R, false, true>(cohort, C, rows, R_, dim, psi, counts, scores, st);
    }
    KTF_CHECK_LAUNCH(who);
    return topn_launch<R>(who, scores, R_, C, C, top_n, mean, std_, stream);
}

}  // namespace

extern "C" int ktf_topn_stats_f64(const double* x, int64_t R, int64_t C, int64_t ld, int32_t top_n, double* mean, double* std,
                                  void* stream) {
    return topn_launch<double>("ktf_topn_stats_f64", x, R, C, ld, top_n, mean, std, stream);
}
extern "C" int ktf_topn_stats_f32(const float* x, int64_t R, int64_t C, int64_t ld, int32_t top_n, double* mean, double* std,
                                  void* stream) {
    return topn_launch<float>("ktf_topn_stats_f32", x, R, C, ld, top_n, mean, std, stream);
}

extern "C" int64_t ktf_plda_cohort_workspace_bytes(int64_t R, int64_t C, int32_t dim, int32_t dtype_bytes) {
    if (R < 0 || C < 1 || dim <= 0 || (dtype_bytes != 4 && dtype_bytes != 8)) return KTF_EINVAL;
    if (R > 0 && C > INT64_MAX / 8 / R) return KTF_EINVAL;
    return R * C * (int64_t)dtype_bytes;
}
extern "C" int ktf_plda_cohort_stats_f64(const double* rows_tr, int64_t R, const double* cohort_tr, int64_t C, int32_t dim,
                                         const double* psi, const double* counts, int32_t role, int32_t top_n, double* mean,
                                         double* std, void* workspace, size_t workspace_bytes, void* stream) {
    return cohort_launch<double>("ktf_plda_cohort_stats_f64", rows_tr, R, cohort_tr, C, dim, psi, counts, role, top_n, mean, std, workspace,
                                 workspace_bytes, stream);
}
extern "C" int ktf_plda_cohort_stats_f32(const float* rows_tr, int64_t R, const float* cohort_tr, int64_t C, int32_t dim,
                                         const float* psi, const float* counts, int32_t role, int32_t top_n, double* mean, double* std,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    return cohort_launch<float>("ktf_plda_cohort_stats_f32", rows_tr, R, cohort_tr, C, dim, psi, counts, role, top_n, mean, std, workspace,
                                workspace_bytes, stream);
}
