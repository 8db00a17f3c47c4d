// UBM training statistics: the E-steps and accumulators of Kaldi's gmm-global-init-from-feats, gmm-global-acc-stats --gselect and
// fgmm-global-acc-stats --gselect (the updates run in fp64 NumPy on the host, kaldi_tflite_amd/training.py).
//
//   gpre_kernel       one wave per frame, one listed Gaussian per lane: the fp32 diagonal log-likelihood in ascending d, softmax
//                     over the list in slot order, the frame's log-likelihood, the count of frames with a non-empty list.
//   gdense_ll_kernel  (gmm_loglike.hip) the log-likelihoods of ALL Gaussians on the tile of gmm_loglike.h (the bits of
//   gdense_sm_kernel  ktf_ivector_post_f32), written to the workspace (F, I); then one wave per frame: softmax over all I, P (fp64),
//                     Xaug = [1, x, x^2] (fp64).
//   gmm_bucket.hip    the pairs bucketed by Gaussian, the buckets cut into items of KTF_GMM_ACC_ITEM_ROWS rows: item starts and,
//                     for the Gaussians with more than one item, the starts of their partial results.
//   gacc_diag_kernel  one workgroup per item, VALU fp64: wave w takes the item's rows r = w (mod 4) in order, lane l the columns
//                     l and l + 64; the four waves' sums are added in wave order.
//   gacc_full_kernel  one workgroup per item: Z^T diag(p) Z with z = [1, x] on v_mfma_f64_16x16x4_f64. GACC_RB rows at a time are
//                     gathered into LDS as fp64; the lower-triangle 16 x 16 tiles of the product are dealt out to the four waves
//                     (tile t to wave t mod 4), A = p z (exact in fp64) and B = z read from LDS, four rows per MFMA in ascending row
//                     order. Element (0, 0) is occ, column 0 mean_acc, the rest cov_acc; the upper triangle is the mirror.
//   gacc_reduce_kernel  per Gaussian with more than one item: its partials added in ascending item order, then into the accumulator.
// An item of a Gaussian with a single item adds straight into the accumulator (the same sum). No floating-point atomics anywhere.
#include "gmm_bucket.h"
#include "gmm_loglike.h"
#include "f64_mfma.h"

namespace {

constexpr int GACC_THREADS = 256;
constexpr int GACC_WAVES = GACC_THREADS / 64;
constexpr int GACC_RB = 32;                               // rows gathered per stage of the full form
constexpr int GACC_MAX_NT = (KTF_IVECTOR_MAX_FEAT_DIM + 1 + 15) / 16;   // 16-wide tiles along z = [1, x]: 9
constexpr int GPRE_WAVES = 4;

inline int gacc_nt(int D) { return (D + 1 + 15) / 16; }
// doubles of one partial result: [occ, mean_acc, var_acc] or the (D + 1)^2 square whose lower triangle is written
inline int64_t gacc_stride(int D, int full) { return full ? (int64_t)(D + 1) * (D + 1) : 2 * (int64_t)D + 1; }

struct GaccLayout {
    SecLayout sec;
    int64_t istart, pstart, part, total, max_items, max_parts;
};

GaccLayout gacc_layout(int64_t F, int64_t I, int64_t D, int64_t n, int full) {
    GaccLayout l;
    l.sec = sec_layout(F > 0 ? F : 1, I, n, true);
    const int64_t np = F * n;
    l.max_items = np / KTF_GMM_ACC_ITEM_ROWS + I;          // sum of ceil(count / rows) over the Gaussians
    l.max_parts = 2 * (np / KTF_GMM_ACC_ITEM_ROWS) + 1;    // a Gaussian with count > rows has ceil(count / rows) < 2 count / rows items
    int64_t at = l.sec.bytes;
    l.istart = at; at += al256((I + 1) * 4);
    l.pstart = at; at += al256((I + 1) * 4);
    l.part = at;   at += al256(l.max_parts * gacc_stride((int)D, full) * 8);
    l.total = at;
    return l;
}

// ---------------------------------------------------------------- (a) posteriors on a preselected list
__global__ void __launch_bounds__(64 * GPRE_WAVES) gpre_kernel(const float* __restrict__ x, int64_t F, int D, int64_t ldx,
                                                               const int* __restrict__ gsel, int n, const float* __restrict__ mi,
                                                               const float* __restrict__ iv, const float* __restrict__ gconst, int I,
                                                               float* __restrict__ post, float* __restrict__ loglike, int* __restrict__ valid) {
    __shared__ float xs[GPRE_WAVES][KTF_IVECTOR_MAX_FEAT_DIM];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * GPRE_WAVES + wv;
    if (t >= F) return;                                      // (no workgroup barrier below: a wave works alone)
    for (int d = lane; d < D; d += 64) xs[wv][d] = x[t * ldx + d];
    wave_lds_sync();
    int g = -1;
    if (lane < n) {
        g = gsel[t * n + lane];
        if (g < 0 || g >= I) g = -1;
    }
    float l = -INFINITY;
    if (g >= 0) {
        const float* mg = mi + (int64_t)g * D;
        const float* vg = iv + (int64_t)g * D;
        float acc = gconst[g];
        for (int d = 0; d < D; ++d) {
            const float xd = xs[wv][d];
            acc = fmaf(xd, mg[d], acc);
            acc = fmaf(-0.5f * (xd * xd), vg[d], acc);
        }
        l = acc;
    }
    float mx = l;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const bool any = mx > -INFINITY;                         // nothing listed, or every listed l is -inf: an empty list
    const float e = (g >= 0 && any) ? expf(l - mx) : 0.f;
    const float tot = wave_sum(e);
    if (lane < n) post[t * n + lane] = any ? e / tot : 0.f;
    if (lane == 0) {
        loglike[t] = any ? mx + logf(tot) : 0.f;
        if (valid && any) atomicAdd(valid, 1);               // an integer count: the order of the adds cannot change it
    }
}

// ---------------------------------------------------------------- (b) dense posteriors
// one wave per frame; lane l owns the Gaussians l, l + 64, ...: its sum in that order, then the butterfly
__global__ void __launch_bounds__(64 * GPRE_WAVES) gdense_sm_kernel(const float* __restrict__ x, int64_t F, int D, int64_t ldx,
                                                                    const float* __restrict__ ll, int I, double* __restrict__ P,
                                                                    double* __restrict__ Xaug, float* __restrict__ loglike) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * GPRE_WAVES + (threadIdx.x >> 6);
    if (t >= F) return;
    const float* lt = ll + t * I;
    float mx = -INFINITY;
    for (int g = lane; g < I; g += 64) mx = fmaxf(mx, lt[g]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const bool any = mx > -INFINITY;
    float s = 0.f;
    if (any)
        for (int g = lane; g < I; g += 64) s += expf(lt[g] - mx);
    const float tot = wave_sum(s);
    for (int g = lane; g < I; g += 64) P[t * I + g] = any ? (double)(expf(lt[g] - mx) / tot) : 0.0;
    const int C = 2 * D + 1;
    for (int c = lane; c < C; c += 64) {
        double v = 1.0;
        if (c >= 1) {
            const double xv = (double)x[t * ldx + (c <= D ? c - 1 : c - 1 - D)];
            v = c <= D ? xv : xv * xv;                       // exact: 24-bit factors
        }
        Xaug[t * C + c] = v;
    }
    if (lane == 0) loglike[t] = any ? mx + logf(tot) : 0.f;
}

// ---------------------------------------------------------------- (d) statistics on (frame, slot) pairs
// element (i, j), j <= i, of sum p z z^T -> the accumulators (z = [1, x]); the mirror gets the same value
__device__ __forceinline__ void gacc_emit_full(int i, int j, double v, int g, int D, double* __restrict__ occ, double* __restrict__ mean,
                                               double* __restrict__ cov) {
    if (i == 0) occ[g] += v;
    else if (j == 0) mean[(int64_t)g * D + i - 1] += v;
    else {
        double* c = cov + (int64_t)g * D * D;
        c[(int64_t)(i - 1) * D + j - 1] += v;
        if (i != j) c[(int64_t)(j - 1) * D + i - 1] += v;
    }
}

__device__ __forceinline__ void gacc_emit_diag(int c, double v, int g, int D, double* __restrict__ occ, double* __restrict__ mean,
                                               double* __restrict__ var) {
    if (c == 0) occ[g] += v;
    else if (c <= D) mean[(int64_t)g * D + c - 1] += v;
    else var[(int64_t)g * D + c - 1 - D] += v;
}

__global__ void __launch_bounds__(GACC_THREADS) gacc_diag_kernel(const float* __restrict__ x, int D, int64_t ldx, const float* __restrict__ post,
                                                                 int n, const int* __restrict__ start, const int* __restrict__ pairs,
                                                                 const int* __restrict__ istart, const int* __restrict__ pstart, int I,
                                                                 double* __restrict__ occ, double* __restrict__ mean, double* __restrict__ var,
                                                                 double* __restrict__ part) {
    __shared__ double red[GACC_WAVES][2 * KTF_IVECTOR_MAX_FEAT_DIM + 1];
    const BucketItem it = bucket_item(blockIdx.x, start, istart, I, KTF_GMM_ACC_ITEM_ROWS);
    if (it.g < 0) return;
    const int slot = it.items > 1 ? pstart[it.g] + it.k : -1;        // of its partial result; a single item adds to the accumulator
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double o = 0.0, m[2] = {0.0, 0.0}, s[2] = {0.0, 0.0};
    for (int r = it.r0 + wv; r < it.r1; r += GACC_WAVES) {
        const int pid = pairs[r];
        const double p = (double)post[pid];
        if (p == 0.0) continue;                              // a zero weight: the slot is skipped (wave-uniform)
        const float* xr = x + (int64_t)(pid / n) * ldx;
        o += p;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int d = lane + 64 * q;
            const double xv = d < D ? (double)xr[d] : 0.0;
            m[q] = fma(p, xv, m[q]);
            s[q] = fma(p, xv * xv, s[q]);                    // x^2 is exact in fp64
        }
    }
    if (lane == 0) red[wv][0] = o;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int d = lane + 64 * q;
        if (d < D) {
            red[wv][1 + d] = m[q];
            red[wv][1 + D + d] = s[q];
        }
    }
    __syncthreads();
    const int C = 2 * D + 1;
    for (int c = tid; c < C; c += GACC_THREADS) {
        double v = red[0][c];
#pragma unroll
        for (int w = 1; w < GACC_WAVES; ++w) v += red[w][c];
        if (slot >= 0) part[(int64_t)slot * C + c] = v;
        else gacc_emit_diag(c, v, it.g, D, occ, mean, var);
    }
}

// NT = ceil((D + 1) / 16) tiles along z; TPW lower-triangle tiles per wave: 4 * TPW fp64 accumulators per lane (at most 48)
template <int NT>
__global__ void __launch_bounds__(GACC_THREADS) gacc_full_kernel(const float* __restrict__ x, int D, int64_t ldx, const float* __restrict__ post,
                                                                 int n, const int* __restrict__ start, const int* __restrict__ pairs,
                                                                 const int* __restrict__ istart, const int* __restrict__ pstart, int I,
                                                                 double* __restrict__ occ, double* __restrict__ mean, double* __restrict__ cov,
                                                                 double* __restrict__ part) {
    constexpr int ZP = 16 * NT;
    constexpr int NTILES = NT * (NT + 1) / 2;
    constexpr int TPW = (NTILES + GACC_WAVES - 1) / GACC_WAVES;
    __shared__ double zs[GACC_RB][ZP];
    __shared__ double ps[GACC_RB];
    const BucketItem it = bucket_item(blockIdx.x, start, istart, I, KTF_GMM_ACC_ITEM_ROWS);
    if (it.g < 0) return;
    const int slot = it.items > 1 ? pstart[it.g] + it.k : -1;        // of its partial result; a single item adds to the accumulator
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lc = lane & 15, lk = lane >> 4;
    const int Dz = D + 1;
    int ti[TPW], tj[TPW];
#pragma unroll
    for (int s = 0; s < TPW; ++s) {
        const int t = wv + GACC_WAVES * s;
        int a = 0;
        while ((a + 1) * (a + 2) / 2 <= t) ++a;
        ti[s] = a;
        tj[s] = t - a * (a + 1) / 2;
    }
    f64x4 acc[TPW];
#pragma unroll
    for (int s = 0; s < TPW; ++s) acc[s] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int rb = it.r0; rb < it.r1; rb += GACC_RB) {
        if (tid < GACC_RB) ps[tid] = rb + tid < it.r1 ? (double)post[pairs[rb + tid]] : 0.0;
        for (int e = tid; e < GACC_RB * ZP; e += GACC_THREADS) {
            const int r = e / ZP, c = e - r * ZP;
            double v = 0.0;
            if (rb + r < it.r1 && c < Dz) {
                const int pid = pairs[rb + r];
                if (post[pid] != 0.f) v = c == 0 ? 1.0 : (double)x[(int64_t)(pid / n) * ldx + c - 1];   // a zero weight: skipped
            }
            zs[r][c] = v;
        }
        __syncthreads();
#pragma unroll
        for (int k0 = 0; k0 < GACC_RB; k0 += 4) {
            if (rb + k0 >= it.r1) break;
            const double pk = ps[k0 + lk];
#pragma unroll
            for (int s = 0; s < TPW; ++s) {
                if (wv + GACC_WAVES * s < NTILES) {
                    const double a = pk * zs[k0 + lk][16 * ti[s] + lc];       // exact: 24-bit factors
                    const double b = zs[k0 + lk][16 * tj[s] + lc];
                    acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[s], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    // result reg r of lane l is element (16 ti + (l >> 4) + 4 r, 16 tj + (l & 15)); the lower triangle only
#pragma unroll
    for (int s = 0; s < TPW; ++s) {
        if (wv + GACC_WAVES * s >= NTILES) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 16 * ti[s] + lk + 4 * r, j = 16 * tj[s] + lc;
            if (i < Dz && j <= i) {
                if (slot >= 0) part[((int64_t)slot * Dz + i) * Dz + j] = acc[s][r];
                else gacc_emit_full(i, j, acc[s][r], it.g, D, occ, mean, cov);
            }
        }
    }
}

// one workgroup column per Gaussian: elements e of the partial (the lower triangle for the full form), items ascending
__global__ void __launch_bounds__(256) gacc_reduce_kernel(const double* __restrict__ part, const int* __restrict__ istart,
                                                          const int* __restrict__ pstart, int D, int full, double* __restrict__ occ,
                                                          double* __restrict__ mean, double* __restrict__ second) {
    const int g = blockIdx.x;
    const int ni = istart[g + 1] - istart[g];
    if (ni <= 1) return;
    const int Dz = D + 1;
    const int64_t stride = full ? (int64_t)Dz * Dz : 2 * (int64_t)D + 1;
    const double* p0 = part + (int64_t)pstart[g] * stride;
    for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < stride; e += (int64_t)gridDim.y * 256) {
        const int i = full ? (int)(e / Dz) : 0, j = full ? (int)(e - (int64_t)i * Dz) : 0;
        if (full && j > i) continue;
        double v = p0[e];
        for (int k = 1; k < ni; ++k) v += p0[(int64_t)k * stride + e];
        if (full) gacc_emit_full(i, j, v, g, D, occ, mean, second);
        else gacc_emit_diag((int)e, v, g, D, occ, mean, second);
    }
}

template <int NT>
void gacc_launch_full(int items, hipStream_t st, const float* x, int D, int64_t ldx, const float* post, int n, const int* start,
                      const int* pairs, const int* istart, const int* pstart, int I, double* occ, double* mean, double* cov, double* part) {
    hipLaunchKernelGGL(gacc_full_kernel<NT>, dim3(items), dim3(GACC_THREADS), 0, st, x, D, ldx, post, n, start, pairs, istart, pstart, I, occ,
                       mean, cov, part);
}

}  // namespace

extern "C" int ktf_gmm_post_preselect_f32(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* gselect, int32_t n,
                                          const float* means_invvars, const float* inv_vars, const float* gconst, int32_t I, float* post,
                                          float* loglike, int32_t* valid, void* stream) {
    const char* who = "ktf_gmm_post_preselect_f32";
    const int rc = bucket_check_shape(who, F, I, D, n);
    if (rc != KTF_OK) return rc;
    KTF_REQUIRE(ldx >= D, "%s: ldx %lld < D %d", who, (long long)ldx, (int)D);
    if (F == 0) return KTF_OK;
    KTF_REQUIRE(x && gselect && means_invvars && inv_vars && gconst && post && loglike, "%s: null argument", who);
    hipLaunchKernelGGL(gpre_kernel, dim3((unsigned)((F + GPRE_WAVES - 1) / GPRE_WAVES)), dim3(64 * GPRE_WAVES), 0, (hipStream_t)stream, x, F,
                       (int)D, ldx, gselect, (int)n, means_invvars, inv_vars, gconst, (int)I, post, loglike, valid);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int64_t ktf_gmm_post_dense_workspace_bytes(int64_t F, int32_t I) {
    const char* who = "ktf_gmm_post_dense_workspace_bytes";
    KTF_REQUIRE(I >= 1 && I <= KTF_IVECTOR_MAX_GAUSS, "%s: %d Gaussians outside 1 .. %d", who, (int)I, KTF_IVECTOR_MAX_GAUSS);
    KTF_REQUIRE(F >= 0 && F < ((int64_t)1 << 31), "%s: frame count %lld out of range", who, (long long)F);
    return al256((F > 0 ? F : 1) * I * 4);
}

extern "C" int ktf_gmm_post_dense_f32(const float* x, int64_t F, int32_t D, int64_t ldx, const float* W, const float* gconst, int32_t I,
                                      double* P, double* Xaug, float* loglike, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_gmm_post_dense_f32";
    const int64_t need = ktf_gmm_post_dense_workspace_bytes(F, I);
    if (need < 0) return (int)need;
    KTF_REQUIRE(D >= 1 && D <= KTF_IVECTOR_MAX_FEAT_DIM, "%s: feature dim %d outside 1 .. %d", who, (int)D, KTF_IVECTOR_MAX_FEAT_DIM);
    KTF_REQUIRE(ldx >= D, "%s: ldx %lld < D %d", who, (long long)ldx, (int)D);
    if (F == 0) return KTF_OK;
    KTF_REQUIRE(x && W && gconst && P && Xaug && loglike && workspace, "%s: null argument", who);
    if (ktf_check_workspace(who, workspace, workspace_bytes, need) != KTF_OK) return KTF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    float* ll = (float*)workspace;
    const int rc = gmm_dense_loglike(who, x, F, (int)D, ldx, W, gconst, (int)I, ll, st);
    if (rc != KTF_OK) return rc;
    hipLaunchKernelGGL(gdense_sm_kernel, dim3((unsigned)((F + GPRE_WAVES - 1) / GPRE_WAVES)), dim3(64 * GPRE_WAVES), 0, st, x, F, (int)D, ldx,
                       (const float*)ll, (int)I, P, Xaug, loglike);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int64_t ktf_gmm_acc_workspace_bytes(int64_t F, int32_t I, int32_t D, int32_t n, int32_t full) {
    const int rc = bucket_check_shape("ktf_gmm_acc_workspace_bytes", F, I, D, n);
    if (rc != KTF_OK) return rc;
    return gacc_layout(F, I, D, n, full != 0).total;
}

extern "C" int ktf_gmm_acc_f64(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* gauss, const float* post, int32_t n, int32_t I,
                               int32_t full, double* occ, double* mean_acc, double* second_acc, void* workspace, size_t workspace_bytes,
                               void* stream) {
    const char* who = "ktf_gmm_acc_f64";
    int rc = bucket_check_shape(who, F, I, D, n);
    if (rc != KTF_OK) return rc;
    KTF_REQUIRE(ldx >= D, "%s: ldx %lld < D %d", who, (long long)ldx, (int)D);
    KTF_REQUIRE(occ && mean_acc && second_acc && workspace, "%s: null argument", who);
    KTF_REQUIRE(F == 0 || (x && gauss && post), "%s: null frames / posteriors", who);
    const GaccLayout l = gacc_layout(F, I, D, n, full != 0);
    if (ktf_check_workspace(who, workspace, workspace_bytes, l.total) != KTF_OK) return KTF_EINVAL;
    if (F == 0) return KTF_OK;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int* start = (const int*)(ws + l.sec.start);
    const int* pairs = (const int*)(ws + l.sec.pairs);
    int* istart = (int*)(ws + l.istart);
    int* pstart = (int*)(ws + l.pstart);
    double* part = (double*)(ws + l.part);
    if ((rc = sec_bucket(who, gauss, F * n, (int)I, l.sec, ws, st)) != KTF_OK) return rc;
    if ((rc = bucket_items(who, start, (int)I, KTF_GMM_ACC_ITEM_ROWS, istart, pstart, st)) != KTF_OK) return rc;
    const int items = (int)l.max_items;
#define KTF_GACC_FULL(NT)                                                                                                              \
    case NT:                                                                                                                           \
        gacc_launch_full<NT>(items, st, x, (int)D, ldx, post, (int)n, start, pairs, istart, pstart, (int)I, occ, mean_acc, second_acc, \
                             part);                                                                                                    \
        break
    if (full) {
        static_assert(GACC_MAX_NT == 9, "one case per tile count");
        switch (gacc_nt(D)) {
            KTF_GACC_FULL(1);
            KTF_GACC_FULL(2);
            KTF_GACC_FULL(3);
            KTF_GACC_FULL(4);
            KTF_GACC_FULL(5);
            KTF_GACC_FULL(6);
            KTF_GACC_FULL(7);
            KTF_GACC_FULL(8);
            default: KTF_GACC_FULL(9);
        }
    } else {
        hipLaunchKernelGGL(gacc_diag_kernel, dim3(items), dim3(GACC_THREADS), 0, st, x, (int)D, ldx, post, (int)n, start, pairs,
                           (const int*)istart, (const int*)pstart, (int)I, occ, mean_acc, second_acc, part);
    }
#undef KTF_GACC_FULL
    KTF_CHECK_LAUNCH(who);
    const int64_t stride = gacc_stride(D, full != 0);
    const int gy = (int)(stride / 256 / 4) + 1;
    hipLaunchKernelGGL(gacc_reduce_kernel, dim3(I, gy), dim3(256), 0, st, (const double*)part, (const int*)istart, (const int*)pstart, (int)D,
                       (int)(full != 0), occ, mean_acc, second_acc);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
