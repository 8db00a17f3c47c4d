// i-vector extraction: Kaldi's `gmm-global-get-post | scale-post | ivector-extract` (sid/extract_ivectors.sh), batched over the
// utterances of one call. Frames of all utterances lie end to end: utterance b owns rows [offsets[b], offsets[b + 1]).
//
//   ivpost_kernel     (a) per frame the n best log-likelihoods of a diagonal UBM, gconst + x.mi - x^2.iv / 2, as one fp32 GEMM of
//                     [x, x^2] (F x 2D) against W (2D x I) with the selection fused: the frames x I matrix never leaves LDS. 32
//                     frames per workgroup, one Gaussian per thread per 256-column tile; after each tile a wave merges its
//                     frames' columns into a sorted list (one list entry per lane) under the list's worst entry as threshold.
//   ivstats_kernel    (b) gamma_i = sum_t p_ti, F_i = sum_t p_ti x_t (fp64), posterior scale and max_count scale applied first.
//                     One workgroup per utterance; wave w owns the Gaussians g = w (mod 4) and each lane the columns d = lane
//                     (mod 64), so every (g, d) sum is taken by one lane in frame order: no atomics, no barriers.
//   ivgemm_kernel     (c) C = A . W in fp64, 64 x 64 tiles, K cut into chunks whose size depends on K alone (never on the batch),
//   ivreduce_kernel       the chunks' partial tiles summed in chunk order: linear = F . sigmaInvM, Q = gamma . U.
//   ivsolve_kernel    (d) per utterance: Q + I unpacked, blocked Cholesky (32-column panels, in the workspace), forward and back
//                     substitution of linear + priorOffset e0, ivector(0) -= priorOffset.
// Every stage is per utterance with a fixed reduction order, so an utterance's bits do not depend on its batch or position.
// (a) is in this file; (b) - (d) are compiled once in ivector_stages.hip, for the extractor training and the VB speaker update too.
#include "ivector_stages.h"
#include "gmm_loglike.h"

namespace {

inline size_t ivpost_lds_bytes(int D, int n) { return ivp_tile_lds_bytes(D) + (size_t)4 * (IVP_FT * (IVP_GT + 1) + 2 * IVP_FT * n + IVP_FT); }

__global__ void __launch_bounds__(IVP_GT) ivpost_kernel(const float* __restrict__ x, int64_t F, int D, int64_t ldx,
                                                         const float* __restrict__ W, const float* __restrict__ gconst, int I, int n,
                                                         int ns, float min_post, int* __restrict__ gauss, float* __restrict__ post) {
    // n = min(num_gselect, I) entries kept, ns = num_gselect slots written per frame. Dynamic LDS (ivpost_lds_bytes):
    extern __shared__ __attribute__((aligned(16))) float ivp_lds[];
    float(*xs)[IVP_FT] = reinterpret_cast<float(*)[IVP_FT]>(ivp_lds);                        // [x, x^2] transposed (2D rows):
    float(*ll)[IVP_GT + 1] = reinterpret_cast<float(*)[IVP_GT + 1]>(ivp_lds + 2 * D * IVP_FT); // a float4 is 4 frames of one k
    float* lval = ivp_lds + 2 * D * IVP_FT + IVP_FT * (IVP_GT + 1);                           // (IVP_FT, n) sorted lists
    int* lidx = reinterpret_cast<int*>(lval + IVP_FT * n);
    int* lcnt = lidx + IVP_FT * n;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t f0 = (int64_t)blockIdx.x * IVP_FT;
    const int K = 2 * D;
    ivp_load_frames(xs, x, f0, F, D, ldx, tid);
    if (tid < IVP_FT) lcnt[tid] = 0;
    __syncthreads();
    for (int g0 = 0; g0 < I; g0 += IVP_GT) {
        const int g = g0 + tid;
        if (g < I) {
            float acc[IVP_FT];
            ivp_loglikes(acc, xs, W, gconst[g], I, g, K);
#pragma unroll
            for (int f = 0; f < IVP_FT; ++f) ll[f][tid] = acc[f];
        }
        __syncthreads();
        // merge: wave wv owns frames wv, wv + 4, ...; lane j holds list entry j
        for (int f = wv; f < IVP_FT; f += IVP_GT / 64) {
            if (f0 + f >= F) break;
            float val = lane < lcnt[f] ? lval[f * n + lane] : 0.f;
            int idx = lane < lcnt[f] ? lidx[f * n + lane] : 0;
            int cnt = lcnt[f];
            for (int c = 0; c < IVP_GT; c += 64) {
                const int gg = g0 + c + lane;
                const float v = gg < I ? ll[f][c + lane] : 0.f;
                const float tv = __shfl(val, n - 1);
                const int ti = __shfl(idx, n - 1);
                unsigned long long m = __ballot(gg < I && (cnt < n || ranks_before(v, gg, tv, ti)));
                while (m) {
                    const int src = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const float cv = __shfl(v, src);
                    const int cg = g0 + c + src;
                    if (cnt == n && !ranks_before(cv, cg, __shfl(val, n - 1), __shfl(idx, n - 1))) continue;
                    const int pos = __popcll(__ballot(lane < cnt && ranks_before(val, idx, cv, cg)));
                    const float pv = __shfl(val, lane > 0 ? lane - 1 : 0);
                    const int pi = __shfl(idx, lane > 0 ? lane - 1 : 0);
                    if (lane == pos) {
                        val = cv;
                        idx = cg;
                    } else if (lane > pos) {
                        val = pv;
                        idx = pi;
                    }
                    cnt = cnt < n ? cnt + 1 : n;
                }
            }
            if (lane < n) {
                lval[f * n + lane] = val;
                lidx[f * n + lane] = idx;
            }
            if (lane == 0) lcnt[f] = cnt;
        }
        __syncthreads();
    }
    // posteriors: exp(l - max) over the kept set, the smallest dropped while below min_post of the running sum, renormalised
    for (int f = wv; f < IVP_FT; f += IVP_GT / 64) {
        const int64_t t = f0 + f;
        if (t >= F) break;
        const int cnt = lcnt[f];
        const float mx = lval[f * n];
        const float e = lane < cnt ? expf(lval[f * n + lane] - mx) : 0.f;
        int keep = cnt;
        float sum = 0.f;
        for (int j = 0; j < cnt; ++j) sum += __shfl(e, j);
        while (keep > 1) {
            const float last = __shfl(e, keep - 1);
            if (!(last < min_post * sum)) break;
            sum -= last;
            --keep;
        }
        if (lane < ns) {
            gauss[t * ns + lane] = lane < keep ? lidx[f * n + lane] : -1;
            post[t * ns + lane] = lane < keep ? e / sum : 0.f;
        }
    }
}

}  // namespace

extern "C" int ktf_ivector_post_f32(const float* x, int64_t F, int32_t D, int64_t ldx, const float* W, const float* gconst, int32_t I,
                                    int32_t n, float min_post, int32_t* gauss, float* post, void* stream) {
    const char* who = "ktf_ivector_post_f32";
    KTF_REQUIRE(F >= 0 && F <= ((int64_t)1 << 40), "%s: frame count %lld out of range", who, (long long)F);
    KTF_REQUIRE(D >= 1 && D <= KTF_IVECTOR_MAX_FEAT_DIM, "%s: feature dim %d outside 1 .. %d", who, (int)D, KTF_IVECTOR_MAX_FEAT_DIM);
    KTF_REQUIRE(ldx >= D, "%s: ldx %lld < D %d", who, (long long)ldx, (int)D);
    KTF_REQUIRE(I >= 1 && I <= KTF_IVECTOR_MAX_GAUSS, "%s: %d Gaussians outside 1 .. %d", who, (int)I, KTF_IVECTOR_MAX_GAUSS);
    KTF_REQUIRE(n >= 1 && n <= KTF_IVECTOR_MAX_GSELECT, "%s: num_gselect %d outside 1 .. %d", who, (int)n, KTF_IVECTOR_MAX_GSELECT);
    KTF_REQUIRE(min_post >= 0.f && min_post < 1.f, "%s: min_post %g outside [0, 1)", who, (double)min_post);
    if (F == 0) return KTF_OK;
    KTF_REQUIRE(x && W && gconst && gauss && post, "%s: null argument", who);
    const int keep = n < I ? n : I;
    const size_t lds = ivpost_lds_bytes(D, keep);
    KTF_LDS_ONCE(ivpost_lds_bytes(KTF_IVECTOR_MAX_FEAT_DIM, KTF_IVECTOR_MAX_GSELECT), ivpost_kernel);
    hipLaunchKernelGGL(ivpost_kernel, dim3((unsigned)((F + IVP_FT - 1) / IVP_FT)), dim3(IVP_GT), lds, (hipStream_t)stream, x, F, (int)D, ldx,
                       W, gconst, (int)I, keep, (int)n, min_post, gauss, post);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int64_t ktf_ivector_workspace_bytes(int32_t B, int32_t I, int32_t D, int32_t S) {
    const char* who = "ktf_ivector_workspace_bytes";
    KTF_REQUIRE(B >= 1 && B <= 65535, "%s: batch %d outside 1 .. 65535", who, (int)B);
    KTF_REQUIRE(I >= 1 && I <= KTF_IVECTOR_MAX_GAUSS, "%s: %d Gaussians outside 1 .. %d", who, (int)I, KTF_IVECTOR_MAX_GAUSS);
    KTF_REQUIRE(D >= 1 && D <= KTF_IVECTOR_MAX_FEAT_DIM, "%s: feature dim %d outside 1 .. %d", who, (int)D, KTF_IVECTOR_MAX_FEAT_DIM);
    KTF_REQUIRE(S >= 1 && S <= KTF_IVECTOR_MAX_DIM, "%s: i-vector dim %d outside 1 .. %d", who, (int)S, KTF_IVECTOR_MAX_DIM);
    return iv_layout(B, I, D, S).total;
}

extern "C" int ktf_ivector_extract(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* offsets, int32_t B, const int32_t* gauss,
                                   const float* post, int32_t n, float posterior_scale, float acoustic_weight, float max_count,
                                   const double* sigma_inv_M, const double* U, int32_t I, int32_t S, double prior_offset, void* ivectors,
                                   int32_t out_dtype_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_ivector_extract";
    const int64_t need = ktf_ivector_workspace_bytes(B, I, D, S);
    if (need < 0) return (int)need;
    KTF_REQUIRE(F >= 0 && F < ((int64_t)1 << 31), "%s: frame count %lld out of range", who, (long long)F);
    KTF_REQUIRE(ldx >= D, "%s: ldx %lld < D %d", who, (long long)ldx, (int)D);
    KTF_REQUIRE(n >= 1 && n <= KTF_IVECTOR_MAX_GSELECT, "%s: %d slots per frame outside 1 .. %d", who, (int)n, KTF_IVECTOR_MAX_GSELECT);
    KTF_REQUIRE(posterior_scale >= 0.f && acoustic_weight >= 0.f && max_count >= 0.f,
                "%s: posterior_scale, acoustic_weight and max_count must be >= 0", who);
    KTF_REQUIRE(out_dtype_bytes == 4 || out_dtype_bytes == 8, "%s: out_dtype_bytes %d, need 4 or 8", who, (int)out_dtype_bytes);
    KTF_REQUIRE(offsets && sigma_inv_M && U && ivectors && workspace, "%s: null argument", who);
    KTF_REQUIRE(F == 0 || (x && gauss && post), "%s: null frames / posteriors", who);
    if (ktf_check_workspace(who, workspace, workspace_bytes, need) != KTF_OK) return KTF_EINVAL;
    return iv_run_stages(who, x, F, (int)D, ldx, offsets, (int)B, gauss, post, (int)n, posterior_scale, acoustic_weight, max_count,
                         sigma_inv_M, U, (int)I, (int)S, prior_offset, ivectors, (int)out_dtype_bytes, (char*)workspace, (hipStream_t)stream);
}
