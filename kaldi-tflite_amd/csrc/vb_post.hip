// VB-HMM resegmentation (vb_common.h): the frame posteriors and their bucketing by Gaussian.
//
//   gdense_ll_kernel  (gmm_loglike.hip) the log-likelihoods of ALL Gaussians on the tile of gmm_loglike.h (the bits of
//   vb_select_kernel  ktf_ivector_post_f32), to the workspace (F, I); then one wave per frame: G = logsumexp over all I,
//                     p = exp(l - G) stat_scale, and the up to n candidates p >= sparsity_thr, largest first (n rounds of a wave
//                     arg-max after the last one taken).
#include "vb_common.h"
#include "gmm_bucket.h"
#include "gmm_loglike.h"

namespace {

constexpr int VSEL_WAVES = 4;

// one wave per frame; lane l owns the Gaussians l, l + 64, ... and overwrites their l with p (read back by the same lane only)
__global__ void __launch_bounds__(64 * VSEL_WAVES) vb_select_kernel(float* __restrict__ ll, int64_t F, int I, int n, float ll_scale,
                                                                    float stat_scale, float thr, int* __restrict__ gauss,
                                                                    float* __restrict__ post, float* __restrict__ loglike,
                                                                    int* __restrict__ truncated) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * VSEL_WAVES + (threadIdx.x >> 6);
    if (t >= F) return;
    float* lt = ll + t * I;
    float mx = -INFINITY;
    for (int g = lane; g < I; g += 64) mx = fmaxf(mx, lt[g] * ll_scale);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const bool any = mx > -INFINITY && mx < INFINITY;
    float s = 0.f;
    if (any)
        for (int g = lane; g < I; g += 64) s += expf(lt[g] * ll_scale - mx);
    const float G = any ? mx + logf(wave_sum(s)) : 0.f;
    int cnt = 0;
    for (int g = lane; g < I; g += 64) {
        const float p = any ? expf(lt[g] * ll_scale - G) * stat_scale : 0.f;
        lt[g] = p;
        cnt += (any && p >= thr) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    float lastp = INFINITY;
    int lastg = -1;
    bool open = any;
    for (int k = 0; k < n; ++k) {
        float bp = -1.f;
        int bg = 0x7fffffff;
        if (open) {
            for (int g = lane; g < I; g += 64) {
                const float p = lt[g];
                if (p >= thr && ranks_before(lastp, lastg, p, g) && ranks_before(p, g, bp, bg)) {
                    bp = p;
                    bg = g;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float op = __shfl_xor(bp, o, 64);
                const int og = __shfl_xor(bg, o, 64);
                if (ranks_before(op, og, bp, bg)) {
                    bp = op;
                    bg = og;
                }
            }
            open = bg != 0x7fffffff;
        }
        if (lane == 0) {
            gauss[t * n + k] = open ? bg : -1;
            post[t * n + k] = open ? bp : 0.f;
        }
        lastp = bp;
        lastg = bg;
    }
    if (lane == 0) {
        loglike[t] = G;
        if (cnt > n) atomicAdd(truncated, 1);                // an integer count: the order of the adds cannot change it
    }
}

}  // namespace

extern "C" int64_t ktf_vb_post_workspace_bytes(int64_t F, int32_t I) {
    const char* who = "ktf_vb_post_workspace_bytes";
    KTF_REQUIRE(F >= 0 && F < ((int64_t)1 << 31), "%s: frame count %lld out of range", who, (long long)F);
    KTF_REQUIRE(I >= 1 && I <= KTF_IVECTOR_MAX_GAUSS, "%s: %d Gaussians outside 1 .. %d", who, (int)I, KTF_IVECTOR_MAX_GAUSS);
    return al256((F > 0 ? F : 1) * I * 4);
}

extern "C" int ktf_vb_post_f32(const float* x, int64_t F, int32_t D, int64_t ldx, const float* W, const float* gconst, int32_t I, int32_t n,
                               float ll_scale, float stat_scale, float sparsity_thr, int32_t* gauss, float* post, float* loglike,
                               int32_t* truncated, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_vb_post_f32";
    const int64_t need = ktf_vb_post_workspace_bytes(F, I);
    if (need < 0) return (int)need;
    KTF_REQUIRE(D >= 1 && D <= KTF_IVECTOR_MAX_FEAT_DIM, "%s: feature dim %d outside 1 .. %d", who, (int)D, KTF_IVECTOR_MAX_FEAT_DIM);
    KTF_REQUIRE(ldx >= D, "%s: ldx %lld < D %d", who, (long long)ldx, (int)D);
    KTF_REQUIRE(n >= 1 && n <= KTF_IVECTOR_MAX_GSELECT, "%s: num_slots %d outside 1 .. %d", who, (int)n, KTF_IVECTOR_MAX_GSELECT);
    KTF_REQUIRE(ll_scale > 0.f && stat_scale > 0.f, "%s: ll_scale and stat_scale must be > 0", who);
    KTF_REQUIRE(sparsity_thr >= 0.f, "%s: sparsity_thr %g < 0", who, (double)sparsity_thr);
    KTF_REQUIRE(truncated && workspace, "%s: null argument", who);
    KTF_REQUIRE(F == 0 || (x && W && gconst && gauss && post && loglike), "%s: null argument", who);
    if (ktf_check_workspace(who, workspace, workspace_bytes, need) != KTF_OK) return KTF_EINVAL;
    if (F == 0) return KTF_OK;
    hipStream_t st = (hipStream_t)stream;
    float* ll = (float*)workspace;
    const int rc = gmm_dense_loglike(who, x, F, (int)D, ldx, W, gconst, (int)I, ll, st);
    if (rc != KTF_OK) return rc;
    hipLaunchKernelGGL(vb_select_kernel, dim3((unsigned)((F + VSEL_WAVES - 1) / VSEL_WAVES)), dim3(64 * VSEL_WAVES), 0, st, ll, F, (int)I, (int)n,
                       ll_scale, stat_scale, sparsity_thr, gauss, post, loglike, truncated);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int64_t ktf_vb_bucket_workspace_bytes(int64_t F, int32_t I, int32_t n) {
    const int rc = bucket_check_pairs("ktf_vb_bucket_workspace_bytes", F, I, n);
    if (rc != KTF_OK) return rc;
    return sec_layout(F > 0 ? F : 1, I, n, true).bytes;
}

extern "C" int ktf_vb_bucket(const int32_t* gauss, int64_t F, int32_t n, int32_t I, int32_t* start, int32_t* pairs, void* workspace,
                             size_t workspace_bytes, void* stream) {
    const char* who = "ktf_vb_bucket";
    const int64_t need = ktf_vb_bucket_workspace_bytes(F, I, n);
    if (need < 0) return (int)need;
    KTF_REQUIRE(start && workspace, "%s: null argument", who);
    KTF_REQUIRE(F == 0 || (gauss && pairs), "%s: null argument", who);
    if (ktf_check_workspace(who, workspace, workspace_bytes, need) != KTF_OK) return KTF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (F == 0) {
        KTF_CHECK_HIP(hipMemsetAsync(start, 0, (size_t)(I + 1) * 4, st), who, "hipMemsetAsync");
        return KTF_OK;
    }
    char* ws = (char*)workspace;
    const SecLayout l = sec_layout(F, I, n, true);
    const int rc = sec_bucket(who, gauss, F * n, (int)I, l, ws, st);
    if (rc != KTF_OK) return rc;
    KTF_CHECK_HIP(hipMemcpyAsync(start, ws + l.start, (size_t)(I + 1) * 4, hipMemcpyDeviceToDevice, st), who, "hipMemcpyAsync");
    KTF_CHECK_HIP(hipMemcpyAsync(pairs, ws + l.pairs, (size_t)(F * n) * 4, hipMemcpyDeviceToDevice, st), who, "hipMemcpyAsync");
    return KTF_OK;
}
