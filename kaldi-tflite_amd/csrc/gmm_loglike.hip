// The log-likelihoods of all Gaussians of a diagonal GMM on the tile of gmm_loglike.h, written to a (F, I) matrix.
#include "gmm_loglike.h"

namespace {

__global__ void __launch_bounds__(IVP_GT) gdense_ll_kernel(const float* __restrict__ x, int64_t F, int D, int64_t ldx, const float* __restrict__ W,
                                                           const float* __restrict__ gconst, int I, float* __restrict__ ll) {
    extern __shared__ __attribute__((aligned(16))) float gd_lds[];
    float(*xs)[IVP_FT] = reinterpret_cast<float(*)[IVP_FT]>(gd_lds);
    const int tid = threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.x * IVP_FT;
    ivp_load_frames(xs, x, f0, F, D, ldx, tid);
    __syncthreads();
    for (int g = tid; g < I; g += IVP_GT) {
        float acc[IVP_FT];
        ivp_loglikes(acc, xs, W, gconst[g], I, g, 2 * D);
#pragma unroll
        for (int f = 0; f < IVP_FT; ++f)
            if (f0 + f < F) ll[(f0 + f) * I + g] = acc[f];
    }
}

}  // namespace

int gmm_dense_loglike(const char* who, const float* x, int64_t F, int D, int64_t ldx, const float* W, const float* gconst, int I, float* ll,
                      hipStream_t stream) {
    KTF_LDS_ONCE(ivp_tile_lds_bytes(KTF_IVECTOR_MAX_FEAT_DIM), gdense_ll_kernel);
    hipLaunchKernelGGL(gdense_ll_kernel, dim3((unsigned)((F + IVP_FT - 1) / IVP_FT)), dim3(IVP_GT), ivp_tile_lds_bytes(D), stream, x, F, D,
                       ldx, W, gconst, I, ll);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
