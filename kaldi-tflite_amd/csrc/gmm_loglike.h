// The diagonal-GMM log-likelihood tile shared by the fused selection of ktf_ivector_post_f32 (ivector.hip) and the dense kernel of
// gmm_loglike.hip (ktf_gmm_post_dense_f32 in gmm_train.hip, ktf_vb_post_f32 in vb_post.hip): IVP_FT frames per workgroup as [x, x^2]
// transposed in LDS, one Gaussian per thread, l = gconst + sum_k [x, x^2]_k W_kg with one fmaf per term in ascending k. Both
// kernels therefore give the same bits for the same frame and Gaussian.
#pragma once
#include "common.h"

namespace {

constexpr int IVP_FT = 32;          // frames per workgroup of the posterior kernels
constexpr int IVP_GT = 256;         // Gaussians per tile (= threads)

// LDS bytes of the tile's frames: 2D rows of IVP_FT floats
inline size_t ivp_tile_lds_bytes(int D) { return (size_t)4 * 2 * D * IVP_FT; }

// (v, g) ranks before (w, h): the larger value first, the lower index on ties
__device__ __forceinline__ bool ranks_before(float v, int g, float w, int h) { return v > w || (v == w && g < h); }

// xs (2D rows of IVP_FT): [x, x^2] of frames f0 .. f0 + IVP_FT - 1 transposed (a float4 is 4 frames of one k); zeros beyond F
__device__ __forceinline__ void ivp_load_frames(float (*xs)[IVP_FT], const float* __restrict__ x, int64_t f0, int64_t F, int D, int64_t ldx,
                                                int tid) {
    for (int e = tid; e < IVP_FT * D; e += IVP_GT) {
        const int f = e / D, d = e - f * D;
        const float v = f0 + f < F ? x[(f0 + f) * ldx + d] : 0.f;
        xs[d][f] = v;
        xs[D + d][f] = v * v;
    }
}

// acc[f] = the log-likelihood of Gaussian g (< I) on the tile's frame f; W (K = 2D, I) row-major
__device__ __forceinline__ void ivp_loglikes(float (&acc)[IVP_FT], const float (*xs)[IVP_FT], const float* __restrict__ W, float gc, int I,
                                             int g, int K) {
#pragma unroll
    for (int f = 0; f < IVP_FT; ++f) acc[f] = gc;
    for (int k = 0; k < K; ++k) {
        const float w = W[(int64_t)k * I + g];
        const float4* xr = reinterpret_cast<const float4*>(&xs[k][0]);
#pragma unroll
        for (int q = 0; q < IVP_FT / 4; ++q) {
            const float4 v = xr[q];
            acc[4 * q + 0] = fmaf(v.x, w, acc[4 * q + 0]);
            acc[4 * q + 1] = fmaf(v.y, w, acc[4 * q + 1]);
            acc[4 * q + 2] = fmaf(v.z, w, acc[4 * q + 2]);
            acc[4 * q + 3] = fmaf(v.w, w, acc[4 * q + 3]);
        }
    }
}

}  // namespace

// ll (F, I) = the log-likelihoods of ALL I Gaussians on the F frames of x (F >= 1): one launch, IVP_FT frames per workgroup
int gmm_dense_loglike(const char* who, const float* x, int64_t F, int D, int64_t ldx, const float* W, const float* gconst, int I, float* ll,
                      hipStream_t stream);
