// Stages (b) - (d) of i-vector extraction (see ivector.hip) and the per-utterance posterior covariance of its statistics, compiled
// once in ivector_stages.hip: shared by the extraction (ivector.hip), the extractor-training statistics (ivector_train.hip) and the
// speaker update of VB resegmentation (vb_speaker.hip). Here: the workspace layout, the device helpers the clients' own kernels use
// and the host functions that launch the stages.
#pragma once
#include "common.h"

constexpr int64_t GKC = 2048;       // GEMM K chunk: a function of K alone
constexpr int COV_THREADS = 256;

// frames [t0, t1) of utterance b, clamped to the F rows the caller declared (an inconsistent table reads nothing out of range)
__device__ __forceinline__ void utt_rows(const int* off, int b, int64_t F, int64_t* t0, int64_t* t1) {
    int64_t a = off[b], e = off[b + 1];
    a = a < 0 ? 0 : (a > F ? F : a);
    e = e < a ? a : (e > F ? F : e);
    *t0 = a;
    *t1 = e;
}

// fixed tree over the workgroup's 256 partial sums
__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int s = COV_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

struct IvLayout {
    int64_t F, gamma, lpart, lin, qpart, q, L, total;
    int nkl, nkq;
};

inline IvLayout iv_layout(int64_t B, int64_t I, int64_t D, int64_t S) {
    IvLayout l;
    const int64_t P = S * (S + 1) / 2;
    l.nkl = (int)((I * D + GKC - 1) / GKC);
    l.nkq = (int)((I + GKC - 1) / GKC);
    int64_t at = 0;
    l.F = at;     at += al256(B * I * D * 8);
    l.gamma = at; at += al256(B * I * 8);
    l.lpart = at; at += al256(l.nkl * B * S * 8);
    l.lin = at;   at += al256(B * S * 8);
    l.qpart = at; at += al256(l.nkq * B * P * 8);
    l.q = at;     at += al256(B * P * 8);
    l.L = at;     at += al256(B * S * S * 8);
    l.total = at;
    return l;
}

// out (M x N) = A (M x K, lda) . W (K x N, ldw) in fp64: nk = ceil(K / GKC) chunks, their partial tiles (`part`, unused for nk = 1)
// summed in chunk order
int iv_gemm(const char* who, const double* A, int64_t lda, const double* W, int64_t ldw, double* part, double* out, int nk, int64_t M,
            int64_t N, int64_t K, hipStream_t st);

// Stages (b) - (d) for one chunk of B utterances in the workspace `ws` (iv_layout): statistics, linear and quadratic terms, the
// Cholesky factor (left in l.L) and the solve written to `ivectors` (fp32 or fp64). Arguments are checked by the caller.
int iv_run_stages(const char* who, const float* x, int64_t F, int D, int64_t ldx, const int32_t* offsets, int B, const int32_t* gauss,
                  const float* post, int n, float posterior_scale, float acoustic_weight, float max_count, const double* sigma_inv_M,
                  const double* U, int I, int S, double prior_offset, void* ivectors, int out_dtype_bytes, char* ws, hipStream_t st);

// (d) alone, one workgroup per utterance: Q (B, P) packed lower triangle, lin (B, S) -> the Cholesky factor of Q + I in L (B, S, S) and
// the solve in out (B, S), fp32 or fp64. An utterance b with off[b] == off[b + 1] (clamped to F) gets the zero vector.
int iv_solve(const char* who, const double* Q, const double* lin, const int* off, int B, int64_t F, int S, double prior_offset, double* L,
             void* out, int out_dtype_bytes, hipStream_t st);

// L (B, S, S): on entry the Cholesky factor left by iv_solve, on exit its inverse (lower triangle). scat (B, P) = the posterior
// covariance plus w w^T, wv (B, S) = the posterior mean w, tail (B, 2) = (1 if the utterance has frames, the marginal-likelihood scalar).
int iv_cov(const char* who, const double* lin, const int* off, int B, int64_t F, int S, double prior_offset, double* L, double* scat,
           double* wv, double* tail, hipStream_t st);
