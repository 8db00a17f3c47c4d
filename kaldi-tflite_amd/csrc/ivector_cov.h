// The per-utterance posterior covariance of the i-vector statistics (ivcov_kernel), shared by the extractor-training statistics of
// ivector_train.hip and the speaker update of vb_reseg.hip. Every translation unit that includes this gets its own copy.
#pragma once
#include "ivector_stages.h"

namespace {

constexpr int COV_THREADS = 256;

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

// Lws (B, S, S): on entry the Cholesky factor (lower triangle, the rest undefined), on exit its inverse X (lower triangle).
// scat (B, P), wv (B, S), tail (B, 2) = (1 if the utterance has frames, the marginal-likelihood scalar).
__global__ void __launch_bounds__(COV_THREADS) ivcov_kernel(const double* __restrict__ lin, const int* __restrict__ off, int64_t F, int S,
                                                             double prior_offset, double* __restrict__ Lws, double* __restrict__ scat,
                                                             double* __restrict__ wv, double* __restrict__ tail) {
    __shared__ double Dinv[NB][NB + 1];
    __shared__ double Ta[NB][NB + 1];
    __shared__ double Tb[NB][NB + 1];
    __shared__ double y[1024];
    __shared__ double z[1024];
    __shared__ double red[COV_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t P = (int64_t)S * (S + 1) / 2;
    double* sc = scat + (int64_t)b * P;
    int64_t t0, t1;
    utt_rows(off, b, F, &t0, &t1);
    if (t1 == t0) {                              // no frames: contributes nothing and is not counted
        for (int64_t e = tid; e < P; e += COV_THREADS) sc[e] = 0.0;
        for (int i = tid; i < S; i += COV_THREADS) wv[(int64_t)b * S + i] = 0.0;
        if (tid == 0) tail[2 * b] = tail[2 * b + 1] = 0.0;
        return;
    }
    double* L = Lws + (int64_t)b * S * S;
    double ld = 0.0;
    for (int j = tid; j < S; j += COV_THREADS) ld += log(L[(int64_t)j * S + j]);
    for (int i = tid; i < S; i += COV_THREADS) y[i] = lin[(int64_t)b * S + i] + (i == 0 ? prior_offset : 0.0);
    const double logdet = block_sum(ld, red, tid);
    const int nt = (S + NB - 1) / NB;
    // X = L^-1 in place, block row by block row: X_ii = L_ii^-1, X_ij = -X_ii sum_{j <= k < i} L_ik X_kj (column blocks ascending:
    // block (i, j) of L is last read by column block j)
    for (int bi = 0; bi < nt; ++bi) {
        const int i0 = bi * NB, nb = S - i0 < NB ? S - i0 : NB;
        for (int e = tid; e < NB * NB; e += COV_THREADS) {
            const int r = e / NB, c = e - r * NB;
            Ta[r][c] = (r < nb && c <= r) ? L[(int64_t)(i0 + r) * S + i0 + c] : (r == c ? 1.0 : 0.0);   // identity past nb
        }
        __syncthreads();
        if (tid < NB) {                          // column tid of the diagonal block's inverse by forward substitution
            const int c = tid;
            for (int r = 0; r < NB; ++r) {
                double v = 0.0;
                if (r >= c) {
                    double s = r == c ? 1.0 : 0.0;
                    for (int k = c; k < r; ++k) s = fma(-Ta[r][k], Dinv[k][c], s);
                    v = s / Ta[r][r];
                }
                Dinv[r][c] = v;
            }
        }
        __syncthreads();
        for (int bj = 0; bj < bi; ++bj) {
            const int j0 = bj * NB;
            double acc[NB * NB / COV_THREADS] = {};
            for (int bk = bj; bk < bi; ++bk) {
                const int k0 = bk * NB;
                for (int e = tid; e < NB * NB; e += COV_THREADS) {
                    const int r = e / NB, c = e - r * NB;
                    Ta[r][c] = r < nb ? L[(int64_t)(i0 + r) * S + k0 + c] : 0.0;
                    Tb[r][c] = (bk > bj || c <= r) ? L[(int64_t)(k0 + r) * S + j0 + c] : 0.0;             // X_kj, lower on its diagonal
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < NB * NB / COV_THREADS; ++q) {
                    const int e = tid + COV_THREADS * q, r = e / NB, c = e - r * NB;
                    double s = acc[q];
#pragma unroll
                    for (int k = 0; k < NB; ++k) s = fma(Ta[r][k], Tb[k][c], s);
                    acc[q] = s;
                }
                __syncthreads();
            }
#pragma unroll
            for (int q = 0; q < NB * NB / COV_THREADS; ++q) {
                const int e = tid + COV_THREADS * q, r = e / NB, c = e - r * NB;
                Ta[r][c] = acc[q];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < NB * NB / COV_THREADS; ++q) {
                const int e = tid + COV_THREADS * q, r = e / NB, c = e - r * NB;
                double s = 0.0;
                for (int k = 0; k <= r; ++k) s = fma(Dinv[r][k], Ta[k][c], s);
                if (r < nb) L[(int64_t)(i0 + r) * S + j0 + c] = -s;
            }
            __syncthreads();
        }
        for (int e = tid; e < NB * NB; e += COV_THREADS) {
            const int r = e / NB, c = e - r * NB;
            if (r < nb && c <= r) L[(int64_t)(i0 + r) * S + i0 + c] = Dinv[r][c];
        }
        __syncthreads();
    }
    // z = X lin' (a wave per row), w = X^T z (a thread per column, rows ascending)
    for (int i = wave; i < S; i += COV_THREADS / 64) {
        double s = 0.0;
        for (int k = lane; k <= i; k += 64) s = fma(L[(int64_t)i * S + k], y[k], s);
        s = wave_sum_d(s);
        if (lane == 0) z[i] = s;
    }
    __syncthreads();
    double qd = 0.0;
    for (int j = tid; j < S; j += COV_THREADS) {
        double s = 0.0;
        for (int k = j; k < S; ++k) s = fma(L[(int64_t)k * S + j], z[k], s);
        y[j] = s;
        wv[(int64_t)b * S + j] = s;
        qd = fma(z[j], z[j], qd);
    }
    const double quad = block_sum(qd, red, tid);             // (its barriers also publish y)
    if (tid == 0) {
        tail[2 * b] = 1.0;
        tail[2 * b + 1] = 0.5 * quad - logdet - 0.5 * prior_offset * prior_offset;
    }
    // W = X^T X + w w^T, lower tiles: C_ij = sum_{k >= i} X_ki X_kj
    for (int ti = 0; ti < nt; ++ti)
        for (int tj = 0; tj <= ti; ++tj) {
            const int i0 = ti * NB, j0 = tj * NB;
            double acc[NB * NB / COV_THREADS] = {};
            for (int bk = ti; bk < nt; ++bk) {
                const int k0 = bk * NB;
                for (int e = tid; e < NB * NB; e += COV_THREADS) {
                    const int k = e / NB, c = e - k * NB;
                    const bool row = k0 + k < S;
                    Ta[k][c] = (row && i0 + c <= k0 + k) ? L[(int64_t)(k0 + k) * S + i0 + c] : 0.0;
                    Tb[k][c] = (row && j0 + c <= k0 + k) ? L[(int64_t)(k0 + k) * S + j0 + c] : 0.0;
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < NB * NB / COV_THREADS; ++q) {
                    const int e = tid + COV_THREADS * q, r = e / NB, c = e - r * NB;
                    double s = acc[q];
#pragma unroll
                    for (int k = 0; k < NB; ++k) s = fma(Ta[k][r], Tb[k][c], s);
                    acc[q] = s;
                }
                __syncthreads();
            }
#pragma unroll
            for (int q = 0; q < NB * NB / COV_THREADS; ++q) {
                const int e = tid + COV_THREADS * q, r = e / NB, c = e - r * NB;
                const int i = i0 + r, j = j0 + c;
                if (i < S && j <= i) sc[(int64_t)i * (i + 1) / 2 + j] = acc[q] + y[i] * y[j];
            }
        }
}

}  // namespace
