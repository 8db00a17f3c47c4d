// The kernels of stages (b) - (d) of i-vector extraction and of the posterior covariance, and the host sequences that launch them
// (ivector_stages.h; the stages are described at the top of ivector.hip, ivcov_kernel at the top of ivector_train.hip).
#include "ivector_stages.h"

namespace {

constexpr int IVS_WAVES = 4;        // stats kernel: Gaussian owners per utterance
constexpr int IVS_BATCH = 8;        // owned slots whose loads are in flight together
constexpr int GT = 64;              // GEMM tile (rows and columns)
constexpr int GK = 16;              // GEMM K step
constexpr int NB = 32;              // Cholesky panel width
constexpr int SOLVE_THREADS = 256;

// (b): gamma (B, I) and Fst (B, I, D) are zero on entry. Slots with an index outside [0, I) are skipped.
__global__ void __launch_bounds__(64 * IVS_WAVES) ivstats_kernel(const float* __restrict__ x, int64_t F, int D, int64_t ldx, const int* __restrict__ off,
                                                                  const int* __restrict__ gauss, const float* __restrict__ post, int n, int I,
                                                                  float post_scale, float acoustic_weight, float max_count,
                                                                  double* __restrict__ gamma, double* __restrict__ Fst) {
    __shared__ double part[64 * IVS_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t t0, t1;
    utt_rows(off, b, F, &t0, &t1);
    // total posterior after scale-post (fp64, a fixed order: thread-strided, then a fixed tree)
    double tot = 0.0;
    for (int64_t e = t0 * n + tid; e < t1 * n; e += 64 * IVS_WAVES)
        if (gauss[e] >= 0 && gauss[e] < I) tot += (double)(post[e] * post_scale);
    part[tid] = tot;
    __syncthreads();
    for (int s = 64 * IVS_WAVES / 2; s > 0; s >>= 1) {
        if (tid < s) part[tid] += part[tid + s];
        __syncthreads();
    }
    // ivector-extract: ScalePosterior(acoustic_weight * max_count_scale), the scale rounded to BaseFloat
    const double this_t = (double)acoustic_weight * part[0];
    const double mcs = (max_count > 0.f && this_t > (double)max_count) ? (double)max_count / this_t : 1.0;
    const float scale = (float)((double)acoustic_weight * mcs);
    double* gm = gamma + (int64_t)b * I;
    double* Fb = Fst + (int64_t)b * I * D;
    const int ncol = D + 1;                                  // column D is gamma
    for (int64_t t = t0; t < t1; ++t) {
        int gs = -1;
        float ws = 0.f;
        if (lane < n) {
            gs = gauss[t * n + lane];
            ws = (post[t * n + lane] * post_scale) * scale;
        }
        double xv[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int c = lane + 64 * r;
            xv[r] = c < D ? (double)x[t * ldx + c] : 1.0;
        }
        unsigned long long m = __ballot(lane < n && gs >= 0 && gs < I && gs % IVS_WAVES == wv);
        while (m) {
            int gb[IVS_BATCH];
            double wb[IVS_BATCH];
            int nb = 0;
#pragma unroll
            for (int r = 0; r < IVS_BATCH; ++r) {
                gb[r] = -1;
                wb[r] = 0.0;
            }
            // a run of distinct Gaussians in slot order (a repeated one waits for the next run: frame order per Gaussian)
#pragma unroll
            for (int r = 0; r < IVS_BATCH; ++r) {
                if (m && nb == r) {
                    const int s = __ffsll((long long)m) - 1;
                    const int g = __shfl(gs, s);
                    bool dup = false;
#pragma unroll
                    for (int q = 0; q < r; ++q) dup |= gb[q] == g;
                    if (!dup) {
                        gb[r] = g;
                        wb[r] = (double)__shfl(ws, s);
                        m &= m - 1;
                        ++nb;
                    }
                }
            }
            double v[IVS_BATCH][3];
#pragma unroll
            for (int r = 0; r < IVS_BATCH; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int c = lane + 64 * q;
                    v[r][q] = 0.0;
                    if (r < nb && c < ncol) v[r][q] = c < D ? Fb[(int64_t)gb[r] * D + c] : gm[gb[r]];
                }
#pragma unroll
            for (int r = 0; r < IVS_BATCH; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int c = lane + 64 * q;
                    if (r < nb && c < ncol) {
                        const double nv = v[r][q] + wb[r] * xv[q];
                        if (c < D) Fb[(int64_t)gb[r] * D + c] = nv;
                        else gm[gb[r]] = nv;
                    }
                }
        }
    }
}

// (c): part[kc] (M x N, ldc) = A[:, kc*GKC .. ) . W[kc*GKC .. , :]; A (M x K, lda), W (K x N, ldw), all fp64 row-major.
__global__ void __launch_bounds__(256) ivgemm_kernel(const double* __restrict__ A, int64_t lda, const double* __restrict__ W, int64_t ldw,
                                                      double* __restrict__ part, int64_t ldc, int64_t M, int64_t N, int64_t K) {
    __shared__ double As[GK][GT + 1];
    __shared__ double Ws[GK][GT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * GT, n0 = (int64_t)blockIdx.y * GT, kc = blockIdx.z;
    const int64_t k0 = kc * GKC, k1 = k0 + GKC < K ? k0 + GKC : K;
    double acc[4][4] = {};
    for (int64_t kk = k0; kk < k1; kk += GK) {
        for (int e = tid; e < GK * GT; e += 256) {
            const int r = e / GK, k = e - r * GK;            // A: row r, k (k fastest: contiguous along K)
            const int64_t gm = m0 + r, gk = kk + k;
            As[k][r] = (gm < M && gk < k1) ? A[gm * lda + gk] : 0.0;
            const int k2 = e / GT, c = e - k2 * GT;          // W: k2, column c (c fastest)
            const int64_t gk2 = kk + k2, gn = n0 + c;
            Ws[k2][c] = (gk2 < k1 && gn < N) ? W[gk2 * ldw + gn] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < GK; ++k) {
            double a[4], w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[k][ty + 16 * i];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = Ws[k][tx + 16 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], w[j], acc[i][j]);
        }
        __syncthreads();
    }
    double* P = part + kc * M * ldc;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t gm = m0 + ty + 16 * i, gn = n0 + tx + 16 * j;
            if (gm < M && gn < N) P[gm * ldc + gn] = acc[i][j];
        }
}

__global__ void ivreduce_kernel(const double* __restrict__ part, int nk, int64_t total, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    double s = part[e];
    for (int k = 1; k < nk; ++k) s += part[(int64_t)k * total + e];
    out[e] = s;
}

// (d): one workgroup per utterance. Qp (B, P) packed lower triangle, lin (B, S); L (B, S, S) workspace (row-major, lower used).
template <typename T>
__global__ void __launch_bounds__(SOLVE_THREADS) ivsolve_kernel(const double* __restrict__ Qp, const double* __restrict__ lin,
                                                                 const int* __restrict__ off, int64_t F, int S, double prior_offset,
                                                                 double* __restrict__ Lws, T* __restrict__ out) {
    __shared__ double Ld[NB][NB + 1];
    __shared__ double Pi[NB][NB + 1];
    __shared__ double Pj[NB][NB + 1];
    __shared__ double y[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    T* o = out + (int64_t)b * S;
    int64_t t0, t1;
    utt_rows(off, b, F, &t0, &t1);
    if (t1 == t0) {                              // no frames: the zero vector
        for (int i = tid; i < S; i += SOLVE_THREADS) o[i] = (T)0;
        return;
    }
    const int64_t P = (int64_t)S * (S + 1) / 2;
    const double* q = Qp + (int64_t)b * P;
    double* L = Lws + (int64_t)b * S * S;
    for (int64_t e = tid; e < P; e += SOLVE_THREADS) {
        const int i = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
        int r = i;
        if ((int64_t)r * (r + 1) / 2 > e) --r;
        if ((int64_t)(r + 1) * (r + 2) / 2 <= e) ++r;
        const int c = (int)(e - (int64_t)r * (r + 1) / 2);
        L[(int64_t)r * S + c] = q[e] + (r == c ? 1.0 : 0.0);
    }
    for (int i = tid; i < S; i += SOLVE_THREADS) y[i] = lin[(int64_t)b * S + i] + (i == 0 ? prior_offset : 0.0);
    __syncthreads();
    for (int kb = 0; kb < S; kb += NB) {
        const int nb = S - kb < NB ? S - kb : NB;
        for (int e = tid; e < NB * NB; e += SOLVE_THREADS) {
            const int i = e / NB, j = e - i * NB;
            Ld[i][j] = (i < nb && j <= i) ? L[(int64_t)(kb + i) * S + kb + j] : (i == j ? 1.0 : 0.0);   // identity past nb
        }
        __syncthreads();
        for (int j = 0; j < nb; ++j) {
            if (tid == 0) Ld[j][j] = sqrt(Ld[j][j]);
            __syncthreads();
            if (tid > j && tid < nb) Ld[tid][j] /= Ld[j][j];
            __syncthreads();
            for (int e = tid; e < NB * NB; e += SOLVE_THREADS) {
                const int i = e / NB, k = e - i * NB;
                if (i > j && i < nb && k > j && k <= i) Ld[i][k] -= Ld[i][j] * Ld[k][j];
            }
            __syncthreads();
        }
        for (int e = tid; e < NB * NB; e += SOLVE_THREADS) {
            const int i = e / NB, j = e - i * NB;
            if (i < nb && j <= i) L[(int64_t)(kb + i) * S + kb + j] = Ld[i][j];
        }
        // panel: rows below the block, L21 = A21 L11^-T (one row per thread)
        const int r0 = kb + nb;
        for (int i = r0 + tid; i < S; i += SOLVE_THREADS) {
            double* row = L + (int64_t)i * S + kb;         // the thread's own row: its writes are its own later reads
            for (int j = 0; j < nb; ++j) {
                double v = row[j];
                for (int k = 0; k < j; ++k) v = fma(-row[k], Ld[j][k], v);
                row[j] = v / Ld[j][j];
            }
        }
        __syncthreads();
        // trailing update: A22 -= L21 L21^T on the lower tiles
        const int nt = (S - r0 + NB - 1) / NB;
        for (int ti = 0; ti < nt; ++ti)
            for (int tj = 0; tj <= ti; ++tj) {
                const int i0 = r0 + ti * NB, j0 = r0 + tj * NB;
                for (int e = tid; e < NB * NB; e += SOLVE_THREADS) {
                    const int r = e / NB, k = e - r * NB;
                    Pi[r][k] = (i0 + r < S && k < nb) ? L[(int64_t)(i0 + r) * S + kb + k] : 0.0;
                    Pj[r][k] = (j0 + r < S && k < nb) ? L[(int64_t)(j0 + r) * S + kb + k] : 0.0;
                }
                __syncthreads();
                for (int e = tid; e < NB * NB; e += SOLVE_THREADS) {
                    const int r = e / NB, c = e - r * NB;
                    if (i0 + r < S && j0 + c < S && j0 + c <= i0 + r) {
                        double s = 0.0;
#pragma unroll
                        for (int k = 0; k < NB; ++k) s = fma(Pi[r][k], Pj[c][k], s);
                        L[(int64_t)(i0 + r) * S + j0 + c] -= s;
                    }
                }
                __syncthreads();
            }
    }
    // L z = y, then L^T w = z (in place in y)
    for (int j = 0; j < S; ++j) {
        const double zj = y[j] / L[(int64_t)j * S + j];
        __syncthreads();
        if (tid == 0) y[j] = zj;
        for (int i = j + 1 + tid; i < S; i += SOLVE_THREADS) y[i] -= L[(int64_t)i * S + j] * zj;
        __syncthreads();
    }
    for (int j = S - 1; j >= 0; --j) {
        const double wj = y[j] / L[(int64_t)j * S + j];
        __syncthreads();
        if (tid == 0) y[j] = wj;
        for (int i = tid; i < j; i += SOLVE_THREADS) y[i] -= L[(int64_t)j * S + i] * wj;
        __syncthreads();
    }
    for (int i = tid; i < S; i += SOLVE_THREADS) o[i] = (T)(i == 0 ? y[i] - prior_offset : y[i]);
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

int iv_gemm(const char* who, const double* A, int64_t lda, const double* W, int64_t ldw, double* part, double* out, int nk, int64_t M,
            int64_t N, int64_t K, hipStream_t st) {
    double* dst = nk == 1 ? out : part;
    hipLaunchKernelGGL(ivgemm_kernel, dim3(ktf_cdiv(M, GT), ktf_cdiv(N, GT), nk), dim3(256), 0, st, A, lda, W, ldw, dst, N, M, N, K);
    KTF_CHECK_LAUNCH(who);
    if (nk > 1) {
        const int64_t total = M * N;
        hipLaunchKernelGGL(ivreduce_kernel, dim3(ktf_cdiv(total, 256)), dim3(256), 0, st, (const double*)part, nk, total, out);
        KTF_CHECK_LAUNCH(who);
    }
    return KTF_OK;
}

int iv_solve(const char* who, const double* Q, const double* lin, const int* off, int B, int64_t F, int S, double prior_offset, double* L,
             void* out, int out_dtype_bytes, hipStream_t st) {
    if (out_dtype_bytes == 8)
        hipLaunchKernelGGL(ivsolve_kernel<double>, dim3(B), dim3(SOLVE_THREADS), 0, st, Q, lin, off, F, S, prior_offset, L, (double*)out);
    else
        hipLaunchKernelGGL(ivsolve_kernel<float>, dim3(B), dim3(SOLVE_THREADS), 0, st, Q, lin, off, F, S, prior_offset, L, (float*)out);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

int iv_cov(const char* who, const double* lin, const int* off, int B, int64_t F, int S, double prior_offset, double* L, double* scat,
           double* wv, double* tail, hipStream_t st) {
    hipLaunchKernelGGL(ivcov_kernel, dim3(B), dim3(COV_THREADS), 0, st, lin, off, F, S, prior_offset, L, scat, wv, tail);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

int iv_run_stages(const char* who, const float* x, int64_t F, int D, int64_t ldx, const int32_t* offsets, int B, const int32_t* gauss,
                  const float* post, int n, float posterior_scale, float acoustic_weight, float max_count, const double* sigma_inv_M,
                  const double* U, int I, int S, double prior_offset, void* ivectors, int out_dtype_bytes, char* ws, hipStream_t st) {
    const IvLayout l = iv_layout(B, I, D, S);
    double* Fst = (double*)(ws + l.F);
    double* gam = (double*)(ws + l.gamma);
    double* lin = (double*)(ws + l.lin);
    double* q = (double*)(ws + l.q);
    KTF_CHECK_HIP(hipMemsetAsync(ws, 0, (size_t)l.lpart, st), who, "hipMemsetAsync");   // F and gamma
    hipLaunchKernelGGL(ivstats_kernel, dim3(B), dim3(64 * IVS_WAVES), 0, st, x, F, D, ldx, offsets, gauss, post, n, I, posterior_scale,
                       acoustic_weight, max_count, gam, Fst);
    KTF_CHECK_LAUNCH(who);
    const int64_t P = (int64_t)S * (S + 1) / 2;
    int rc = iv_gemm(who, Fst, (int64_t)I * D, sigma_inv_M, S, (double*)(ws + l.lpart), lin, l.nkl, B, S, (int64_t)I * D, st);
    if (rc != KTF_OK) return rc;
    rc = iv_gemm(who, gam, I, U, P, (double*)(ws + l.qpart), q, l.nkq, B, P, I, st);
    if (rc != KTF_OK) return rc;
    return iv_solve(who, q, lin, offsets, B, F, S, prior_offset, (double*)(ws + l.L), ivectors, out_dtype_bytes, st);
}
