// Dense PLDA scoring of recordings with conversation-dependent PCA: Kaldi's `ivector-plda-scoring-dense`, the scoring stage of
// x-vector diarization, batched over the recordings of one call. The reference ships its golden table
// (testdata/plda/plda_scores.py, RefPldaScores.ark) and no implementation.
//
// Per recording r (rows X, n x D; P = min(n, D)):
//   dense_mean_kernel       m = mean(X)                                                        (fp64)
//   dense_moments_kernel    G = Xc Xc^T / n (n <= D) or Xc^T Xc / n (n > D), Xc = X - m         (fp64, P x P)
//   dense_jacobi_kernel     eigenvalues (descending) and eigenvectors of G                       (fp64)
//   dense_subspace_kernel   d (EstPca's loop, clamped to the numerical rank), M (d x D), K = M T^-1, W' = K K^T = L L^T,
//                           L^-1, H = L^-1 K, Bp = H diag(psi) H^T                                (fp64)
//   dense_jacobi_kernel     Bp = U diag(s) U^T                                                    (fp64)
//   dense_project_kernel    T' = U^T L^-1, A' = T' M, offset' = -A' mean, psi' = max(s, 0)        (fp64)
//   dense_transform_kernel  every row: A' x + offset', length norm in dimension d                (fp64 -> R)
//   dense_score_kernel      every pair of the recording's rows (plda_score_tile)                 (R)
// (Plda::ApplyTransform's W = T^-1 T^-T and B = T^-1 diag(psi) T^-T enter only as M W M^T = K K^T and
// C^-1 M B M^T C^-T = H diag(psi) H^T: one D x D product per recording instead of two, symmetric by construction.)
// Recordings without PCA (target_energy = KTF_PLDA_DENSE_NO_PCA, or rank 0) run the model as it is through plda_transform_row /
// plda_score_tile: PLDA.call's bits. Every stage is one launch over all recordings; sizes, offsets and d live on the device.
#include "common.h"
#include "plda_common.h"

namespace {

constexpr int DN_META = 8;                 // int64 per recording
enum { M_ROW = 0, M_N = 1, M_P = 2, M_SCORE = 3, M_WS = 4, M_GRAM = 5 };
constexpr int DN_THREADS = 1024;           // the per-recording kernels: one workgroup of 16 waves per recording
constexpr int JAC_LDS_MAX = KTF_PLDA_DENSE_JACOBI_LDS;                     // fp64 matrices up to this size stay in LDS
constexpr int JAC_HALF = KTF_PLDA_DENSE_MAX_DIM / 2;                       // pairs per round
constexpr size_t JAC_LDS_BYTES = sizeof(double) * ((size_t)JAC_LDS_MAX * JAC_LDS_MAX + 3 * JAC_HALF + 32 + KTF_PLDA_DENSE_MAX_DIM) +
                                 sizeof(int) * 2 * JAC_HALF;               // 143,616 B
constexpr double JAC_TOL = 1e-14;          // converged: off-diagonal Frobenius norm <= JAC_TOL * Frobenius norm

__host__ __device__ inline int64_t rnd32(int64_t v) { return (v + 31) & ~(int64_t)31; }

// fp64 scratch of one recording (offsets in doubles from its base): the host sizes it, the kernels address it
struct Region {
    double *mean, *lam, *off, *psi, *A, *V, *E, *M, *K, *H;
};
__host__ __device__ inline int64_t region_doubles(int64_t P, int64_t D) {
    return rnd32(D) + 3 * rnd32(P) + 3 * rnd32(P * P) + 3 * rnd32(P * D);
}
__device__ inline Region region(double* b, int64_t P, int64_t D) {
    Region g;
    g.mean = b; b += rnd32(D);
    g.lam = b; b += rnd32(P);
    g.off = b; b += rnd32(P);
    g.psi = b; b += rnd32(P);
    g.A = b; b += rnd32(P * P);
    g.V = b; b += rnd32(P * P);
    g.E = b; b += rnd32(P * P);
    g.M = b; b += rnd32(P * D);
    g.K = b; b += rnd32(P * D);
    g.H = b;
    return g;
}

// sum over the 1024 threads, the same value in every thread (red: 16 doubles of LDS; the caller syncs before red is reused)
__device__ inline double block_sum(double v, double* red) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0;
#pragma unroll
    for (int w = 0; w < DN_THREADS / 64; ++w) s += red[w];
    return s;
}

// ----------------------------------------------------------------------------- moments
template <typename R>
__global__ __launch_bounds__(512) void dense_mean_kernel(const R* __restrict__ x, int D, const int64_t* __restrict__ meta,
                                                         double* __restrict__ ws) {
    const int64_t* mt = meta + (int64_t)blockIdx.x * DN_META;
    const int64_t row0 = mt[M_ROW], n = mt[M_N];
    Region g = region(ws + mt[M_WS], mt[M_P], D);
    for (int c = threadIdx.x; c < D; c += 512) {
        double s = 0;
        for (int64_t i = 0; i < n; ++i) s += (double)x[(row0 + i) * D + c];
        g.mean[c] = s / (double)n;
    }
}

// G (P x P) of recording blockIdx.z in 32 x 32 tiles, four outputs per thread, the summed index staged 32 at a time.
// G[i][j] = sum_k Z(i, k) Z(j, k) / n with Z(i, k) = Xc[i][k] (Gram, k < D) or Xc[k][i] (covariance, k < n): (i, j) and (j, i)
// add the same products in the same order, G is symmetric bit for bit.
template <typename R>
__global__ __launch_bounds__(256) void dense_moments_kernel(const R* __restrict__ x, int D, const int64_t* __restrict__ meta,
                                                            double* __restrict__ ws) {
    __shared__ double zi[32][33], zj[32][33];
    const int64_t* mt = meta + (int64_t)blockIdx.z * DN_META;
    const int64_t row0 = mt[M_ROW], n = mt[M_N];
    const int P = (int)mt[M_P];
    const bool gram = mt[M_GRAM] != 0;
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    if (i0 >= P || j0 >= P) return;
    Region g = region(ws + mt[M_WS], P, D);
    const int64_t K = gram ? D : n;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    double acc[2][2] = {{0, 0}, {0, 0}};
    for (int64_t k0 = 0; k0 < K; k0 += 32) {
        __syncthreads();
        for (int e = threadIdx.x; e < 32 * 32; e += 256) {
            // Gram: consecutive threads walk k (a row of X); covariance: they walk i (again a row of X)
            const int a = gram ? e >> 5 : e & 31, kk = gram ? e & 31 : e >> 5;
            const int64_t k = k0 + kk;
            double vi = 0, vj = 0;
            if (k < K) {
                if (gram) {
                    const double mk = g.mean[k];
                    if (i0 + a < P) vi = (double)x[(row0 + i0 + a) * D + k] - mk;
                    if (j0 + a < P) vj = (double)x[(row0 + j0 + a) * D + k] - mk;
                } else {
                    if (i0 + a < P) vi = (double)x[(row0 + k) * D + i0 + a] - g.mean[i0 + a];
                    if (j0 + a < P) vj = (double)x[(row0 + k) * D + j0 + a] - g.mean[j0 + a];
                }
            }
            zi[a][kk] = vi;
            zj[a][kk] = vj;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < 32; ++kk) {
            const double a0 = zi[ty][kk], a1 = zi[ty + 16][kk], b0 = zj[tx][kk], b1 = zj[tx + 16][kk];
            acc[0][0] += a0 * b0; acc[0][1] += a0 * b1;
            acc[1][0] += a1 * b0; acc[1][1] += a1 * b1;
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int i = i0 + ty + 16 * u, j = j0 + tx + 16 * v;
            if (i < P && j < P) g.A[(int64_t)i * P + j] = acc[u][v] / (double)n;
        }
}

// ----------------------------------------------------------------------------- eigensolver
// Parallel-order cyclic Jacobi on the symmetric matrix in g.A (size N, row stride N), one workgroup per recording. A sweep is N' - 1
// rounds (N' = N rounded up to even; index N is a dummy that pairs with nothing) of the round-robin tournament: each round
// rotates N'/2 disjoint index pairs at once. A round's rotations act on disjoint 2 x 2 blocks of A, one thread per block pair
// (P <= Q; the mirror block is written from the same values), so no element is read by one thread and written by another.
// Eigenvectors accumulate as the ROWS of V (V <- J^T V), read and written along rows.
// The matrix lives in LDS while N <= JAC_LDS_MAX, in g.A (L2-resident) otherwise. At most KTF_PLDA_DENSE_MAX_SWEEPS sweeps: a
// matrix not converged by then adds 1 to *status (and is still sorted and written).
// Out: g.lam = eigenvalues, descending; g.A = the matching eigenvectors as rows (row stride N).
// Size N: meta's P (dims == NULL) or dims[r] (0: nothing to do).
__global__ __launch_bounds__(DN_THREADS) void dense_jacobi_kernel(const int64_t* __restrict__ meta, double* __restrict__ ws, int D,
                                                                  const int32_t* __restrict__ dims, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) double jl[];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int64_t* mt = meta + (int64_t)r * DN_META;
    const int P = (int)mt[M_P];
    const int N = dims ? dims[r] : P;
    if (N <= 0 || N > P) return;
    Region g = region(ws + mt[M_WS], P, D);
    double* pc = jl + JAC_LDS_MAX * JAC_LDS_MAX;
    double* ps = pc + JAC_HALF;
    double* pt = ps + JAC_HALF;
    double* red = pt + JAC_HALF;                                   // 32
    double* dg = red + 32;                                         // KTF_PLDA_DENSE_MAX_DIM
    int* pp = reinterpret_cast<int*>(dg + KTF_PLDA_DENSE_MAX_DIM);
    int* pq = pp + JAC_HALF;
    const bool in_lds = N <= JAC_LDS_MAX;
    double* A = in_lds ? jl : g.A;
    double* V = g.V;
    const int NN = N * N;
    for (int e = tid; e < NN; e += DN_THREADS) {
        if (in_lds) A[e] = g.A[e];
        V[e] = (e / N == e % N) ? 1.0 : 0.0;
    }
    const int m = N + (N & 1), h = m / 2;
    bool converged = false;
    for (int sw = 0;; ++sw) {
        __syncthreads();
        double o = 0, t = 0;
        for (int e = tid; e < NN; e += DN_THREADS) {
            const double v = A[e];
            t += v * v;
            if (e / N != e % N) o += v * v;
        }
        o = block_sum(o, red);
        __syncthreads();
        t = block_sum(t, red);
        if (o <= JAC_TOL * JAC_TOL * t || !(t > 0)) {              // (t == 0: the zero matrix; t NaN: cannot converge)
            converged = t == 0 || o <= JAC_TOL * JAC_TOL * t;
            break;
        }
        if (sw == KTF_PLDA_DENSE_MAX_SWEEPS) break;
        for (int rd = 0; rd < m - 1; ++rd) {
            if (tid < h) {
                int a, b;
                if (tid == 0) a = rd, b = m - 1;
                else a = (rd + tid) % (m - 1), b = (rd - tid + m - 1) % (m - 1);
                const int p = min(a, b), q = max(a, b);
                double c = 1, s = 0, tt = 0;
                if (q < N) {
                    const double apq = A[p * N + q];
                    if (apq != 0) {
                        const double th = (A[q * N + q] - A[p * N + p]) / (2 * apq);
                        tt = fabs(th) > 1e150 ? 0.5 / th : copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1));
                        c = 1 / sqrt(tt * tt + 1);
                        s = tt * c;
                    }
                }
                pp[tid] = p; pq[tid] = q; pc[tid] = c; ps[tid] = s; pt[tid] = tt;
            }
            __syncthreads();
            for (int e = tid; e < h * h; e += DN_THREADS) {
                const int bp = e / h, bq = e - bp * h;
                if (bq < bp) continue;
                const int p = pp[bp], q = pq[bp], u = pp[bq], w = pq[bq];
                const bool qv = q < N, wv = w < N;
                if (bp == bq) {
                    if (qv) {
                        const double apq = A[p * N + q], tt = pt[bp];
                        A[p * N + p] -= tt * apq;
                        A[q * N + q] += tt * apq;
                        A[p * N + q] = 0;
                        A[q * N + p] = 0;
                    }
                    continue;
                }
                const double c1 = pc[bp], s1 = ps[bp], c2 = pc[bq], s2 = ps[bq];
                const double x00 = A[p * N + u], x01 = wv ? A[p * N + w] : 0, x10 = qv ? A[q * N + u] : 0,
                             x11 = qv && wv ? A[q * N + w] : 0;
                const double y00 = c1 * x00 - s1 * x10, y01 = c1 * x01 - s1 * x11;      // J_P^T X
                const double y10 = s1 * x00 + c1 * x10, y11 = s1 * x01 + c1 * x11;
                const double z00 = c2 * y00 - s2 * y01, z01 = s2 * y00 + c2 * y01;      // ... J_Q
                const double z10 = c2 * y10 - s2 * y11, z11 = s2 * y10 + c2 * y11;
                A[p * N + u] = z00; A[u * N + p] = z00;
                if (wv) { A[p * N + w] = z01; A[w * N + p] = z01; }
                if (qv) { A[q * N + u] = z10; A[u * N + q] = z10; }
                if (qv && wv) { A[q * N + w] = z11; A[w * N + q] = z11; }
            }
            for (int e = tid; e < h * N; e += DN_THREADS) {
                const int k = e / N, col = e - k * N;
                const int q = pq[k];
                if (q >= N) continue;
                const int p = pp[k];
                const double c = pc[k], s = ps[k], vp = V[p * N + col], vq = V[q * N + col];
                V[p * N + col] = c * vp - s * vq;
                V[q * N + col] = s * vp + c * vq;
            }
            __syncthreads();
        }
    }
    if (!converged && tid == 0) atomicAdd(status, 1);
    __syncthreads();
    for (int i = tid; i < N; i += DN_THREADS) dg[i] = A[i * N + i];
    __syncthreads();
    int* rank = pp;                                                // 2 * JAC_HALF = KTF_PLDA_DENSE_MAX_DIM ints
    for (int i = tid; i < N; i += DN_THREADS) {
        const double li = dg[i];
        int k = 0;
        for (int j = 0; j < N; ++j) k += (dg[j] > li) || (dg[j] == li && j < i);
        rank[i] = k;
        g.lam[k] = li;
    }
    __syncthreads();
    for (int e = tid; e < NN; e += DN_THREADS) {
        const int i = e / N, col = e - i * N;
        g.A[rank[i] * N + col] = V[e];
    }
}

// ----------------------------------------------------------------------------- the model in the subspace
// d from the sorted eigenvalues (EstPca: tot = sum lam; e = 0; d = 1; while (e / tot <= target) e += lam[d++ - 1]), clamped to the
// count of eigenvalues above floor * lam[0] (none when lam[0] <= floor * (tot + |m|^2), the mean squared row norm); then M, K = M Tinv, W' = K K^T, its Cholesky factor L, L^-1, H = L^-1 K and
// Bp = H diag(psi) H^T (into g.A, row stride d, for the second eigensolve). d == 0: no PCA for this recording.
template <typename R>
__global__ __launch_bounds__(DN_THREADS) void dense_subspace_kernel(const R* __restrict__ x, int D, const int64_t* __restrict__ meta,
                                                                    double* __restrict__ ws, double target, double floor_rel,
                                                                    const double* __restrict__ Tinv, const double* __restrict__ psi,
                                                                    int32_t* __restrict__ dims, int32_t* __restrict__ status) {
    __shared__ int sd;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int64_t* mt = meta + (int64_t)r * DN_META;
    const int64_t row0 = mt[M_ROW], n = mt[M_N];
    const int P = (int)mt[M_P];
    const bool gram = mt[M_GRAM] != 0;
    Region g = region(ws + mt[M_WS], P, D);
    if (tid == 0) {
        double tot = 0;
        for (int k = 0; k < P; ++k) tot += g.lam[k];
        double e = 0;
        int d = 1;
        while (d - 1 < P && e / tot <= target) {
            e += g.lam[d - 1];
            ++d;
        }
        double m2 = 0;                                             // |m|^2: tot + m2 = the mean squared row norm
        for (int c = 0; c < D; ++c) m2 += g.mean[c] * g.mean[c];
        int rank = 0;
        if (g.lam[0] > floor_rel * (tot + m2))                     // (not so: rows equal up to rounding)
            while (rank < P && g.lam[rank] > floor_rel * g.lam[0]) ++rank;
        d = min(d, rank);
        sd = d;
        dims[r] = d;
    }
    __syncthreads();
    const int d = sd;
    if (d == 0) return;
    // M: the retained eigenvectors of the covariance as rows; Gram eigenvectors v are lifted: Xc^T v / sqrt(n lam)
    for (int e = tid; e < d * D; e += DN_THREADS) {
        const int k = e / D, c = e - k * D;
        double v;
        if (gram) {
            const double mc = g.mean[c];
            double s = 0;
            for (int64_t i = 0; i < n; ++i) s += g.A[(int64_t)k * P + i] * ((double)x[(row0 + i) * D + c] - mc);
            v = s / sqrt((double)n * g.lam[k]);
        } else {
            v = g.A[(int64_t)k * P + c];
        }
        g.M[(int64_t)k * D + c] = v;
    }
    __syncthreads();
    for (int e = tid; e < d * D; e += DN_THREADS) {                 // K = M Tinv
        const int k = e / D, c = e - k * D;
        double s = 0;
        for (int l = 0; l < D; ++l) s += g.M[(int64_t)k * D + l] * Tinv[(int64_t)l * D + c];
        g.K[(int64_t)k * D + c] = s;
    }
    __syncthreads();
    double* L = g.V;                                               // W' = K K^T, then its Cholesky factor (lower)
    for (int e = tid; e < d * d; e += DN_THREADS) {
        const int a = e / d, b = e - a * d;
        double s = 0;
        for (int c = 0; c < D; ++c) s += g.K[(int64_t)a * D + c] * g.K[(int64_t)b * D + c];
        L[e] = s;
    }
    __syncthreads();
    for (int k = 0; k < d; ++k) {
        if (tid == 0) {
            const double v = L[k * d + k];
            if (!(v > 0)) atomicAdd(status, 1);                    // (K has full row rank: W' is positive definite)
            L[k * d + k] = sqrt(v > 0 ? v : 1e-300);
        }
        __syncthreads();
        const double lkk = L[k * d + k];
        for (int i = k + 1 + tid; i < d; i += DN_THREADS) L[i * d + k] /= lkk;
        __syncthreads();
        const int t = d - k - 1;
        for (int e = tid; e < t * t; e += DN_THREADS) {
            const int i = k + 1 + e / t, j = k + 1 + e % t;
            if (j <= i) L[i * d + j] -= L[i * d + k] * L[j * d + k];
        }
        __syncthreads();
    }
    double* Li = g.E;                                              // L^-1 (lower), row by row
    for (int e = tid; e < d * d; e += DN_THREADS) Li[e] = 0;
    __syncthreads();
    for (int i = 0; i < d; ++i) {
        for (int j = tid; j <= i; j += DN_THREADS) {
            double s = i == j ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) s -= L[i * d + k] * Li[k * d + j];
            Li[i * d + j] = s / L[i * d + i];
        }
        __syncthreads();
    }
    for (int e = tid; e < d * D; e += DN_THREADS) {                 // H = L^-1 K
        const int a = e / D, c = e - a * D;
        double s = 0;
        for (int k = 0; k <= a; ++k) s += Li[a * d + k] * g.K[(int64_t)k * D + c];
        g.H[(int64_t)a * D + c] = s;
    }
    __syncthreads();
    for (int e = tid; e < d * d; e += DN_THREADS) {                 // Bp = H diag(psi) H^T
        const int a = e / d, b = e - a * d;
        double s = 0;
        for (int c = 0; c < D; ++c) s += g.H[(int64_t)a * D + c] * g.H[(int64_t)b * D + c] * psi[c];     // (symmetric bit for bit)
        g.A[e] = s;
    }
}

// T' = U^T L^-1 (U^T: the rows dense_jacobi_kernel left in g.A), A' = T' M (into g.K), offset' = -A' mean, psi' = max(s, 0)
// (Plda::ApplyTransform floors psi at 0); psi' also in the layer's dtype for the score tiles.
template <typename R>
__global__ __launch_bounds__(DN_THREADS) void dense_project_kernel(int D, const int64_t* __restrict__ meta, double* __restrict__ ws,
                                                                   const double* __restrict__ mean, const int32_t* __restrict__ dims,
                                                                   R* __restrict__ psi_r) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const int d = dims[r];
    if (d == 0) return;
    const int64_t* mt = meta + (int64_t)r * DN_META;
    Region g = region(ws + mt[M_WS], mt[M_P], D);
    double* Tp = g.V;
    for (int e = tid; e < d * d; e += DN_THREADS) {
        const int k = e / d, j = e - k * d;
        double s = 0;
        for (int m = j; m < d; ++m) s += g.A[k * d + m] * g.E[m * d + j];
        Tp[e] = s;
    }
    __syncthreads();
    for (int e = tid; e < d * D; e += DN_THREADS) {
        const int k = e / D, c = e - k * D;
        double s = 0;
        for (int j = 0; j < d; ++j) s += Tp[k * d + j] * g.M[(int64_t)j * D + c];
        g.K[(int64_t)k * D + c] = s;
    }
    __syncthreads();
    for (int k = tid >> 6; k < d; k += DN_THREADS / 64) {
        double s = 0;
        for (int c = tid & 63; c < D; c += 64) s += g.K[(int64_t)k * D + c] * mean[c];
        s = wave_sum_d(s);
        if ((tid & 63) == 0) g.off[k] = -s;
    }
    for (int k = tid; k < d; k += DN_THREADS) {
        const double p = fmax(g.lam[k], 0.0);
        g.psi[k] = p;
        psi_r[(int64_t)r * D + k] = (R)p;
    }
}

// ----------------------------------------------------------------------------- transform and scores
__device__ inline int find_recording(const int64_t* meta, int R_, int64_t row) {
    int lo = 0, hi = R_ - 1;                                       // the last recording whose first row is <= row
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (meta[(int64_t)mid * DN_META + M_ROW] <= row) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One workgroup per row. d == 0: plda_transform_row with the model (PLDA.call's bits), D values at tr + row * D. Otherwise
// z = A' x + offset' and the length norm in fp64 with dimension d, stored as R at tr + row0 * D + (row - row0) * d.
template <typename R>
__global__ __launch_bounds__(256) void dense_transform_kernel(const R* __restrict__ x, int D, const int64_t* __restrict__ meta, int R_,
                                                              double* __restrict__ ws, const int32_t* __restrict__ dims,
                                                              const R* __restrict__ A, const R* __restrict__ offset,
                                                              const R* __restrict__ psi, int normalize, int simple,
                                                              R* __restrict__ tr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    const int64_t row = blockIdx.x;
    const int r = find_recording(meta, R_, row);
    const int d = dims[r];
    if (d == 0) {
        plda_transform_row<R>(x + row * D, D, A, offset, psi, normalize, simple, tr + row * D, smraw);
        return;
    }
    const int64_t* mt = meta + (int64_t)r * DN_META;
    const int64_t row0 = mt[M_ROW];
    Region g = region(ws + mt[M_WS], mt[M_P], D);
    double* xs = reinterpret_cast<double*>(smraw);
    double* ys = xs + D;
    double* red = ys + D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < D; i += 256) xs[i] = (double)x[row * D + i];
    __syncthreads();
    for (int k = wave; k < d; k += 4) {
        double acc = 0;
        for (int c = lane; c < D; c += 64) acc += g.K[(int64_t)k * D + c] * xs[c];
        acc = wave_sum_d(acc);
        if (lane == 0) ys[k] = acc + g.off[k];
    }
    __syncthreads();
    double f = 1;
    if (normalize) {
        double part = 0;
        for (int k = threadIdx.x; k < d; k += 256) {
            const double v = ys[k];
            part += simple ? v * v : v * v / (g.psi[k] + 1.0);
        }
        part = wave_sum_d(part);
        if (lane == 0) red[wave] = part;
        __syncthreads();
        const double tot = red[0] + red[1] + red[2] + red[3];
        f = sqrt((double)d / tot);
    }
    R* out = tr + row0 * D + (row - row0) * d;
    for (int k = threadIdx.x; k < d; k += 256) out[k] = (R)(ys[k] * f);
}

// 64 x 64 tiles of every recording's n x n block (blockIdx.z = recording), packed at scores + its offset.
template <typename R>
__global__ __launch_bounds__(256) void dense_score_kernel(const R* __restrict__ tr, int D, const int64_t* __restrict__ meta,
                                                          const int32_t* __restrict__ dims, const R* __restrict__ psi,
                                                          const R* __restrict__ psi_r, R* __restrict__ scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];      // PLDA_LDS_BYTES(R)
    const int r = blockIdx.z;
    const int64_t* mt = meta + (int64_t)r * DN_META;
    const int64_t n = mt[M_N], i0 = (int64_t)blockIdx.y * PLDA_TILE, j0 = (int64_t)blockIdx.x * PLDA_TILE;
    if (i0 >= n || j0 >= n) return;
    const int d = dims[r];
    const R* y = tr + mt[M_ROW] * D;
    plda_score_tile<R>(y, n, y, n, d ? d : D, d ? psi_r + (int64_t)r * D : psi, scores + mt[M_SCORE], i0, j0, smraw);
}

// ----------------------------------------------------------------------------- per-recording table
struct Layout {
    size_t meta, tr, psi_r, f64, total;    // byte offsets into the workspace
    int64_t S, max_n, max_p;
};

// The per-recording table (meta, DN_META int64 each: first row, n, P, score offset, fp64 scratch offset, Gram?) and the totals the
// host sizes the call by. The host runs it to check and size, the device (dense_meta_kernel) to fill the table.
__host__ __device__ inline void fill_meta(const int32_t* lengths, int32_t R_, int32_t dim, bool pca, int64_t* meta, int64_t* S_out,
                                          int64_t* f64_out, int64_t* max_n, int64_t* max_p) {
    int64_t S = 0, sc = 0, f64 = 0, mn = 0, mp = 0;
    for (int32_t r = 0; r < R_; ++r) {
        const int64_t n = lengths[r], P = n < dim ? n : dim;
        if (meta) {
            int64_t* m = meta + (int64_t)r * DN_META;
            m[M_ROW] = S; m[M_N] = n; m[M_P] = P; m[M_SCORE] = sc; m[M_WS] = f64; m[M_GRAM] = n <= dim;
            m[6] = m[7] = 0;
        }
        S += n;
        sc += n * n;
        if (pca) f64 += region_doubles(P, dim);
        mn = n > mn ? n : mn;
        mp = P > mp ? P : mp;
    }
    *S_out = S; *f64_out = f64; *max_n = mn; *max_p = mp;
}

__global__ void dense_meta_kernel(const int32_t* __restrict__ lengths, int32_t R_, int32_t dim, int pca, int64_t* __restrict__ meta) {
    int64_t S, f64, mn, mp;
    if (threadIdx.x == 0) fill_meta(lengths, R_, dim, pca != 0, meta, &S, &f64, &mn, &mp);
}

// ----------------------------------------------------------------------------- host side
// Checks lengths (a HOST array) and sizes the workspace.
static int dense_layout(const char* who, const int32_t* lengths, int32_t R_, int32_t dim, bool pca, Layout* lay) {
    KTF_REQUIRE(lengths, "%s: null lengths", who);
    KTF_REQUIRE(R_ >= 1, "%s: need at least one recording (R = %d)", who, (int)R_);
    KTF_REQUIRE(dim >= 1 && dim <= KTF_PLDA_DENSE_MAX_DIM, "%s: dim %d outside 1..%d (PLDA.call serves any dim)", who, (int)dim,
                KTF_PLDA_DENSE_MAX_DIM);
    for (int32_t r = 0; r < R_; ++r)
        KTF_REQUIRE(lengths[r] >= 1, "%s: lengths[%d] = %d, every recording needs a row", who, (int)r, (int)lengths[r]);
    int64_t f64 = 0;
    fill_meta(lengths, R_, dim, pca, nullptr, &lay->S, &f64, &lay->max_n, &lay->max_p);
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    lay->meta = 0;
    lay->tr = al((size_t)R_ * DN_META * sizeof(int64_t));
    lay->psi_r = lay->tr + al((size_t)lay->S * dim * sizeof(double));
    lay->f64 = lay->psi_r + al((size_t)R_ * dim * sizeof(double));
    lay->total = lay->f64 + al((size_t)f64 * sizeof(double));
    return KTF_OK;
}

static bool dense_no_pca(double t) { return t == KTF_PLDA_DENSE_NO_PCA; }

template <typename R>
static int plda_dense_launch(const char* who, const R* x, int64_t S, int32_t dim, const int32_t* lengths,
                             const int32_t* lengths_dev, int32_t R_, double target, const R* A, const R* offset, const R* psi, const double* mean64,
                             const double* Tinv64, const double* psi64, int32_t normalize_length, int32_t simple_length_norm,
                             R* scores, int32_t* dims, void* workspace, size_t workspace_bytes, int32_t* status, void* stream) {
    const bool pca = !dense_no_pca(target);
    KTF_REQUIRE(x && lengths_dev && A && offset && psi && scores && dims && workspace && status, "%s: null argument", who);
    KTF_REQUIRE(!pca || (mean64 && Tinv64 && psi64), "%s: null fp64 model constant (mean64 / Tinv64 / psi64)", who);
    KTF_REQUIRE(!pca || (target >= 0 && target < 1), "%s: target_energy %g outside [0, 1) (KTF_PLDA_DENSE_NO_PCA: no PCA)", who,
                target);
    Layout lay;
    int rc = dense_layout(who, lengths, R_, dim, pca, &lay);
    if (rc != KTF_OK) return rc;
    KTF_REQUIRE(lay.S == S, "%s: lengths add up to %lld rows, x has %lld", who, (long long)lay.S, (long long)S);
    KTF_REQUIRE(workspace_bytes >= lay.total, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes, lay.total);
    KTF_REQUIRE(ktf_cdiv(lay.max_n, PLDA_TILE) < 65536 && R_ < 65536, "%s: too many rows or recordings", who);

    hipStream_t st = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)workspace;
    int64_t* meta = (int64_t*)(w + lay.meta);
    R* tr = (R*)(w + lay.tr);
    R* psi_r = (R*)(w + lay.psi_r);
    double* ws = (double*)(w + lay.f64);
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(dims, 0, (size_t)R_ * sizeof(int32_t), st);
    if (e != hipSuccess) {
        ktf_set_error("%s: %s", who, hipGetErrorString(e));
        return KTF_ELAUNCH;
    }
    hipLaunchKernelGGL(dense_meta_kernel, dim3(1), dim3(64), 0, st, lengths_dev, R_, dim, (int)pca, meta);
    KTF_CHECK_LAUNCH(who);
    if (pca) {
        const double floor_rel = sizeof(R) == 8 ? KTF_PLDA_DENSE_RANK_FLOOR_F64 : KTF_PLDA_DENSE_RANK_FLOOR_F32;
        const unsigned tp = (unsigned)ktf_cdiv(lay.max_p, 32);
        hipLaunchKernelGGL(dense_mean_kernel<R>, dim3((unsigned)R_), dim3(512), 0, st, x, dim, meta, ws);
        KTF_CHECK_LAUNCH(who);
        hipLaunchKernelGGL(dense_moments_kernel<R>, dim3(tp, tp, (unsigned)R_), dim3(256), 0, st, x, dim, meta, ws);
        KTF_CHECK_LAUNCH(who);
        KTF_LDS_ONCE((int)JAC_LDS_BYTES, dense_jacobi_kernel);
        hipLaunchKernelGGL(dense_jacobi_kernel, dim3((unsigned)R_), dim3(DN_THREADS), JAC_LDS_BYTES, st, meta, ws, dim,
                           (const int32_t*)nullptr, status);
        KTF_CHECK_LAUNCH(who);
        hipLaunchKernelGGL(dense_subspace_kernel<R>, dim3((unsigned)R_), dim3(DN_THREADS), 0, st, x, dim, meta, ws, target,
                           floor_rel, Tinv64, psi64, dims, status);
        KTF_CHECK_LAUNCH(who);
        hipLaunchKernelGGL(dense_jacobi_kernel, dim3((unsigned)R_), dim3(DN_THREADS), JAC_LDS_BYTES, st, meta, ws, dim,
                           (const int32_t*)dims, status);
        KTF_CHECK_LAUNCH(who);
        hipLaunchKernelGGL(dense_project_kernel<R>, dim3((unsigned)R_), dim3(DN_THREADS), 0, st, dim, meta, ws, mean64, dims, psi_r);
        KTF_CHECK_LAUNCH(who);
    }
    const size_t lds_t = sizeof(double) * (2 * (size_t)dim + 8);
    hipLaunchKernelGGL(dense_transform_kernel<R>, dim3((unsigned)S), dim3(256), lds_t, st, x, dim, meta, R_, ws, dims, A, offset, psi,
                       normalize_length, simple_length_norm, tr);
    KTF_CHECK_LAUNCH(who);
    const unsigned ts = (unsigned)ktf_cdiv(lay.max_n, PLDA_TILE);
    KTF_LDS_ONCE((int)PLDA_LDS_BYTES(R), dense_score_kernel<R>);
    hipLaunchKernelGGL(dense_score_kernel<R>, dim3(ts, ts, (unsigned)R_), dim3(256), PLDA_LDS_BYTES(R), st, tr, dim, meta, dims, psi,
                       psi_r, scores);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

}  // namespace

extern "C" int64_t ktf_plda_dense_workspace_bytes(const int32_t* lengths, int32_t R, int32_t dim, double target_energy) {
    Layout lay;
    const int rc = dense_layout("ktf_plda_dense_workspace_bytes", lengths, R, dim, !dense_no_pca(target_energy), &lay);
    return rc == KTF_OK ? (int64_t)lay.total : (int64_t)rc;
}

extern "C" int ktf_plda_dense_f64(const double* x, int64_t S, int32_t dim, const int32_t* lengths, const int32_t* lengths_dev,
                                  int32_t R, double target_energy, const double* A, const double* offset, const double* psi,
                                  const double* mean64, const double* Tinv64, const double* psi64, int32_t normalize_length,
                                  int32_t simple_length_norm, double* scores, int32_t* dims, void* workspace,
                                  size_t workspace_bytes, int32_t* status, void* stream) {
    return plda_dense_launch<double>("ktf_plda_dense_f64", x, S, dim, lengths, lengths_dev, R, target_energy, A, offset, psi, mean64, Tinv64,
                                     psi64, normalize_length, simple_length_norm, scores, dims, workspace, workspace_bytes,
                                     status, stream);
}
extern "C" int ktf_plda_dense_f32(const float* x, int64_t S, int32_t dim, const int32_t* lengths, const int32_t* lengths_dev,
                                  int32_t R, double target_energy, const float* A, const float* offset, const float* psi,
                                  const double* mean64, const double* Tinv64, const double* psi64, int32_t normalize_length,
                                  int32_t simple_length_norm, float* scores, int32_t* dims, void* workspace,
                                  size_t workspace_bytes, int32_t* status, void* stream) {
    return plda_dense_launch<float>("ktf_plda_dense_f32", x, S, dim, lengths, lengths_dev, R, target_energy, A, offset, psi, mean64, Tinv64,
                                    psi64, normalize_length, simple_length_norm, scores, dims, workspace, workspace_bytes,
                                    status, stream);
}
