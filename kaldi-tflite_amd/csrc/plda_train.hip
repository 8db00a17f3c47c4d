// PLDA back-end training statistics: the parts of Kaldi's `ivector-compute-lda`, `ivector-compute-plda` and
// `est-pca --read-vectors=true` whose cost grows with the number of rows N or speakers S. The O(D^3)
// factorisations (Cholesky, symmetric eigendecompositions) run in fp64 NumPy on the host (kaldi_tflite_amd/training.py).
//
//   class_stats_kernel      per speaker: the fp64 sum of its rows in list order, divided by the count; the count   (fp32 -> fp64)
//   colsum_kernel           fixed row chunks: the fp64 column sums of each chunk, then the chunks added in order   (-> fp64)
//   gram_kernel             G = sum_r w_r (y_r - c)(y_r - c)^T over fixed row chunks, upper-triangle 64 x 64 tiles  (fp64)
//   gram_reduce_kernel      the chunks' partial tiles added in chunk order; (i, j) and (j, i) written from one value
//   em_project_kernel       y_s = P (mu_s - mbar); a_s = n_s lam / (1 + n_s lam) y_s, b_s = y_s / (1 + n_s lam)    (fp64)
//
// Determinism: every split of the rows depends on the row count and D only; partial sums are added in a fixed order by one
// thread each; no atomics. Results are bit-identical run to run and independent of the device or stream.
#include "common.h"

namespace {

constexpr int TILE = 64;                   // output tile (TILE x TILE), 256 threads, 4 x 4 outputs per thread
constexpr int KSTEP = 16;                  // rows (gram) / summed index (projection) staged per LDS round
constexpr int GRAM_MIN_ROWS = 512;         // a chunk holds at least this many rows ...
constexpr int GRAM_MAX_BLOCKS = 1024;      // ... and tiles x chunks stays below this (about four workgroups per CU)
constexpr int COLSUM_ROWS = 256;           // rows per chunk of colsum_kernel

__host__ __device__ inline int gram_tiles_1d(int D) { return (D + TILE - 1) / TILE; }
__host__ __device__ inline int gram_tiles(int D) {
    const int t = gram_tiles_1d(D);
    return t * (t + 1) / 2;
}
inline int64_t gram_chunks(int64_t rows, int D) {
    const int64_t by_rows = (rows + GRAM_MIN_ROWS - 1) / GRAM_MIN_ROWS;
    const int64_t cap = GRAM_MAX_BLOCKS / gram_tiles(D) > 1 ? GRAM_MAX_BLOCKS / gram_tiles(D) : 1;
    return by_rows < 1 ? 1 : (by_rows < cap ? by_rows : cap);
}

// upper-triangle tile t (0 .. nt(nt+1)/2) -> (ti, tj), ti <= tj, row by row
__device__ inline void tile_of(int t, int nt, int& ti, int& tj) {
    ti = 0;
    while (t >= nt - ti) {
        t -= nt - ti;
        ++ti;
    }
    tj = ti + t;
}

// acc[u][v] += sum_k zi[k][ty + 16u] * zj[k][tx + 16v]: the staged rows in order (one chain per output)
__device__ inline void tile_fma(const double (*zi)[TILE + 1], const double (*zj)[TILE + 1], int ty, int tx, double acc[4][4]) {
#pragma unroll 4
    for (int k = 0; k < KSTEP; ++k) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = zi[k][ty + 16 * u];
            b[u] = zj[k][tx + 16 * u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[u][v] += a[u] * b[v];
    }
}

// ----------------------------------------------------------------------------- per-speaker means
// One workgroup per speaker, threads over D. A speaker whose range of the list is empty or outside it, or who names a row outside x,
// gets a NaN row and count 0 (the host refuses such maps before launching: this only keeps the kernel inside its arrays).
__global__ __launch_bounds__(256) void class_stats_kernel(const float* __restrict__ x, int64_t N, int D, const int32_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ utts, int64_t n_idx, double* __restrict__ means,
                                                          int32_t* __restrict__ counts) {
    const int64_t s = blockIdx.x;
    const int64_t lo = offsets[s], hi = offsets[s + 1];
    bool ok = lo >= 0 && lo < hi && hi <= n_idx;
    for (int64_t k = lo; ok && k < hi; ++k) ok = utts[k] >= 0 && utts[k] < N;
    for (int d = threadIdx.x; d < D; d += 256) {
        double acc = 0.0;
        if (ok)
            for (int64_t k = lo; k < hi; ++k) acc += (double)x[(int64_t)utts[k] * D + d];
        means[s * D + d] = ok ? acc / (double)(hi - lo) : __builtin_nan("");
    }
    if (threadIdx.x == 0) counts[s] = ok ? (int32_t)(hi - lo) : 0;
}

// ----------------------------------------------------------------------------- column sums
// Partial sums of rows [c * COLSUM_ROWS, ...) of chunk c (blockIdx.y), columns blockIdx.x * 256 + threadIdx.x, in row order.
template <typename R>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const R* __restrict__ y, int64_t rows, int D, double* __restrict__ part) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    const int64_t r0 = (int64_t)blockIdx.y * COLSUM_ROWS;
    const int64_t r1 = r0 + COLSUM_ROWS < rows ? r0 + COLSUM_ROWS : rows;
    double acc = 0.0;
#pragma unroll 8
    for (int64_t r = r0; r < r1; ++r) acc += (double)y[r * D + d];
    part[(int64_t)blockIdx.y * D + d] = acc;
}

__global__ __launch_bounds__(256) void colsum_reduce_kernel(const double* __restrict__ part, int64_t chunks, int D, double scale,
                                                            double* __restrict__ out) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    double acc = 0.0;
    for (int64_t c = 0; c < chunks; ++c) acc += part[c * D + d];
    out[d] = acc * scale;
}

// ----------------------------------------------------------------------------- weighted Gram matrix
// Workgroup (tile blockIdx.x, chunk blockIdx.y): the chunk's rows of sum_r w_r (y_r - c)(y_r - c)^T on the upper-triangle tile, in
// row order, to part[chunk][tile][64][64]. Row r of the list is y[idx ? idx[r] : r]; a listed index outside [0, N) contributes
// nothing (the host refuses such lists: this only keeps the kernel inside its arrays). w (per list position) and c may be null.
template <typename R>
__global__ __launch_bounds__(256) void gram_kernel(const R* __restrict__ y, int64_t N, int D, const int32_t* __restrict__ idx,
                                                   int64_t rows, const double* __restrict__ center, const double* __restrict__ w,
                                                   int64_t chunks, double* __restrict__ part) {
    __shared__ double zi[KSTEP][TILE + 1], zj[KSTEP][TILE + 1];
    const int nt = gram_tiles_1d(D);
    int ti, tj;
    tile_of(blockIdx.x, nt, ti, tj);
    const int i0 = ti * TILE, j0 = tj * TILE;
    const int64_t per = (rows + chunks - 1) / chunks;
    const int64_t r0 = (int64_t)blockIdx.y * per;
    const int64_t r1 = r0 + per < rows ? r0 + per : rows;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    double acc[4][4] = {};
    for (int64_t k0 = r0; k0 < r1; k0 += KSTEP) {
        __syncthreads();
        for (int e = threadIdx.x; e < KSTEP * TILE; e += 256) {
            const int kk = e / TILE, col = e % TILE;
            const int64_t r = k0 + kk;
            double vi = 0, vj = 0;
            if (r < r1) {
                const int64_t row = idx ? (int64_t)idx[r] : r;
                if (row >= 0 && row < N) {
                    const double wr = w ? w[r] : 1.0;
                    const R* yr = y + row * D;
                    if (i0 + col < D) vi = wr * ((double)yr[i0 + col] - (center ? center[i0 + col] : 0.0));
                    if (j0 + col < D) vj = (double)yr[j0 + col] - (center ? center[j0 + col] : 0.0);
                }
            }
            zi[kk][col] = vi;
            zj[kk][col] = vj;
        }
        __syncthreads();
        tile_fma(zi, zj, ty, tx, acc);
    }
    double* out = part + ((int64_t)blockIdx.y * gram_tiles(D) + blockIdx.x) * (TILE * TILE);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) out[(ty + 16 * u) * TILE + tx + 16 * v] = acc[u][v];
}

// G (D x D) from the partial tiles, chunks added in order; an element (i, j), i <= j, is read from its upper-triangle tile and
// written to (i, j) and (j, i): G is symmetric bit for bit.
__global__ __launch_bounds__(256) void gram_reduce_kernel(const double* __restrict__ part, int D, int64_t chunks,
                                                          double* __restrict__ G) {
    const int nt = gram_tiles_1d(D), T = gram_tiles(D);
    int ti, tj;
    tile_of(blockIdx.x, nt, ti, tj);
    for (int e = threadIdx.x; e < TILE * TILE; e += 256) {
        const int i = ti * TILE + e / TILE, j = tj * TILE + e % TILE;
        if (i >= D || j >= D || i > j) continue;
        double acc = 0.0;
        for (int64_t c = 0; c < chunks; ++c) acc += part[(c * T + blockIdx.x) * (TILE * TILE) + e];
        G[(int64_t)i * D + j] = acc;
        G[(int64_t)j * D + i] = acc;
    }
}

// ----------------------------------------------------------------------------- EM row transform
// Workgroup (column tile blockIdx.x, speaker tile blockIdx.y): y[s][d] = sum_k (mu[s][k] - mbar[k]) P[d][k] in k order, then
// a[s][d] = n_s lam_d / (1 + n_s lam_d) y[s][d] and b[s][d] = y[s][d] / (1 + n_s lam_d).
__global__ __launch_bounds__(256) void em_project_kernel(const double* __restrict__ mu, int64_t S, int D, const double* __restrict__ mbar,
                                                         const double* __restrict__ P, const double* __restrict__ lam,
                                                         const int32_t* __restrict__ counts, double* __restrict__ a,
                                                         double* __restrict__ b) {
    __shared__ double zs[KSTEP][TILE + 1], zp[KSTEP][TILE + 1];
    const int64_t s0 = (int64_t)blockIdx.y * TILE;
    const int d0 = blockIdx.x * TILE;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    double acc[4][4] = {};
    for (int k0 = 0; k0 < D; k0 += KSTEP) {
        __syncthreads();
        for (int e = threadIdx.x; e < KSTEP * TILE; e += 256) {
            const int kk = e % KSTEP, col = e / KSTEP;              // consecutive threads walk k: a row of mu / of P
            const int k = k0 + kk;
            double vs = 0, vp = 0;
            if (k < D) {
                if (s0 + col < S) vs = mu[(s0 + col) * D + k] - mbar[k];
                if (d0 + col < D) vp = P[(int64_t)(d0 + col) * D + k];
            }
            zs[kk][col] = vs;
            zp[kk][col] = vp;
        }
        __syncthreads();
        tile_fma(zs, zp, ty, tx, acc);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t s = s0 + ty + 16 * u;
        if (s >= S) continue;
        const double n = (double)counts[s];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int d = d0 + tx + 16 * v;
            if (d >= D) continue;
            const double nl = n * lam[d], den = 1.0 + nl;
            a[s * D + d] = nl / den * acc[u][v];
            b[s * D + d] = acc[u][v] / den;
        }
    }
}

}  // namespace

// ----------------------------------------------------------------------------- C-ABI
extern "C" int ktf_train_class_means(const float* x, int64_t N, int32_t D, const int32_t* offsets, int64_t S, const int32_t* utts,
                                     int64_t n_idx, double* means, int32_t* counts, void* stream) {
    KTF_REQUIRE(x && offsets && utts && means && counts, "ktf_train_class_means: null argument");
    KTF_REQUIRE(N >= 1 && S >= 1 && n_idx >= 1, "ktf_train_class_means: bad sizes (N >= 1, S >= 1, n_idx >= 1)");
    KTF_REQUIRE(D >= 1 && D <= KTF_TRAIN_MAX_DIM, "ktf_train_class_means: D must be in 1 .. %d", KTF_TRAIN_MAX_DIM);
    KTF_REQUIRE(S < (1ll << 31) && n_idx < (1ll << 31), "ktf_train_class_means: too many speakers or list entries");
    hipLaunchKernelGGL(class_stats_kernel, dim3((unsigned)S), dim3(256), 0, (hipStream_t)stream, x, N, (int)D, offsets, utts, n_idx,
                       means, counts);
    KTF_CHECK_LAUNCH("ktf_train_class_means");
    return KTF_OK;
}

extern "C" int64_t ktf_train_workspace_bytes(int64_t rows, int32_t D) {
    KTF_REQUIRE(rows >= 1, "ktf_train_workspace_bytes: rows must be >= 1");
    KTF_REQUIRE(D >= 1 && D <= KTF_TRAIN_MAX_DIM, "ktf_train_workspace_bytes: D must be in 1 .. %d", KTF_TRAIN_MAX_DIM);
    const int64_t gram = gram_chunks(rows, D) * gram_tiles(D) * (int64_t)(TILE * TILE);
    const int64_t cols = (rows + COLSUM_ROWS - 1) / COLSUM_ROWS * (int64_t)D;
    return (int64_t)sizeof(double) * (gram > cols ? gram : cols);
}

template <typename R>
static int colmean(const char* who, const R* y, int64_t rows, int32_t D, double* out, void* ws, size_t ws_bytes, void* stream) {
    KTF_REQUIRE(y && out && ws, "%s: null argument", who);
    KTF_REQUIRE(rows >= 1, "%s: bad sizes (rows >= 1)", who);
    KTF_REQUIRE(D >= 1 && D <= KTF_TRAIN_MAX_DIM, "%s: D must be in 1 .. %d", who, KTF_TRAIN_MAX_DIM);
    const int64_t chunks = (rows + COLSUM_ROWS - 1) / COLSUM_ROWS;
    KTF_REQUIRE(chunks < 65536, "%s: too many rows", who);
    KTF_REQUIRE(ws_bytes >= (size_t)ktf_train_workspace_bytes(rows, D), "%s: workspace too small", who);
    const unsigned bx = (unsigned)ktf_cdiv(D, 256);
    hipLaunchKernelGGL(colsum_partial_kernel<R>, dim3(bx, (unsigned)chunks), dim3(256), 0, (hipStream_t)stream, y, rows, (int)D,
                       (double*)ws);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(colsum_reduce_kernel, dim3(bx), dim3(256), 0, (hipStream_t)stream, (const double*)ws, chunks, (int)D,
                       1.0 / (double)rows, out);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_train_mean_f32(const float* x, int64_t rows, int32_t D, double* mean, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    return colmean("ktf_train_mean_f32", x, rows, D, mean, workspace, workspace_bytes, stream);
}
extern "C" int ktf_train_mean_f64(const double* y, int64_t rows, int32_t D, double* mean, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    return colmean("ktf_train_mean_f64", y, rows, D, mean, workspace, workspace_bytes, stream);
}

template <typename R>
static int gram(const char* who, const R* y, int64_t N, int32_t D, const int32_t* idx, int64_t rows, const double* center,
                const double* weights, double* G, void* ws, size_t ws_bytes, void* stream) {
    KTF_REQUIRE(y && G && ws, "%s: null argument", who);
    KTF_REQUIRE(N >= 1 && rows >= 1 && (idx || rows <= N), "%s: bad sizes (N >= 1, rows >= 1, rows <= N without idx)", who);
    KTF_REQUIRE(D >= 1 && D <= KTF_TRAIN_MAX_DIM, "%s: D must be in 1 .. %d", who, KTF_TRAIN_MAX_DIM);
    KTF_REQUIRE(rows < (1ll << 40), "%s: too many rows", who);
    KTF_REQUIRE(ws_bytes >= (size_t)ktf_train_workspace_bytes(rows, D), "%s: workspace too small", who);
    const int64_t chunks = gram_chunks(rows, D);
    const int T = gram_tiles(D);
    hipLaunchKernelGGL(gram_kernel<R>, dim3((unsigned)T, (unsigned)chunks), dim3(256), 0, (hipStream_t)stream, y, N, (int)D, idx, rows,
                       center, weights, chunks, (double*)ws);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, (const double*)ws, (int)D, chunks, G);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_train_gram_f32(const float* x, int64_t N, int32_t D, const int32_t* idx, int64_t rows, const double* center,
                                  const double* weights, double* G, void* workspace, size_t workspace_bytes, void* stream) {
    return gram("ktf_train_gram_f32", x, N, D, idx, rows, center, weights, G, workspace, workspace_bytes, stream);
}
extern "C" int ktf_train_gram_f64(const double* y, int64_t N, int32_t D, const int32_t* idx, int64_t rows, const double* center,
                                  const double* weights, double* G, void* workspace, size_t workspace_bytes, void* stream) {
    return gram("ktf_train_gram_f64", y, N, D, idx, rows, center, weights, G, workspace, workspace_bytes, stream);
}

extern "C" int ktf_plda_em_project(const double* mu, int64_t S, int32_t D, const double* mbar, const double* P, const double* lam,
                                   const int32_t* counts, double* a, double* b, void* stream) {
    KTF_REQUIRE(mu && mbar && P && lam && counts && a && b, "ktf_plda_em_project: null argument");
    KTF_REQUIRE(S >= 1, "ktf_plda_em_project: bad sizes (S >= 1)");
    KTF_REQUIRE(D >= 1 && D <= KTF_TRAIN_MAX_DIM, "ktf_plda_em_project: D must be in 1 .. %d", KTF_TRAIN_MAX_DIM);
    KTF_REQUIRE((S + TILE - 1) / TILE < 65536, "ktf_plda_em_project: too many speakers");
    hipLaunchKernelGGL(em_project_kernel, dim3((unsigned)ktf_cdiv(D, TILE), (unsigned)((S + TILE - 1) / TILE)), dim3(256), 0,
                       (hipStream_t)stream, mu, S, (int)D, mbar, P, lam, counts, a, b);
    KTF_CHECK_LAUNCH("ktf_plda_em_project");
    return KTF_OK;
}
