// PLDA device code shared by the whole-batch entry points (pool_post.hip: ktf_plda_*, ktf_plda_score_*, and the verification
// entry points with a count per vector, ktf_plda_transform_n_* / ktf_plda_score_n_* / ktf_plda_trials_*) and the per-recording
// dense scoring (plda_dense.hip: ktf_plda_dense_*). One row's transform and one 64 x 64 tile of trial scores are computed by
// the same instructions wherever they are called from, so a recording scored without PCA gets PLDA.call's bits, and a count of
// 1 gets the bits of the entry points without counts.
#pragma once
#include "common.h"

template <typename R>
__device__ __forceinline__ R wsum(R v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <typename R>
__device__ __forceinline__ R rsqrt_(R v);
template <> __device__ __forceinline__ float rsqrt_<float>(float v) { return sqrtf(v); }
template <> __device__ __forceinline__ double rsqrt_<double>(double v) { return sqrt(v); }
template <typename R>
__device__ __forceinline__ R rlog_(R v);
template <> __device__ __forceinline__ float rlog_<float>(float v) { return logf(v); }
template <> __device__ __forceinline__ double rlog_<double>(double v) { return log(v); }

// transformVector (plda.py:163-196) of ONE input vector x (dim) -> out (dim), by a 256-thread workgroup; one wave per output row
// (strided). smraw: sizeof(R) * (2 * dim + 8) bytes of LDS. num: the number of examples the vector averages (Kaldi's
// TransformIvector(num_examples)): the length normalisation divides by psi + 1 / num (1 / 1 is exactly 1: the plain transform's
// bits); the simple length norm ignores it.
template <typename R>
__device__ __forceinline__ void plda_transform_row(const R* __restrict__ x, int dim, const R* __restrict__ A,
                                                   const R* __restrict__ offset, const R* __restrict__ psi, int normalize,
                                                   int simple, R* __restrict__ out, unsigned char* smraw, R num = (R)1) {
    R* xs = reinterpret_cast<R*>(smraw);
    R* ys = xs + dim;
    R* red = ys + dim;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < dim; i += 256) xs[i] = x[i];
    __syncthreads();
    for (int r = wave; r < dim; r += 4) {
        R acc = 0;
        for (int c = lane; c < dim; c += 64) acc += A[(int64_t)r * dim + c] * xs[c];
        acc = wsum<R>(acc);
        if (lane == 0) ys[r] = acc + offset[r];
    }
    __syncthreads();
    R f = 1;
    if (normalize) {
        R part = 0;
        for (int r = threadIdx.x; r < dim; r += 256) {
            const R v = ys[r];
            part += simple ? v * v : v * v / (psi[r] + (R)1 / num);
        }
        part = wsum<R>(part);
        if (lane == 0) red[wave] = part;
        __syncthreads();
        const R tot = red[0] + red[1] + red[2] + red[3];
        f = simple ? rsqrt_<R>((R)dim) / rsqrt_<R>(tot) : rsqrt_<R>((R)dim / tot);
    }
    for (int r = threadIdx.x; r < dim; r += 256) out[r] = ys[r] * f;
}

// The per-dimension terms of logLikelihoodRatio(inputs, num_examples) (plda.py:198-245; Kaldi's PLDA::LogLikelihoodRatio with
// n = num_examples) for a class of n examples: mean = n psi / (n psi + 1) * y_j, var = 1 + psi / (n psi + 1). With n = 1, n * psi is
// psi exactly, so each is the value the count-free tile computes, bit for bit.
template <typename R>
__device__ __forceinline__ R plda_n_mean(R p, R n, R yj) {
    const R np = n * p;
    return np * yj / (np + (R)1);
}
template <typename R>
__device__ __forceinline__ R plda_n_ivar(R p, R n) { return (R)1 / ((R)1 + p / (n * p + (R)1)); }
template <typename R>
__device__ __forceinline__ R plda_n_logvar(R p, R n) { return rlog_<R>((R)1 + p / (n * p + (R)1)); }

// sum_d f(d) by ONE wave, in the bits of the 256-thread reduction of plda_score_tile (thread t adds d = t, t + 256, ...; wsum per
// wave; the four wave sums added in order): lane l forms all four waves' partials itself. Every lane returns the sum.
template <typename R, typename F>
__device__ __forceinline__ R wave_sum_as_256(int dim, int lane, F f) {
    R t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        R s = 0;
        for (int d = 64 * q + lane; d < dim; d += 256) s += f(d);
        t[q] = wsum<R>(s);
    }
    return t[0] + t[1] + t[2] + t[3];
}

// logLikelihoodRatio (plda.py:198-245): the 64 x 64 block of (test i, class j) pairs at (i0, j0), by a 256-thread workgroup,
// sixteen pairs per thread (rows ti + 16 a, classes tj + 16 b), the dimensions staged through LDS 64 at a time.
// Per dimension the reference forms  mean = psi / (psi + 1) * y_j,  var1 = 1 + psi / (psi + 1),  var2 = 1 + psi  and sums
// (y_i - mean)^2 / var1 and y_i^2 / var2. Neither variance depends on the pair and the second sum not on j: a tile computes the
// per-dimension constants k = psi / (psi + 1), 1 / var1, 1 / var2 once (its only divisions), stages the class rows as k * y_j, sums
// y_i^2 / var2 once per row, and a pair costs one subtraction, one multiplication and one fused multiply-add per dimension, on operands
// that four pairs share (it was three fp64 divisions and three LDS reads per pair and dimension: 0.32 ms for 1024 x 1024 trials of
// dimension 128). Rows are padded by one element: the rows a wave reads side by side would otherwise sit in the same LDS banks.
// A score depends on y_i, y_j, psi and dim only, not on where its pair sits in a tile or a matrix.
// PER_CLASS (ktf_plda_score_n_*): class j averages cnt[j] examples, so 1 / var1 and sum log var1 belong to the class: the tile
// stages them per class row (plda_n_*; one wave per class row for the log sum, wave_sum_as_256) next to k_j * y_j, and a pair reads
// its class's weight instead of the shared one. The no-class term keeps var2 = 1 + psi. With every count 1 the scores are those of
// the count-free tile, bit for bit.
// SWAP_STORE (score_norm.hip, the enroll side of a cohort): the block is stored with the class as the row, scores[j * B + i], so
// that a class's B scores lie side by side. The tile is turned round in the LDS the test rows occupied and written out along i;
// every score is the same expression as in the plain store.
#define PLDA_TILE 64
#define PLDA_DC 64
#define PLDA_LDS_BYTES(R) (sizeof(R) * (2 * PLDA_TILE * (PLDA_DC + 1) + 2 * PLDA_DC + 8))        // 67,648 B in fp64
#define PLDA_N_LDS_BYTES(R) (PLDA_LDS_BYTES(R) + sizeof(R) * (PLDA_TILE * (PLDA_DC + 1) + PLDA_TILE))   // 101,440 B in fp64
template <typename R, bool PER_CLASS = false, bool SWAP_STORE = false>
__device__ __forceinline__ void plda_score_tile(const R* __restrict__ y, int64_t B, const R* __restrict__ yc, int64_t Bc,
                                                int dim, const R* __restrict__ psi, R* __restrict__ scores, int64_t i0,
                                                int64_t j0, unsigned char* smraw, const R* __restrict__ cnt = nullptr) {
    // rows i: vectors y (B of them, "test"); columns j: vectors yc (Bc of them, the classes); PLDA.call uses y == yc
    constexpr int LD = PLDA_DC + 1;
    R* yi = reinterpret_cast<R*>(smraw);       // test rows, this chunk of dimensions
    R* yj = yi + PLDA_TILE * LD;               // class rows times k
    R* iv1 = yj + PLDA_TILE * LD;
    R* iv2 = iv1 + PLDA_DC;
    R* red = iv2 + PLDA_DC;                    // 8
    R* yw = red + 8;                           // PER_CLASS: 1 / var1 of each class row, this chunk of dimensions
    R* l1c = yw + PLDA_TILE * LD;              // PER_CLASS: sum log var1 of each class row
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
    // constant terms: sum log(var1) and sum log(var2)
    R l1 = 0, l2 = 0;
    for (int d = threadIdx.x; d < dim; d += 256) {
        const R p = psi[d];
        if constexpr (!PER_CLASS) l1 += rlog_<R>((R)1 + p / (p + (R)1));
        l2 += rlog_<R>((R)1 + p);
    }
    if constexpr (PER_CLASS) {
        const int lane = threadIdx.x & 63;
        for (int r = threadIdx.x >> 6; r < PLDA_TILE; r += 4) {
            const R n = j0 + r < Bc ? cnt[j0 + r] : (R)1;
            const R l = wave_sum_as_256<R>(dim, lane, [&](int d) { return plda_n_logvar<R>(psi[d], n); });
            if (lane == 0) l1c[r] = l;
        }
    }
    l1 = wsum<R>(l1); l2 = wsum<R>(l2);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = l1; red[4 + (threadIdx.x >> 6)] = l2; }
    R a[4][4], c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        c[u] = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) a[u][v] = 0;
    }
    for (int d0 = 0; d0 < dim; d0 += PLDA_DC) {
        const int dc = min(PLDA_DC, dim - d0);
        __syncthreads();                                       // (the previous chunk has been consumed)
        for (int e = threadIdx.x; e < PLDA_TILE * PLDA_DC; e += 256) {
            const int r = e / PLDA_DC, dd = e - r * PLDA_DC;
            R vi = 0, vj = 0, wj = 0;
            if (dd < dc) {
                const R p = psi[d0 + dd];
                if (i0 + r < B) vi = y[(i0 + r) * dim + d0 + dd];
                if (j0 + r < Bc) {
                    if constexpr (PER_CLASS) {
                        const R n = cnt[j0 + r];
                        vj = plda_n_mean<R>(p, n, yc[(j0 + r) * dim + d0 + dd]);
                        wj = plda_n_ivar<R>(p, n);
                    } else {
                        vj = p * yc[(j0 + r) * dim + d0 + dd] / (p + (R)1);
                    }
                }
            }
            yi[r * LD + dd] = vi;
            yj[r * LD + dd] = vj;
            if constexpr (PER_CLASS) yw[r * LD + dd] = wj;
        }
        if (threadIdx.x < PLDA_DC) {
            const R p = threadIdx.x < dc ? psi[d0 + threadIdx.x] : (R)0;
            iv1[threadIdx.x] = (R)1 / ((R)1 + p / (p + (R)1));
            iv2[threadIdx.x] = (R)1 / ((R)1 + p);
        }
        __syncthreads();
        // sum_d y_i^2 / var2: the sixteen threads of a row group take every sixteenth dimension (added up across the lanes at the end)
        for (int dd = tj; dd < dc; dd += 16) {
            const R w2 = iv2[dd];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const R v = yi[(ti + 16 * u) * LD + dd];
                c[u] += v * v * w2;
            }
        }
        for (int dd = 0; dd < dc; ++dd) {
            const R w1 = iv1[dd];
            R vi[4], vj[4], vw[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                vi[u] = yi[(ti + 16 * u) * LD + dd];
                vj[u] = yj[(tj + 16 * u) * LD + dd];
                if constexpr (PER_CLASS) vw[u] = yw[(tj + 16 * u) * LD + dd];
                else vw[u] = w1;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const R diff = vi[u] - vj[v];
                    a[u][v] += diff * diff * vw[v];
                }
        }
    }
    const R logdet1 = red[0] + red[1] + red[2] + red[3];       // (written before the first barrier of the chunk loop; dim >= 1)
    const R logdet2 = red[4] + red[5] + red[6] + red[7];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) c[u] += __shfl_xor(c[u], o, 64);
        const int64_t i = i0 + ti + 16 * u;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t j = j0 + tj + 16 * v;
            const R ld1 = PER_CLASS ? l1c[tj + 16 * v] : logdet1;
            if constexpr (!SWAP_STORE) {
                if (i < B && j < Bc) scores[i * Bc + j] = (R)(-0.5) * (ld1 + a[u][v]) - (R)(-0.5) * (logdet2 + c[u]);
            } else {
                a[u][v] = (R)(-0.5) * (ld1 + a[u][v]) - (R)(-0.5) * (logdet2 + c[u]);
            }
        }
    }
    if constexpr (SWAP_STORE) {
        __syncthreads();                                           // (the last chunk's test rows have been consumed)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int v = 0; v < 4; ++v) yi[(tj + 16 * v) * LD + ti + 16 * u] = a[u][v];
        __syncthreads();
        for (int e = threadIdx.x; e < PLDA_TILE * PLDA_TILE; e += 256) {
            const int jj = e / PLDA_TILE, ii = e - jj * PLDA_TILE;
            if (i0 + ii < B && j0 + jj < Bc) scores[(j0 + jj) * B + i0 + ii] = yi[jj * LD + ii];
        }
    }
}
