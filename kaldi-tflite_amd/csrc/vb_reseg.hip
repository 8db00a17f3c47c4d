// VB-HMM resegmentation of diarization output (Diez / Burget's VB diarization with an i-vector subspace, as Kaldi's
// diarization/VB_resegmentation.sh runs it), batched over the recordings of one call. Frames of all recordings lie end to end:
// recording r owns rows [offsets[r], offsets[r + 1]) of x and blocks [boffsets[r], boffsets[r + 1]) of q / lls; block b of a
// recording covers its frames [b d, (b + 1) d) with d = downsample.
//
//   vb_ll_kernel      the log-likelihoods of ALL Gaussians on the tile of gmm_loglike.h (the bits of ktf_ivector_post_f32), to the
//   vb_select_kernel  workspace (F, I); then one wave per frame: G = logsumexp over all I, p = exp(l - G) stat_scale, and the up to
//                     n candidates p >= sparsity_thr, largest first (n rounds of a wave arg-max after the last one taken).
//   vb_stats_kernel   N_sc, F_sc: one workgroup per (Gaussian, recording) walks that recording's share of the Gaussian's bucket
//                     (the stable bucketing of gmm_bucket.h) in ascending pair order; thread e owns elements (s, column): no atomics.
//   update            lin = F B and Q = N U (iv_gemm), the blocked Cholesky (ivsolve_kernel), C, a and W = C + a a^T (ivcov_kernel),
//   vb_kl_kernel      kl and the triangle weights of g; vb_nt_kernel: C = A B^T on v_mfma_f64_16x16x4_f64 for h = a B^T and
//                     g = W' U^T (k ascending, four per MFMA: the bits depend on the operands alone).
//   vb_lls_kernel     one wave per block: lane (s, part) takes a quarter of the D terms of speaker s, frames then slots in order.
//   fb_*              forward-backward as a chunked scan, KTF_VB_FB_CHUNK blocks per chunk. fb_matrix_kernel: one wave per
//                     chunk, lane j carries column j of the chunk's K x K transfer matrix through the chunk's steps (a step is
//                     diagonal plus rank one: O(K)), renormalised every step with a running log-scale. fb_carry_kernel: one wave
//                     per recording takes the forward vector through the chunks' matrices and the backward vector through their
//                     transposes. fb_post_kernel: one wave per chunk recomputes its alpha and beta in LDS and writes q and the
//                     chunk's share of the sp sums; fb_sp_kernel adds the shares in chunk order.
// Every stage is per recording with a fixed reduction order: a recording's bits do not depend on its batch or position.
#include "ivector_cov.h"
#include "gmm_bucket.h"
#include "gmm_loglike.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int FBC = KTF_VB_FB_CHUNK;
constexpr int FBK = KTF_VB_MAX_SPEAKERS;
constexpr int VSEL_WAVES = 4;
constexpr int VST_ROWS = 16;        // bucket rows staged in LDS per step
constexpr int VST_ACC = (FBK * (KTF_IVECTOR_MAX_FEAT_DIM + 1) + 255) / 256;   // elements (s, column) per thread
constexpr int NT_MT = 2;            // 16-row MFMA tiles per wave
constexpr int NT_NT = 4;            // 16-column MFMA tiles per wave
constexpr int NT_WAVES = 4;         // waves per workgroup, side by side along N: a workgroup owns 32 x 256 of C

// ---------------------------------------------------------------- 1. posteriors
__global__ void __launch_bounds__(IVP_GT) vb_ll_kernel(const float* __restrict__ x, int64_t F, int D, int64_t ldx, const float* __restrict__ W,
                                                       const float* __restrict__ gconst, int I, float* __restrict__ ll) {
    extern __shared__ __attribute__((aligned(16))) float vb_lds[];
    float(*xs)[IVP_FT] = reinterpret_cast<float(*)[IVP_FT]>(vb_lds);
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

// (p, g) ranks before (w, h): the larger posterior first, the lower index on ties
__device__ __forceinline__ bool vb_better(float p, int g, float w, int h) { return p > w || (p == w && g < h); }

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
                if (p >= thr && vb_better(lastp, lastg, p, g) && vb_better(p, g, bp, bg)) {
                    bp = p;
                    bg = g;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float op = __shfl_xor(bp, o, 64);
                const int og = __shfl_xor(bg, o, 64);
                if (vb_better(op, og, bp, bg)) {
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

// ---------------------------------------------------------------- 2. soft statistics
// first index in [lo, hi) of the ascending list `pairs` whose value is >= v
__device__ __forceinline__ int vb_lower_bound(const int* __restrict__ pairs, int lo, int hi, int64_t v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)pairs[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the recording that owns block (or chunk) w of the ascending table `tab` (N + 1 entries): the last r with tab[r] <= w; -1 beyond
__device__ __forceinline__ int vb_owner(const int* __restrict__ tab, int N, int64_t w) {
    if (w < tab[0] || w >= tab[N]) return -1;
    int lo = 0, hi = N;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Nst (N K, I), Fst (N K, I D): every element is written (zero for an empty share of a bucket)
__global__ void __launch_bounds__(256) vb_stats_kernel(const float* __restrict__ x, int64_t F, int D, int64_t ldx, const int* __restrict__ off,
                                                       const int* __restrict__ boff, int64_t TB, int d, const float* __restrict__ post,
                                                       int n, const int* __restrict__ start, const int* __restrict__ pairs,
                                                       const double* __restrict__ means, const double* __restrict__ q, int K, int I,
                                                       double* __restrict__ Nst, double* __restrict__ Fst) {
    __shared__ double xm[VST_ROWS][KTF_IVECTOR_MAX_FEAT_DIM];
    __shared__ double wq[VST_ROWS][FBK];
    const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    int64_t t0, t1;
    utt_rows(off, r, F, &t0, &t1);
    const int lo = vb_lower_bound(pairs, start[c], start[c + 1], t0 * n);
    const int hi = vb_lower_bound(pairs, lo, start[c + 1], t1 * n);
    const int ncol = D + 1, ne = K * ncol;
    double acc[VST_ACC];
    int es[VST_ACC], ec[VST_ACC];
#pragma unroll
    for (int u = 0; u < VST_ACC; ++u) {
        const int e = tid + 256 * u;
        acc[u] = 0.0;
        es[u] = e < ne ? e / ncol : 0;
        ec[u] = e < ne ? e - es[u] * ncol : 0;
    }
    const int64_t qb0 = boff[r];
    for (int rb = lo; rb < hi; rb += VST_ROWS) {
        const int nr = hi - rb < VST_ROWS ? hi - rb : VST_ROWS;
        for (int e = tid; e < nr * D; e += 256) {
            const int rr = e / D, dd = e - rr * D;
            const int64_t t = pairs[rb + rr] / n;
            xm[rr][dd] = (double)x[t * ldx + dd] - means[(int64_t)c * D + dd];
        }
        for (int e = tid; e < nr * K; e += 256) {
            const int rr = e / K, s = e - rr * K;
            const int p = pairs[rb + rr];
            int64_t qb = qb0 + ((int64_t)(p / n) - t0) / d;
            qb = qb < 0 ? 0 : (qb >= TB ? TB - 1 : qb);
            wq[rr][s] = q[qb * K + s] * (double)post[p];
        }
        __syncthreads();
        for (int rr = 0; rr < nr; ++rr) {
#pragma unroll
            for (int u = 0; u < VST_ACC; ++u)
                if (tid + 256 * u < ne) acc[u] = fma(wq[rr][es[u]], ec[u] < D ? xm[rr][ec[u]] : 1.0, acc[u]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < VST_ACC; ++u)
        if (tid + 256 * u < ne) {
            const int64_t b = (int64_t)r * K + es[u];
            if (ec[u] < D) Fst[(b * I + c) * D + ec[u]] = acc[u];
            else Nst[b * I + c] = acc[u];
        }
}

// ---------------------------------------------------------------- 3. speaker update
__global__ void vb_iota_kernel(int* __restrict__ o, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) o[e] = e;
}

// per speaker row b: kl = (R - tr W) / 2 + sum_j log X_jj (X = L^-1), and Wd = the triangle weights of g = tr(U W) / 2:
// half the diagonal, the off-diagonal entries whole (they count twice)
__global__ void __launch_bounds__(COV_THREADS) vb_kl_kernel(const double* __restrict__ Wp, const double* __restrict__ X, int R,
                                                             double* __restrict__ Wd, double* __restrict__ kl) {
    __shared__ double red[COV_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t P = (int64_t)R * (R + 1) / 2;
    const double* w = Wp + (int64_t)b * P;
    double* wd = Wd + (int64_t)b * P;
    const double* Xb = X + (int64_t)b * R * R;
    for (int64_t e = tid; e < P; e += COV_THREADS) wd[e] = w[e];
    double v = 0.0;
    for (int j = tid; j < R; j += COV_THREADS) v += log(Xb[(int64_t)j * R + j]) - 0.5 * w[(int64_t)j * (j + 1) / 2 + j];
    __syncthreads();
    for (int j = tid; j < R; j += COV_THREADS) wd[(int64_t)j * (j + 1) / 2 + j] = 0.5 * w[(int64_t)j * (j + 1) / 2 + j];
    const double tot = block_sum(v, red, tid);
    if (tid == 0) kl[b] = 0.5 * (double)R + tot;
}

// C (M x N, ldc) = A (M x K, lda) . B (N x K, ldb)^T, all fp64 row-major. v_mfma_f64_16x16x4_f64: lane l holds A[row l & 15]
// [k = l >> 4] and B[col l & 15][k = l >> 4]; result reg r of lane l is C[row (l >> 4) + 4 r][col l & 15]. k runs upwards four at a
// time from zero accumulators: the bits of an element depend on its row of A and its row of B alone.
__global__ void __launch_bounds__(64 * NT_WAVES) vb_nt_kernel(const double* __restrict__ A, int64_t lda, const double* __restrict__ Bm,
                                                              int64_t ldb, double* __restrict__ Cm, int64_t ldc, int64_t M, int64_t N,
                                                              int64_t K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.y * (16 * NT_MT);
    const int64_t n0 = ((int64_t)blockIdx.x * NT_WAVES + wave) * (16 * NT_NT);
    if (n0 >= N) return;
    f64x4 acc[NT_MT][NT_NT];
#pragma unroll
    for (int i = 0; i < NT_MT; ++i)
#pragma unroll
        for (int j = 0; j < NT_NT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0;
    for (int64_t k0 = 0; k0 < K; k0 += 4) {
        const int64_t k = k0 + lk;
        double a[NT_MT], bv[NT_NT];
#pragma unroll
        for (int i = 0; i < NT_MT; ++i) {
            const int64_t m = m0 + 16 * i + lc;
            a[i] = (k < K && m < M) ? A[m * lda + k] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < NT_NT; ++j) {
            const int64_t c = n0 + 16 * j + lc;
            bv[j] = (k < K && c < N) ? Bm[c * ldb + k] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < NT_MT; ++i)
#pragma unroll
            for (int j = 0; j < NT_NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bv[j], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NT_MT; ++i)
#pragma unroll
        for (int j = 0; j < NT_NT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + 16 * i + lk + 4 * r, col = n0 + 16 * j + lc;
                if (row < M && col < N) Cm[row * ldc + col] = acc[i][j][r];
            }
}

int vb_nt(const char* who, const double* A, int64_t lda, const double* Bm, int64_t ldb, double* Cm, int64_t ldc, int64_t M, int64_t N,
          int64_t K, hipStream_t st) {
    hipLaunchKernelGGL(vb_nt_kernel, dim3(ktf_cdiv(N, 16 * NT_NT * NT_WAVES), ktf_cdiv(M, 16 * NT_MT)), dim3(64 * NT_WAVES), 0, st, A, lda,
                       Bm, ldb, Cm, ldc, M, N, K);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

struct UpLayout {
    int64_t lpart, lin, qpart, q, L, wd, tail, off, total;
    int nkl, nkq;
};

UpLayout up_layout(int64_t B, int64_t I, int64_t D, int64_t R) {
    UpLayout l;
    const int64_t P = R * (R + 1) / 2;
    l.nkl = (int)((I * D + GKC - 1) / GKC);
    l.nkq = (int)((I + GKC - 1) / GKC);
    int64_t at = 0;
    l.lpart = at; at += al256(l.nkl * B * R * 8);
    l.lin = at;   at += al256(B * R * 8);
    l.qpart = at; at += al256(l.nkq * B * P * 8);
    l.q = at;     at += al256(B * P * 8);
    l.L = at;     at += al256(B * R * R * 8);
    l.wd = at;    at += al256(B * P * 8);
    l.tail = at;  at += al256(B * 2 * 8);
    l.off = at;   at += al256((B + 1) * 4);
    l.total = at;
    return l;
}

// ---------------------------------------------------------------- block log-likelihood
__global__ void __launch_bounds__(256) vb_lls_kernel(const float* __restrict__ x, int64_t F, int D, int64_t ldx, const int* __restrict__ off,
                                                     const int* __restrict__ boff, int N, int64_t TB, int d, const int* __restrict__ gauss,
                                                     const float* __restrict__ post, int n, int I, const double* __restrict__ means,
                                                     const double* __restrict__ h, const double* __restrict__ g, int K,
                                                     double* __restrict__ lls) {
    const int lane = threadIdx.x & 63, s = lane >> 2, part = lane & 3;
    const int64_t gb = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gb >= TB) return;
    const int r = vb_owner(boff, N, gb);
    if (r < 0) return;
    int64_t t0, t1;
    utt_rows(off, r, F, &t0, &t1);
    const int64_t fa = t0 + (gb - boff[r]) * d;
    const int64_t fe = fa + d < t1 ? fa + d : t1;
    const int64_t row = (int64_t)r * K + (s < K ? s : 0);
    double acc = 0.0;
    for (int64_t t = fa; t < fe; ++t)
        for (int sl = 0; sl < n; ++sl) {
            const int c = gauss[t * n + sl];
            if (c < 0 || c >= I) continue;
            const double p = (double)post[t * n + sl];
            double dot = 0.0;
            if (s < K) {
                const double* hb = h + (row * I + c) * D;
                const double* mc = means + (int64_t)c * D;
                for (int dd = part; dd < D; dd += 4) dot = fma((double)x[t * ldx + dd] - mc[dd], hb[dd], dot);
            }
            dot += __shfl_xor(dot, 1, 64);
            dot += __shfl_xor(dot, 2, 64);
            if (s < K) acc += p * (dot - g[row * I + c]);
        }
    if (s < K && part == 0) lls[gb * K + s] = acc;
}

// ---------------------------------------------------------------- forward-backward
struct FbLayout {
    int64_t cstart, M, sc, ain, bout, spc, total;
    int64_t maxch;
};

FbLayout fb_layout(int64_t TB, int64_t N) {
    FbLayout l;
    l.maxch = TB / FBC + N;                      // every recording adds at most one partial chunk
    int64_t at = 0;
    l.cstart = at; at += al256((N + 1) * 4);
    l.M = at;      at += al256(l.maxch * FBK * FBK * 8);
    l.sc = at;     at += al256(l.maxch * FBK * 8);
    l.ain = at;    at += al256(l.maxch * FBK * 8);
    l.bout = at;   at += al256(l.maxch * FBK * 8);
    l.spc = at;    at += al256(l.maxch * FBK * 8);
    l.total = at;
    return l;
}

// cstart[r] = the chunks of the recordings before r (one thread: N is small next to the frames)
__global__ void fb_cstart_kernel(const int* __restrict__ boff, int N, int* __restrict__ cstart) {
    if (blockIdx.x || threadIdx.x) return;
    int run = 0;
    for (int r = 0; r < N; ++r) {
        cstart[r] = run;
        const int tb = boff[r + 1] - boff[r];
        run += tb > 0 ? (tb + FBC - 1) / FBC : 0;
    }
    cstart[N] = run;
}

struct FbChunk {
    int r, k, b0, b1;               // recording, chunk within it, its blocks [b0, b1) within the recording
    int64_t base;                   // the recording's first block
};

__device__ __forceinline__ FbChunk fb_chunk(int w, const int* __restrict__ boff, const int* __restrict__ cstart, int N, int64_t TB) {
    FbChunk c;
    c.r = vb_owner(cstart, N, w);
    c.k = c.b0 = c.b1 = 0;
    c.base = 0;
    if (c.r < 0) return c;
    c.k = w - cstart[c.r];
    c.base = boff[c.r];
    int64_t tb = (int64_t)boff[c.r + 1] - c.base;
    if (c.base < 0 || c.base + tb > TB) {        // an inconsistent table reads nothing out of range
        c.r = -1;
        return c;
    }
    c.b0 = c.k * FBC;
    c.b1 = c.b0 + FBC < tb ? c.b0 + FBC : (int)tb;
    return c;
}

// e[b][i] = exp(lls - the row's max) and mxs[b] = that max for the chunk's blocks, 64 lanes over the blocks
__device__ __forceinline__ void fb_load_e(double (*e)[FBK], double* mxs, const double* __restrict__ lls, const FbChunk& c, int K, int lane) {
    for (int b = c.b0 + lane; b < c.b1; b += 64) {
        const double* row = lls + (c.base + b) * K;
        double mx = row[0];
        for (int i = 1; i < K; ++i) mx = fmax(mx, row[i]);
        for (int i = 0; i < K; ++i) e[b - c.b0][i] = exp(row[i] - mx);
        mxs[b - c.b0] = mx;
    }
}

// one step of the scaled forward recursion on v (K entries): v_i <- e_i (lp v_i + (1 - lp) sp_i sum v); -> (sum before, sum after)
__device__ __forceinline__ void fb_step(double (&v)[FBK], const double* __restrict__ e, const double (&sp)[FBK], int K, double lp, double* s_in,
                                        double* s_out) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < FBK; ++i)
        if (i < K) s += v[i];
    const double t = (1.0 - lp) * s;
    double s2 = 0.0;
#pragma unroll
    for (int i = 0; i < FBK; ++i)
        if (i < K) {
            v[i] = e[i] * (lp * v[i] + t * sp[i]);
            s2 += v[i];
        }
    *s_in = s;
    *s_out = s2;
}

// the sum of lanes 0 .. K - 1 in lane order, the same bits in every lane (all 64 lanes call)
__device__ __forceinline__ double fb_lanes_sum(double v, int K) {
    double s = 0.0;
    for (int j = 0; j < K; ++j) s += __shfl(v, j, 64);
    return s;
}
__device__ __forceinline__ double fb_lanes_max(double v, int K) {
    double m = -INFINITY;
    for (int j = 0; j < K; ++j) m = fmax(m, __shfl(v, j, 64));
    return m;
}

// Mws[w][j][i] = column j of the product of the chunk's steps (blocks max(b0, 1) .. b1 - 1), scaled to sum 1; sc[w][j] = its log-scale
__global__ void __launch_bounds__(64) fb_matrix_kernel(const double* __restrict__ lls, const int* __restrict__ boff, const int* __restrict__ cstart,
                                                       int N, int64_t TB, int K, const double* __restrict__ sp_in, double lp,
                                                       double* __restrict__ Mws, double* __restrict__ sc) {
    __shared__ double e[FBC][FBK];
    __shared__ double mxs[FBC];
    const int w = blockIdx.x, lane = threadIdx.x;
    const FbChunk c = fb_chunk(w, boff, cstart, N, TB);
    if (c.r < 0) return;
    fb_load_e(e, mxs, lls, c, K, lane);
    __syncthreads();
    if (lane >= K) return;
    double v[FBK], sp[FBK];
#pragma unroll
    for (int i = 0; i < FBK; ++i) {
        v[i] = i == lane ? 1.0 : 0.0;
        sp[i] = i < K ? sp_in[(int64_t)c.r * K + i] : 0.0;
    }
    double ls = 0.0;
    for (int b = c.b0 > 1 ? c.b0 : 1; b < c.b1; ++b) {
        double s, s2;
        fb_step(v, e[b - c.b0], sp, K, lp, &s, &s2);
        const double inv = s2 > 0.0 ? 1.0 / s2 : 0.0;
#pragma unroll
        for (int i = 0; i < FBK; ++i) v[i] *= inv;
        ls += (s2 > 0.0 ? log(s2) : -INFINITY) + mxs[b - c.b0];
    }
    double* m = Mws + ((int64_t)w * FBK + lane) * FBK;
#pragma unroll
    for (int i = 0; i < FBK; ++i) m[i] = v[i];
    sc[(int64_t)w * FBK + lane] = ls;
}

// one wave per recording, lane i = speaker i: ain[w] = the scaled alpha entering chunk w (for a recording's first chunk: alpha of
// block 0), bout[w] = the scaled beta of chunk w's last block, tll = log p(blocks)
__global__ void __launch_bounds__(64) fb_carry_kernel(const double* __restrict__ lls, const int* __restrict__ boff, const int* __restrict__ cstart,
                                                      int N, int64_t TB, int64_t maxch, int K, const double* __restrict__ sp_in,
                                                      const double* __restrict__ Mws, const double* __restrict__ sc, double* __restrict__ ain,
                                                      double* __restrict__ bout, double* __restrict__ tll) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const bool on = lane < K;
    const int64_t base = boff[r];
    const int64_t tb = (int64_t)boff[r + 1] - base;
    const int w0 = cstart[r], nch = cstart[r + 1] - w0;
    if (tb <= 0 || base < 0 || base + tb > TB || w0 + nch > maxch) {      // an inconsistent table touches nothing
        if (lane == 0) tll[r] = 0.0;
        return;
    }
    const double* row0 = lls + base * K;
    const double mx0 = fb_lanes_max(on ? row0[lane] : -INFINITY, K);
    double a = on ? sp_in[(int64_t)r * K + lane] * exp(row0[lane] - mx0) : 0.0;
    double s = fb_lanes_sum(a, K);
    a = s > 0.0 ? a / s : 0.0;
    double la = log(s) + mx0;
    for (int k = 0; k < nch; ++k) {
        const int64_t w = w0 + k;
        if (on) ain[w * FBK + lane] = a;
        const double sj = on ? sc[w * FBK + lane] : -INFINITY;
        const double smax = fb_lanes_max(sj, K);
        const double wt = (on && sj > -INFINITY) ? exp(sj - smax) * a : 0.0;
        double o = 0.0;
        for (int j = 0; j < K; ++j) {
            const double wj = __shfl(wt, j, 64);
            if (on) o = fma(Mws[(w * FBK + j) * FBK + lane], wj, o);
        }
        s = fb_lanes_sum(o, K);
        a = s > 0.0 ? o / s : 0.0;
        la += smax + log(s);
    }
    if (lane == 0) tll[r] = la;
    double bt = on ? 1.0 : 0.0;
    for (int k = nch - 1; k >= 0; --k) {
        const int64_t w = w0 + k;
        if (on) bout[w * FBK + lane] = bt;
        if (k == 0) break;
        double dot = 0.0;                        // lane j: column j of the chunk's matrix against beta
        for (int i = 0; i < K; ++i) {
            const double bi = __shfl(bt, i, 64);
            if (on) dot = fma(Mws[(w * FBK + lane) * FBK + i], bi, dot);
        }
        const double sj = on ? sc[w * FBK + lane] : -INFINITY;
        const double smax = fb_lanes_max(sj, K);
        const double o = (on && sj > -INFINITY) ? exp(sj - smax) * dot : 0.0;
        s = fb_lanes_sum(o, K);
        bt = s > 0.0 ? o / s : 0.0;
    }
}

// one wave per chunk: alpha forwards from ain and beta backwards from bout, both in LDS; then q and the chunk's share of the sp sums
__global__ void __launch_bounds__(64) fb_post_kernel(const double* __restrict__ lls, const int* __restrict__ boff, const int* __restrict__ cstart,
                                                     int N, int64_t TB, int K, const double* __restrict__ sp_in, double lp,
                                                     const double* __restrict__ ain, const double* __restrict__ bout, double* __restrict__ q,
                                                     double* __restrict__ spc) {
    __shared__ double e[FBC][FBK];               // exp(lls - max); after the backward walk e . beta
    __shared__ double ah[FBC][FBK];              // scaled alpha; after the backward walk alpha . beta
    __shared__ double cb[FBC];                   // (1 - lp) sum(alpha_{b-1}) / the step's normaliser; mxs while e is built
    __shared__ double tot[FBC];
    const int w = blockIdx.x, lane = threadIdx.x;
    const FbChunk c = fb_chunk(w, boff, cstart, N, TB);
    if (c.r < 0) return;
    fb_load_e(e, cb, lls, c, K, lane);
    __syncthreads();
    double v[FBK], sp[FBK];
#pragma unroll
    for (int i = 0; i < FBK; ++i) {
        v[i] = i < K ? ain[(int64_t)w * FBK + i] : 0.0;
        sp[i] = i < K ? sp_in[(int64_t)c.r * K + i] : 0.0;
    }
    const int nb = c.b1 - c.b0;
    const int s0 = c.b0 > 1 ? c.b0 : 1;
    // every lane walks the same recursion; lane 0 keeps the rows
    if (c.b0 == 0 && lane == 0) {
#pragma unroll
        for (int i = 0; i < FBK; ++i) ah[0][i] = v[i];
        cb[0] = 0.0;
    }
    for (int b = s0; b < c.b1; ++b) {
        double s, s2;
        fb_step(v, e[b - c.b0], sp, K, lp, &s, &s2);
        const double inv = s2 > 0.0 ? 1.0 / s2 : 0.0;
#pragma unroll
        for (int i = 0; i < FBK; ++i) v[i] *= inv;
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < FBK; ++i) ah[b - c.b0][i] = v[i];
            cb[b - c.b0] = (1.0 - lp) * s * inv;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < FBK; ++i) v[i] = i < K ? bout[(int64_t)w * FBK + i] : 0.0;
    for (int b = c.b1 - 1; b >= c.b0; --b) {
        double eb[FBK];
        double dot = 0.0, at = 0.0;
#pragma unroll
        for (int i = 0; i < FBK; ++i) {
            eb[i] = i < K ? e[b - c.b0][i] * v[i] : 0.0;
            dot = fma(sp[i], eb[i], dot);
            at += i < K ? ah[b - c.b0][i] * v[i] : 0.0;
        }
        __syncthreads();                         // every lane has read row b before lane 0 overwrites it
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < FBK; ++i) {
                ah[b - c.b0][i] *= v[i];
                e[b - c.b0][i] = eb[i];
            }
            tot[b - c.b0] = at;
        }
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < FBK; ++i) {
            v[i] = i < K ? lp * eb[i] + (1.0 - lp) * dot : 0.0;
            s += v[i];
        }
        const double inv = s > 0.0 ? 1.0 / s : 0.0;
#pragma unroll
        for (int i = 0; i < FBK; ++i) v[i] *= inv;
    }
    __syncthreads();
    for (int idx = lane; idx < nb * K; idx += 64) {
        const int b = idx / K, j = idx - b * K;
        q[(c.base + c.b0 + b) * K + j] = ah[b][j] / tot[b];
    }
    if (lane < K) {
        const double spj = sp_in[(int64_t)c.r * K + lane];
        double acc = c.b0 == 0 ? ah[0][lane] / tot[0] : 0.0;
        for (int b = s0; b < c.b1; ++b) acc += cb[b - c.b0] * spj * e[b - c.b0][lane] / tot[b - c.b0];
        spc[(int64_t)w * FBK + lane] = acc;
    }
}

// sp_out (N, K) = the chunks' shares added in chunk order, normalised; a recording without blocks keeps its sp
__global__ void __launch_bounds__(64) fb_sp_kernel(const int* __restrict__ cstart, int64_t maxch, int K, const double* __restrict__ sp_in,
                                                   const double* __restrict__ spc, double* __restrict__ sp_out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const bool on = lane < K;
    const int w0 = cstart[r], nch = w0 + (cstart[r + 1] - w0) <= maxch ? cstart[r + 1] - w0 : 0;
    double acc = 0.0;
    if (on)
        for (int k = 0; k < nch; ++k) acc += spc[(int64_t)(w0 + k) * FBK + lane];
    const double s = fb_lanes_sum(on ? acc : 0.0, K);
    if (on) sp_out[(int64_t)r * K + lane] = (nch > 0 && s > 0.0) ? acc / s : sp_in[(int64_t)r * K + lane];
}

// the sum / max over the 16 lanes of a speaker group by a butterfly: the same bits in every lane (lanes beyond K hold 0 / -inf)
__device__ __forceinline__ double fb_group_sum(double v) {
#pragma unroll
    for (int o = FBK / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double fb_group_max(double v) {
#pragma unroll
    for (int o = FBK / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// The serial form, for tools/bench_vb.py to time the chunked scan against (not on the product's path): one wave per recording,
// lane i = speaker i, walks all the recording's blocks forwards and then backwards. alpha (TB, FBK) and cb (TB) in the workspace
// hold the scaled forward vectors and (1 - lp) sum(alpha_{b-1}) / the step's normaliser; no LDS staging.
__global__ void __launch_bounds__(64) fb_serial_kernel(const double* __restrict__ lls, const int* __restrict__ boff, int64_t TB, int K,
                                                       const double* __restrict__ sp_in, double lp, double* __restrict__ alpha,
                                                       double* __restrict__ cbw, double* __restrict__ q, double* __restrict__ sp_out,
                                                       double* __restrict__ tll) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const bool on = lane < K;
    const int64_t base = boff[r];
    const int64_t tb = (int64_t)boff[r + 1] - base;
    const double spi = on ? sp_in[(int64_t)r * K + lane] : 0.0;
    if (tb <= 0 || base < 0 || base + tb > TB) {                           // no blocks (or an inconsistent table): sp stays
        if (lane == 0) tll[r] = 0.0;
        if (on) sp_out[(int64_t)r * K + lane] = spi;
        return;
    }
    double l = on ? lls[base * K + lane] : -INFINITY;
    double mx = fb_group_max(l);
    double a = on ? spi * exp(l - mx) : 0.0;
    double s = fb_group_sum(a);
    a = s > 0.0 ? a / s : 0.0;
    double la = log(s) + mx;
    if (lane < FBK) alpha[base * FBK + lane] = a;
    if (lane == 0) cbw[base] = 0.0;
    for (int64_t b = 1; b < tb; ++b) {
        l = on ? lls[(base + b) * K + lane] : -INFINITY;
        mx = fb_group_max(l);
        s = fb_group_sum(a);
        const double v = on ? exp(l - mx) * (lp * a + (1.0 - lp) * s * spi) : 0.0;
        const double s2 = fb_group_sum(v);
        const double inv = s2 > 0.0 ? 1.0 / s2 : 0.0;
        a = v * inv;
        la += (s2 > 0.0 ? log(s2) : -INFINITY) + mx;
        if (lane < FBK) alpha[(base + b) * FBK + lane] = a;
        if (lane == 0) cbw[base + b] = (1.0 - lp) * s * inv;
    }
    if (lane == 0) tll[r] = la;
    __syncthreads();                             // lane 0's cbw are read by every lane below
    double bt = on ? 1.0 : 0.0, acc = 0.0;
    for (int64_t b = tb - 1; b >= 0; --b) {
        l = on ? lls[(base + b) * K + lane] : -INFINITY;
        mx = fb_group_max(l);
        const double eb = on ? exp(l - mx) * bt : 0.0;
        const double ab = on ? alpha[(base + b) * FBK + lane] * bt : 0.0;
        const double at = fb_group_sum(ab);
        const double qv = ab / at;
        if (on) q[(base + b) * K + lane] = qv;
        acc += b == 0 ? qv : cbw[base + b] * spi * eb / at;
        const double dot = fb_group_sum(spi * eb);
        const double o = on ? lp * eb + (1.0 - lp) * dot : 0.0;
        s = fb_group_sum(o);
        bt = s > 0.0 ? o / s : 0.0;
    }
    s = fb_group_sum(on ? acc : 0.0);
    if (on) sp_out[(int64_t)r * K + lane] = s > 0.0 ? acc / s : spi;
}

// ---------------------------------------------------------------- the bound
// gsum[r] = sum_t G_t over recording r's frames in fp64: thread-strided from the recording's first frame, then a fixed tree, so the
// bits depend on the recording's values alone, not on where it lies in the packed vector
__global__ void __launch_bounds__(256) vb_gsum_kernel(const float* __restrict__ loglike, const int* __restrict__ off, int64_t F,
                                                      double* __restrict__ gsum) {
    __shared__ double part[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    int64_t t0, t1;
    utt_rows(off, r, F, &t0, &t1);
    double v = 0.0;
    for (int64_t t = t0 + tid; t < t1; t += 256) v += (double)loglike[t];
    part[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) part[tid] += part[tid + s];
        __syncthreads();
    }
    if (tid == 0) gsum[r] = part[0];
}

// bound[r] = stat_scale gsum[r] + tll[r] + sum_s kl[r K + s], s ascending
__global__ void vb_bound_kernel(const double* __restrict__ gsum, const double* __restrict__ tll, const double* __restrict__ kl, int N, int K,
                                double stat_scale, double* __restrict__ bound) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += kl[(int64_t)r * K + k];
    bound[r] = stat_scale * gsum[r] + tll[r] + s;
}

int vb_check_tables(const char* who, int64_t F, int32_t D, int64_t ldx, int32_t N, int64_t TB, int32_t downsample, int32_t K) {
    KTF_REQUIRE(F >= 0 && F < ((int64_t)1 << 31), "%s: frame count %lld out of range", who, (long long)F);
    KTF_REQUIRE(D >= 1 && D <= KTF_IVECTOR_MAX_FEAT_DIM, "%s: feature dim %d outside 1 .. %d", who, (int)D, KTF_IVECTOR_MAX_FEAT_DIM);
    KTF_REQUIRE(ldx >= D, "%s: ldx %lld < D %d", who, (long long)ldx, (int)D);
    KTF_REQUIRE(N >= 1 && N <= 65535, "%s: %d recordings outside 1 .. 65535", who, (int)N);
    KTF_REQUIRE(TB >= 0 && TB <= F, "%s: %lld blocks for %lld frames", who, (long long)TB, (long long)F);
    KTF_REQUIRE(downsample >= 1, "%s: downsample %d < 1", who, (int)downsample);
    KTF_REQUIRE(K >= 1 && K <= KTF_VB_MAX_SPEAKERS, "%s: %d speakers outside 1 .. %d", who, (int)K, KTF_VB_MAX_SPEAKERS);
    return KTF_OK;
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
    KTF_REQUIRE((int64_t)workspace_bytes >= need, "%s: workspace %zu bytes < %lld", who, workspace_bytes, (long long)need);
    KTF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace not 256-byte aligned", who);
    if (F == 0) return KTF_OK;
    hipStream_t st = (hipStream_t)stream;
    float* ll = (float*)workspace;
    hipLaunchKernelGGL(vb_ll_kernel, dim3((unsigned)((F + IVP_FT - 1) / IVP_FT)), dim3(IVP_GT), (size_t)4 * 2 * D * IVP_FT, st, x, F, (int)D, ldx,
                       W, gconst, (int)I, ll);
    KTF_CHECK_LAUNCH(who);
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
    KTF_REQUIRE((int64_t)workspace_bytes >= need, "%s: workspace %zu bytes < %lld", who, workspace_bytes, (long long)need);
    KTF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace not 256-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    if (F == 0) {
        if (hipMemsetAsync(start, 0, (size_t)(I + 1) * 4, st) != hipSuccess) {
            ktf_set_error("%s: hipMemsetAsync failed", who);
            return KTF_ELAUNCH;
        }
        return KTF_OK;
    }
    char* ws = (char*)workspace;
    const SecLayout l = sec_layout(F, I, n, true);
    const int rc = sec_bucket(who, gauss, F * n, (int)I, l, ws, st);
    if (rc != KTF_OK) return rc;
    if (hipMemcpyAsync(start, ws + l.start, (size_t)(I + 1) * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(pairs, ws + l.pairs, (size_t)(F * n) * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
        ktf_set_error("%s: hipMemcpyAsync failed", who);
        return KTF_ELAUNCH;
    }
    return KTF_OK;
}

extern "C" int ktf_vb_speaker_stats(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* offsets, const int32_t* boffsets, int32_t N,
                                    int64_t TB, int32_t downsample, const float* post, int32_t n, const int32_t* start, const int32_t* pairs,
                                    int32_t I, const double* means, const double* q, int32_t K, double* Nst, double* Fst, void* stream) {
    const char* who = "ktf_vb_speaker_stats";
    int rc = vb_check_tables(who, F, D, ldx, N, TB, downsample, K);
    if (rc != KTF_OK) return rc;
    if ((rc = bucket_check_pairs(who, F, I, n)) != KTF_OK) return rc;
    KTF_REQUIRE(offsets && boffsets && start && means && Nst && Fst, "%s: null argument", who);
    KTF_REQUIRE(F == 0 || (x && post && pairs && q), "%s: null frames / posteriors / q", who);
    if (F == 0 || TB == 0) {
        hipStream_t st0 = (hipStream_t)stream;
        if (hipMemsetAsync(Nst, 0, (size_t)N * K * I * 8, st0) != hipSuccess || hipMemsetAsync(Fst, 0, (size_t)N * K * I * D * 8, st0) != hipSuccess) {
            ktf_set_error("%s: hipMemsetAsync failed", who);
            return KTF_ELAUNCH;
        }
        return KTF_OK;
    }
    hipLaunchKernelGGL(vb_stats_kernel, dim3(I, N), dim3(256), 0, (hipStream_t)stream, x, F, (int)D, ldx, offsets, boffsets, TB, (int)downsample,
                       post, (int)n, start, pairs, means, q, (int)K, (int)I, Nst, Fst);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int64_t ktf_vb_update_workspace_bytes(int32_t B, int32_t I, int32_t D, int32_t R) {
    const char* who = "ktf_vb_update_workspace_bytes";
    KTF_REQUIRE(B >= 1 && B <= 65535, "%s: %d speaker rows outside 1 .. 65535", who, (int)B);
    KTF_REQUIRE(I >= 1 && I <= KTF_IVECTOR_MAX_GAUSS, "%s: %d Gaussians outside 1 .. %d", who, (int)I, KTF_IVECTOR_MAX_GAUSS);
    KTF_REQUIRE(D >= 1 && D <= KTF_IVECTOR_MAX_FEAT_DIM, "%s: feature dim %d outside 1 .. %d", who, (int)D, KTF_IVECTOR_MAX_FEAT_DIM);
    KTF_REQUIRE(R >= 1 && R <= KTF_IVECTOR_MAX_DIM, "%s: i-vector dim %d outside 1 .. %d", who, (int)R, KTF_IVECTOR_MAX_DIM);
    return up_layout(B, I, D, R).total;
}

extern "C" int ktf_vb_speaker_update(const double* Nst, const double* Fst, int32_t B, int32_t I, int32_t D, int32_t R, const double* Bm,
                                     const double* U, double* a, double* Wp, double* kl, double* h, double* g, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    const char* who = "ktf_vb_speaker_update";
    const int64_t need = ktf_vb_update_workspace_bytes(B, I, D, R);
    if (need < 0) return (int)need;
    KTF_REQUIRE(Nst && Fst && Bm && U && a && Wp && kl && h && g && workspace, "%s: null argument", who);
    KTF_REQUIRE((int64_t)workspace_bytes >= need, "%s: workspace %zu bytes < %lld", who, workspace_bytes, (long long)need);
    KTF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace not 256-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const UpLayout l = up_layout(B, I, D, R);
    const int64_t P = (int64_t)R * (R + 1) / 2, ID = (int64_t)I * D;
    double* lin = (double*)(ws + l.lin);
    double* Q = (double*)(ws + l.q);
    double* L = (double*)(ws + l.L);
    double* Wd = (double*)(ws + l.wd);
    double* tail = (double*)(ws + l.tail);
    int* off = (int*)(ws + l.off);
    hipLaunchKernelGGL(vb_iota_kernel, dim3(ktf_cdiv(B + 1, 256)), dim3(256), 0, st, off, (int)B + 1);   // every row "has frames"
    KTF_CHECK_LAUNCH(who);
    int rc = iv_gemm(who, Fst, ID, Bm, R, (double*)(ws + l.lpart), lin, l.nkl, B, R, ID, st);
    if (rc != KTF_OK) return rc;
    if ((rc = iv_gemm(who, Nst, I, U, P, (double*)(ws + l.qpart), Q, l.nkq, B, P, I, st)) != KTF_OK) return rc;
    hipLaunchKernelGGL(ivsolve_kernel<double>, dim3(B), dim3(SOLVE_THREADS), 0, st, (const double*)Q, (const double*)lin, (const int*)off,
                       (int64_t)B, (int)R, 0.0, L, a);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(ivcov_kernel, dim3(B), dim3(COV_THREADS), 0, st, (const double*)lin, (const int*)off, (int64_t)B, (int)R, 0.0, L, Wp, a,
                       tail);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(vb_kl_kernel, dim3(B), dim3(COV_THREADS), 0, st, (const double*)Wp, (const double*)L, (int)R, Wd, kl);
    KTF_CHECK_LAUNCH(who);
    if ((rc = vb_nt(who, a, R, Bm, R, h, ID, B, ID, R, st)) != KTF_OK) return rc;                 // h_sc = (B rows of c) a_s
    return vb_nt(who, Wd, P, U, P, g, I, B, I, P, st);                                            // g_sc = tr(U_c W_s) / 2
}

extern "C" int ktf_vb_block_loglike(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* offsets, const int32_t* boffsets, int32_t N,
                                    int64_t TB, int32_t downsample, const int32_t* gauss, const float* post, int32_t n, int32_t I,
                                    const double* means, const double* h, const double* g, int32_t K, double* lls, void* stream) {
    const char* who = "ktf_vb_block_loglike";
    int rc = vb_check_tables(who, F, D, ldx, N, TB, downsample, K);
    if (rc != KTF_OK) return rc;
    if ((rc = bucket_check_pairs(who, F, I, n)) != KTF_OK) return rc;
    KTF_REQUIRE(offsets && boffsets && means && h && g, "%s: null argument", who);
    KTF_REQUIRE(TB == 0 || (x && gauss && post && lls), "%s: null frames / posteriors / output", who);
    if (TB == 0) return KTF_OK;
    hipLaunchKernelGGL(vb_lls_kernel, dim3((unsigned)((TB + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, F, (int)D, ldx, offsets, boffsets, (int)N,
                       TB, (int)downsample, gauss, post, (int)n, (int)I, means, h, g, (int)K, lls);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int64_t ktf_vb_fb_workspace_bytes(int64_t TB, int32_t N) {
    const char* who = "ktf_vb_fb_workspace_bytes";
    KTF_REQUIRE(TB >= 0 && TB < ((int64_t)1 << 31), "%s: block count %lld out of range", who, (long long)TB);
    KTF_REQUIRE(N >= 1 && N <= 65535, "%s: %d recordings outside 1 .. 65535", who, (int)N);
    return fb_layout(TB, N).total;
}

extern "C" int ktf_vb_forward_backward(const double* lls, const int32_t* boffsets, int32_t N, int64_t TB, int32_t K, const double* sp,
                                       double loop_prob, double* q, double* sp_out, double* tll, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    const char* who = "ktf_vb_forward_backward";
    const int64_t need = ktf_vb_fb_workspace_bytes(TB, N);
    if (need < 0) return (int)need;
    KTF_REQUIRE(K >= 1 && K <= KTF_VB_MAX_SPEAKERS, "%s: %d speakers outside 1 .. %d", who, (int)K, KTF_VB_MAX_SPEAKERS);
    KTF_REQUIRE(loop_prob >= 0.0 && loop_prob <= 1.0, "%s: loop_prob %g outside [0, 1]", who, loop_prob);
    KTF_REQUIRE(boffsets && sp && sp_out && tll && workspace, "%s: null argument", who);
    KTF_REQUIRE(TB == 0 || (lls && q), "%s: null lls / q", who);
    KTF_REQUIRE((int64_t)workspace_bytes >= need, "%s: workspace %zu bytes < %lld", who, workspace_bytes, (long long)need);
    KTF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace not 256-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const FbLayout l = fb_layout(TB, N);
    int* cstart = (int*)(ws + l.cstart);
    double* Mws = (double*)(ws + l.M);
    double* sc = (double*)(ws + l.sc);
    double* ain = (double*)(ws + l.ain);
    double* bout = (double*)(ws + l.bout);
    double* spc = (double*)(ws + l.spc);
    hipLaunchKernelGGL(fb_cstart_kernel, dim3(1), dim3(64), 0, st, boffsets, (int)N, cstart);
    KTF_CHECK_LAUNCH(who);
    const unsigned nch = (unsigned)l.maxch;
    hipLaunchKernelGGL(fb_matrix_kernel, dim3(nch), dim3(64), 0, st, lls, boffsets, (const int*)cstart, (int)N, TB, (int)K, sp, loop_prob, Mws, sc);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(fb_carry_kernel, dim3(N), dim3(64), 0, st, lls, boffsets, (const int*)cstart, (int)N, TB, l.maxch, (int)K, sp,
                       (const double*)Mws, (const double*)sc, ain, bout, tll);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(fb_post_kernel, dim3(nch), dim3(64), 0, st, lls, boffsets, (const int*)cstart, (int)N, TB, (int)K, sp, loop_prob,
                       (const double*)ain, (const double*)bout, q, spc);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(fb_sp_kernel, dim3(N), dim3(64), 0, st, (const int*)cstart, l.maxch, (int)K, sp, (const double*)spc, sp_out);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int64_t ktf_vb_fb_serial_workspace_bytes(int64_t TB, int32_t N) {
    const char* who = "ktf_vb_fb_serial_workspace_bytes";
    KTF_REQUIRE(TB >= 0 && TB < ((int64_t)1 << 31), "%s: block count %lld out of range", who, (long long)TB);
    KTF_REQUIRE(N >= 1 && N <= 65535, "%s: %d recordings outside 1 .. 65535", who, (int)N);
    return al256((TB > 0 ? TB : 1) * FBK * 8) + al256((TB > 0 ? TB : 1) * 8);
}

extern "C" int ktf_vb_forward_backward_serial(const double* lls, const int32_t* boffsets, int32_t N, int64_t TB, int32_t K, const double* sp,
                                              double loop_prob, double* q, double* sp_out, double* tll, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    const char* who = "ktf_vb_forward_backward_serial";
    const int64_t need = ktf_vb_fb_serial_workspace_bytes(TB, N);
    if (need < 0) return (int)need;
    KTF_REQUIRE(K >= 1 && K <= KTF_VB_MAX_SPEAKERS, "%s: %d speakers outside 1 .. %d", who, (int)K, KTF_VB_MAX_SPEAKERS);
    KTF_REQUIRE(loop_prob >= 0.0 && loop_prob <= 1.0, "%s: loop_prob %g outside [0, 1]", who, loop_prob);
    KTF_REQUIRE(boffsets && sp && sp_out && tll && workspace, "%s: null argument", who);
    KTF_REQUIRE(TB == 0 || (lls && q), "%s: null lls / q", who);
    KTF_REQUIRE((int64_t)workspace_bytes >= need, "%s: workspace %zu bytes < %lld", who, workspace_bytes, (long long)need);
    KTF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace not 256-byte aligned", who);
    char* ws = (char*)workspace;
    double* alpha = (double*)ws;
    double* cbw = (double*)(ws + al256((TB > 0 ? TB : 1) * FBK * 8));
    hipLaunchKernelGGL(fb_serial_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, lls, boffsets, TB, (int)K, sp, loop_prob, alpha, cbw, q, sp_out,
                       tll);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_vb_loglike_sums(const float* loglike, const int32_t* offsets, int32_t N, int64_t F, double* gsum, void* stream) {
    const char* who = "ktf_vb_loglike_sums";
    KTF_REQUIRE(F >= 0 && F < ((int64_t)1 << 31), "%s: frame count %lld out of range", who, (long long)F);
    KTF_REQUIRE(N >= 1 && N <= 65535, "%s: %d recordings outside 1 .. 65535", who, (int)N);
    KTF_REQUIRE(offsets && gsum && (F == 0 || loglike), "%s: null argument", who);
    hipLaunchKernelGGL(vb_gsum_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, loglike, offsets, F, gsum);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_vb_bound(const double* gsum, const double* tll, const double* kl, int32_t N, int32_t K, double stat_scale, double* bound,
                            void* stream) {
    const char* who = "ktf_vb_bound";
    KTF_REQUIRE(N >= 1 && N <= 65535, "%s: %d recordings outside 1 .. 65535", who, (int)N);
    KTF_REQUIRE(K >= 1 && K <= KTF_VB_MAX_SPEAKERS, "%s: %d speakers outside 1 .. %d", who, (int)K, KTF_VB_MAX_SPEAKERS);
    KTF_REQUIRE(gsum && tll && kl && bound, "%s: null argument", who);
    hipLaunchKernelGGL(vb_bound_kernel, dim3(ktf_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, gsum, tll, kl, (int)N, (int)K, stat_scale, bound);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
