// i-vector extraction: Kaldi's `gmm-global-get-post | scale-post | ivector-extract` (sid/extract_ivectors.sh), batched over the
// utterances of one call. Frames of all utterances lie end to end: utterance b owns rows [offsets[b], offsets[b + 1]).
//
//   ivpost_kernel     (a) per frame the n best log-likelihoods of a diagonal UBM, gconst + x.mi - x^2.iv / 2, as one fp32 GEMM of
//                     [x, x^2] (F x 2D) against W (2D x I) with the selection fused: the frames x I matrix never leaves LDS. 32
//                     frames per workgroup, one Gaussian per thread per 256-column tile; after each tile a wave merges its
//                     frames' columns into a sorted list (one list entry per lane) under the list's worst entry as threshold.
//   ivstats_kernel    (b) gamma_i = sum_t p_ti, F_i = sum_t p_ti x_t (fp64), posterior scale and max_count scale applied first.
//                     One workgroup per utterance; wave w owns the Gaussians g = w (mod 4) and each lane the columns d = lane
//                     (mod 64), so every (g, d) sum is taken by one lane in frame order: no atomics, no barriers.
//   ivgemm_kernel     (c) C = A . W in fp64, 64 x 64 tiles, K cut into chunks whose size depends on K alone (never on the batch),
//   ivreduce_kernel       the chunks' partial tiles summed in chunk order: linear = F . sigmaInvM, Q = gamma . U.
//   ivsolve_kernel    (d) per utterance: Q + I unpacked, blocked Cholesky (32-column panels, in the workspace), forward and back
//                     substitution of linear + priorOffset e0, ivector(0) -= priorOffset.
// Every stage is per utterance with a fixed reduction order, so an utterance's bits do not depend on its batch or position.
#include "common.h"

namespace {

constexpr int IVP_FT = 32;          // frames per workgroup of the posterior kernel
constexpr int IVP_GT = 256;         // Gaussians per tile (= threads)
constexpr int IVS_WAVES = 4;        // stats kernel: Gaussian owners per utterance
constexpr int IVS_BATCH = 8;        // owned slots whose loads are in flight together
constexpr int GT = 64;              // GEMM tile (rows and columns)
constexpr int GK = 16;              // GEMM K step
constexpr int64_t GKC = 2048;       // GEMM K chunk: a function of K alone
constexpr int NB = 32;              // Cholesky panel width
constexpr int SOLVE_THREADS = 256;

inline size_t ivpost_lds_bytes(int D, int n) { return (size_t)4 * (2 * D * IVP_FT + IVP_FT * (IVP_GT + 1) + 2 * IVP_FT * n + IVP_FT); }

__host__ __device__ inline int64_t al256(int64_t b) { return (b + 255) & ~(int64_t)255; }

// (v, g) ranks before (w, h): larger log-likelihood first, the lower index on ties
__device__ __forceinline__ bool better(float v, int g, float w, int h) { return v > w || (v == w && g < h); }

__global__ void __launch_bounds__(IVP_GT) ivpost_kernel(const float* __restrict__ x, int64_t F, int D, int64_t ldx,
                                                         const float* __restrict__ W, const float* __restrict__ gconst, int I, int n,
                                                         int ns, float min_post, int* __restrict__ gauss, float* __restrict__ post) {
    // n = min(num_gselect, I) entries kept, ns = num_gselect slots written per frame. Dynamic LDS (ivpost_lds_bytes):
    extern __shared__ __attribute__((aligned(16))) float ivp_lds[];
    float(*xs)[IVP_FT] = reinterpret_cast<float(*)[IVP_FT]>(ivp_lds);                        // [x, x^2] transposed (2D rows):
    float(*ll)[IVP_GT + 1] = reinterpret_cast<float(*)[IVP_GT + 1]>(ivp_lds + 2 * D * IVP_FT); // a float4 is 4 frames of one k
    float* lval = ivp_lds + 2 * D * IVP_FT + IVP_FT * (IVP_GT + 1);                           // (IVP_FT, n) sorted lists
    int* lidx = reinterpret_cast<int*>(lval + IVP_FT * n);
    int* lcnt = lidx + IVP_FT * n;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t f0 = (int64_t)blockIdx.x * IVP_FT;
    const int K = 2 * D;
    for (int e = tid; e < IVP_FT * D; e += IVP_GT) {
        const int f = e / D, d = e - f * D;
        const float v = f0 + f < F ? x[(f0 + f) * ldx + d] : 0.f;
        xs[d][f] = v;
        xs[D + d][f] = v * v;
    }
    if (tid < IVP_FT) lcnt[tid] = 0;
    __syncthreads();
    for (int g0 = 0; g0 < I; g0 += IVP_GT) {
        const int g = g0 + tid;
        if (g < I) {
            float acc[IVP_FT];
            const float gc = gconst[g];
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
#pragma unroll
            for (int f = 0; f < IVP_FT; ++f) ll[f][tid] = acc[f];
        }
        __syncthreads();
        // merge: wave wv owns frames wv, wv + 4, ...; lane j holds list entry j
        for (int f = wv; f < IVP_FT; f += IVP_GT / 64) {
            if (f0 + f >= F) break;
            float val = lane < lcnt[f] ? lval[f * n + lane] : 0.f;
            int idx = lane < lcnt[f] ? lidx[f * n + lane] : 0;
            int cnt = lcnt[f];
            for (int c = 0; c < IVP_GT; c += 64) {
                const int gg = g0 + c + lane;
                const float v = gg < I ? ll[f][c + lane] : 0.f;
                const float tv = __shfl(val, n - 1);
                const int ti = __shfl(idx, n - 1);
                unsigned long long m = __ballot(gg < I && (cnt < n || better(v, gg, tv, ti)));
                while (m) {
                    const int src = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const float cv = __shfl(v, src);
                    const int cg = g0 + c + src;
                    if (cnt == n && !better(cv, cg, __shfl(val, n - 1), __shfl(idx, n - 1))) continue;
                    const int pos = __popcll(__ballot(lane < cnt && better(val, idx, cv, cg)));
                    const float pv = __shfl(val, lane > 0 ? lane - 1 : 0);
                    const int pi = __shfl(idx, lane > 0 ? lane - 1 : 0);
                    if (lane == pos) {
                        val = cv;
                        idx = cg;
                    } else if (lane > pos) {
                        val = pv;
                        idx = pi;
                    }
                    cnt = cnt < n ? cnt + 1 : n;
                }
            }
            if (lane < n) {
                lval[f * n + lane] = val;
                lidx[f * n + lane] = idx;
            }
            if (lane == 0) lcnt[f] = cnt;
        }
        __syncthreads();
    }
    // posteriors: exp(l - max) over the kept set, the smallest dropped while below min_post of the running sum, renormalised
    for (int f = wv; f < IVP_FT; f += IVP_GT / 64) {
        const int64_t t = f0 + f;
        if (t >= F) break;
        const int cnt = lcnt[f];
        const float mx = lval[f * n];
        const float e = lane < cnt ? expf(lval[f * n + lane] - mx) : 0.f;
        int keep = cnt;
        float sum = 0.f;
        for (int j = 0; j < cnt; ++j) sum += __shfl(e, j);
        while (keep > 1) {
            const float last = __shfl(e, keep - 1);
            if (!(last < min_post * sum)) break;
            sum -= last;
            --keep;
        }
        if (lane < ns) {
            gauss[t * ns + lane] = lane < keep ? lidx[f * n + lane] : -1;
            post[t * ns + lane] = lane < keep ? e / sum : 0.f;
        }
    }
}

// frames [t0, t1) of utterance b, clamped to the F rows the caller declared (an inconsistent table reads nothing out of range)
__device__ __forceinline__ void utt_rows(const int* off, int b, int64_t F, int64_t* t0, int64_t* t1) {
    int64_t a = off[b], e = off[b + 1];
    a = a < 0 ? 0 : (a > F ? F : a);
    e = e < a ? a : (e > F ? F : e);
    *t0 = a;
    *t1 = e;
}

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

struct IvLayout {
    int64_t F, gamma, lpart, lin, qpart, q, L, total;
    int nkl, nkq;
};

IvLayout iv_layout(int64_t B, int64_t I, int64_t D, int64_t S) {
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

}  // namespace

extern "C" int ktf_ivector_post_f32(const float* x, int64_t F, int32_t D, int64_t ldx, const float* W, const float* gconst, int32_t I,
                                    int32_t n, float min_post, int32_t* gauss, float* post, void* stream) {
    const char* who = "ktf_ivector_post_f32";
    KTF_REQUIRE(F >= 0 && F <= ((int64_t)1 << 40), "%s: frame count %lld out of range", who, (long long)F);
    KTF_REQUIRE(D >= 1 && D <= KTF_IVECTOR_MAX_FEAT_DIM, "%s: feature dim %d outside 1 .. %d", who, (int)D, KTF_IVECTOR_MAX_FEAT_DIM);
    KTF_REQUIRE(ldx >= D, "%s: ldx %lld < D %d", who, (long long)ldx, (int)D);
    KTF_REQUIRE(I >= 1 && I <= KTF_IVECTOR_MAX_GAUSS, "%s: %d Gaussians outside 1 .. %d", who, (int)I, KTF_IVECTOR_MAX_GAUSS);
    KTF_REQUIRE(n >= 1 && n <= KTF_IVECTOR_MAX_GSELECT, "%s: num_gselect %d outside 1 .. %d", who, (int)n, KTF_IVECTOR_MAX_GSELECT);
    KTF_REQUIRE(min_post >= 0.f && min_post < 1.f, "%s: min_post %g outside [0, 1)", who, (double)min_post);
    if (F == 0) return KTF_OK;
    KTF_REQUIRE(x && W && gconst && gauss && post, "%s: null argument", who);
    const int keep = n < I ? n : I;
    const size_t lds = ivpost_lds_bytes(D, keep);
    KTF_LDS_ONCE(ivpost_lds_bytes(KTF_IVECTOR_MAX_FEAT_DIM, KTF_IVECTOR_MAX_GSELECT), ivpost_kernel);
    hipLaunchKernelGGL(ivpost_kernel, dim3((unsigned)((F + IVP_FT - 1) / IVP_FT)), dim3(IVP_GT), lds, (hipStream_t)stream, x, F, (int)D, ldx,
                       W, gconst, (int)I, keep, (int)n, min_post, gauss, post);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int64_t ktf_ivector_workspace_bytes(int32_t B, int32_t I, int32_t D, int32_t S) {
    const char* who = "ktf_ivector_workspace_bytes";
    KTF_REQUIRE(B >= 1 && B <= 65535, "%s: batch %d outside 1 .. 65535", who, (int)B);
    KTF_REQUIRE(I >= 1 && I <= KTF_IVECTOR_MAX_GAUSS, "%s: %d Gaussians outside 1 .. %d", who, (int)I, KTF_IVECTOR_MAX_GAUSS);
    KTF_REQUIRE(D >= 1 && D <= KTF_IVECTOR_MAX_FEAT_DIM, "%s: feature dim %d outside 1 .. %d", who, (int)D, KTF_IVECTOR_MAX_FEAT_DIM);
    KTF_REQUIRE(S >= 1 && S <= KTF_IVECTOR_MAX_DIM, "%s: i-vector dim %d outside 1 .. %d", who, (int)S, KTF_IVECTOR_MAX_DIM);
    return iv_layout(B, I, D, S).total;
}

extern "C" int ktf_ivector_extract(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* offsets, int32_t B, const int32_t* gauss,
                                   const float* post, int32_t n, float posterior_scale, float acoustic_weight, float max_count,
                                   const double* sigma_inv_M, const double* U, int32_t I, int32_t S, double prior_offset, void* ivectors,
                                   int32_t out_dtype_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_ivector_extract";
    const int64_t need = ktf_ivector_workspace_bytes(B, I, D, S);
    if (need < 0) return (int)need;
    KTF_REQUIRE(F >= 0 && F < ((int64_t)1 << 31), "%s: frame count %lld out of range", who, (long long)F);
    KTF_REQUIRE(ldx >= D, "%s: ldx %lld < D %d", who, (long long)ldx, (int)D);
    KTF_REQUIRE(n >= 1 && n <= KTF_IVECTOR_MAX_GSELECT, "%s: %d slots per frame outside 1 .. %d", who, (int)n, KTF_IVECTOR_MAX_GSELECT);
    KTF_REQUIRE(posterior_scale >= 0.f && acoustic_weight >= 0.f && max_count >= 0.f,
                "%s: posterior_scale, acoustic_weight and max_count must be >= 0", who);
    KTF_REQUIRE(out_dtype_bytes == 4 || out_dtype_bytes == 8, "%s: out_dtype_bytes %d, need 4 or 8", who, (int)out_dtype_bytes);
    KTF_REQUIRE(offsets && sigma_inv_M && U && ivectors && workspace, "%s: null argument", who);
    KTF_REQUIRE(F == 0 || (x && gauss && post), "%s: null frames / posteriors", who);
    KTF_REQUIRE((int64_t)workspace_bytes >= need, "%s: workspace %zu bytes < %lld", who, workspace_bytes, (long long)need);
    KTF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace not 256-byte aligned", who);
    const IvLayout l = iv_layout(B, I, D, S);
    char* ws = (char*)workspace;
    double* Fst = (double*)(ws + l.F);
    double* gam = (double*)(ws + l.gamma);
    double* lin = (double*)(ws + l.lin);
    double* q = (double*)(ws + l.q);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, (size_t)l.lpart, st) != hipSuccess) {  // F and gamma
        ktf_set_error("%s: hipMemsetAsync failed", who);
        return KTF_ELAUNCH;
    }
    hipLaunchKernelGGL(ivstats_kernel, dim3(B), dim3(64 * IVS_WAVES), 0, st, x, F, (int)D, ldx, offsets, gauss, post, (int)n, (int)I,
                       posterior_scale, acoustic_weight, max_count, gam, Fst);
    KTF_CHECK_LAUNCH(who);
    const int64_t P = (int64_t)S * (S + 1) / 2;
    int rc = iv_gemm(who, Fst, (int64_t)I * D, sigma_inv_M, S, (double*)(ws + l.lpart), lin, l.nkl, B, S, (int64_t)I * D, st);
    if (rc != KTF_OK) return rc;
    rc = iv_gemm(who, gam, I, U, P, (double*)(ws + l.qpart), q, l.nkq, B, P, I, st);
    if (rc != KTF_OK) return rc;
    double* L = (double*)(ws + l.L);
    if (out_dtype_bytes == 8)
        hipLaunchKernelGGL(ivsolve_kernel<double>, dim3(B), dim3(SOLVE_THREADS), 0, st, (const double*)q, (const double*)lin, offsets,
                           F, (int)S, prior_offset, L, (double*)ivectors);
    else
        hipLaunchKernelGGL(ivsolve_kernel<float>, dim3(B), dim3(SOLVE_THREADS), 0, st, (const double*)q, (const double*)lin, offsets,
                           F, (int)S, prior_offset, L, (float*)ivectors);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
