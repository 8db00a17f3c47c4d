// The classification head's loss in training: one family of kernels for include/ktf_loss.h (rules cited by number or as N1, N2) and
// include/ktf_head.h (rules H1 - H7: sub-centres, an inter-top-k penalty and label smoothing).
//   ktf_loss_row_inv_norm[_backward]             loss_inv_norm_kernel / loss_inv_norm_bwd_kernel: a wave per row
//   ktf_loss_margin_softmax_forward / ktf_head_forward     loss_forward_kernel<false / true>: a workgroup per row -- the selection of H2
//                                       (full only), then two passes over the row (maximum, then the sum of exponentials)
//   ktf_loss_margin_softmax_backward / ktf_head_backward   loss_backward_kernel<false / true>: a workgroup per (block of rows, chunk of
//                                       classes), one pass that writes dz and the partial sums of dinv_x and dinv_w ->
//                                       loss_finalize_kernel adds them (cosine head only)
// Two instantiations of one body. The plain one (FULL = false) has K = 1 as a constant, no selection, no `hard`, `member` or `sub_y`, no
// smoothing sum, one running sum and one store per class: 8 waves / SIMD. The full one (FULL = true) is what ktf_head.h describes, with a
// run-time K: 4 waves / SIMD, and 1.35 to 1.5 times the plain one's time with every switch off, which is why ktf_loss_* always launches
// the plain one and ktf_head_* always the full one. What differs stands under `if constexpr (FULL)` or `FULL ? :`. The shape of the
// forward class loop is one of those differences (loss_for_classes): in the full one's blocks of LOSS_UNROLL classes, with the centre
// index as the outer loop, every class's loads stand behind the class's own bounds check, and the plain instantiation compiled that way
// no longer issues the eight loads of an unrolled step together as its strided `#pragma unroll 4` loop does, so it keeps that loop. Both
// shapes visit a thread's classes in the same order, and with K = 1, topk = 0 and smoothing = 0 every operation on a value is the same
// in both instantiations in the same order, which is what makes their outputs equal bit for bit (H5).
// One access pattern for every alignment (rule 8, H5): a lane reads and writes one float at a time; a thread owns a class and reads its K
// centres one after the other, so a wave covers 64 * K contiguous floats per step. Every sum and every output value is fp64 arithmetic
// rounded once; the fp64 exponential per class is what these kernels spend their time on.
#include "common.h"
#include "../../include/ktf_loss.h"
#include "../../include/ktf_head.h"

static_assert(KTF_HEAD_SLOT_ROWS == KTF_LOSS_SLOT_ROWS && KTF_HEAD_CHUNK_CLASSES == KTF_LOSS_CHUNK_COLS,
              "both headers describe one set of kernels: one slot size, one chunk size");

// every fp64 operation is rounded on its own: no contraction into fma
#pragma clang fp contract(off)

namespace {

constexpr int LOSS_THREADS = KTF_LOSS_CHUNK_COLS;
constexpr int LOSS_WAVES = LOSS_THREADS / 64;
constexpr int LOSS_ROWS = KTF_LOSS_SLOT_ROWS;
constexpr int LOSS_KMAX = KTF_HEAD_MAX_CENTERS;
constexpr int LOSS_NORM_ROWS = 4;       // inverse norms: rows (waves) per workgroup
constexpr int LOSS_UNROLL = 4;          // full forward: classes a thread has in flight
constexpr int LOSS_CAND = 4;            // full forward: classes a thread holds for the selection of H2
constexpr int LOSS_FIN_BATCH = 8;       // finalize: partial sums a thread has in flight

struct LossParams {
    const float* z;
    int64_t ldz;
    int B, N, K;
    const int32_t* labels;
    const float* inv_x;     // both NULL: plain head
    const float* inv_w;
    int kind;
    double margin, scale, cm, sm, msm;   // cos m, sin m, m * sin m (rule 3)
    int topk, width;                     // width = max(topk, 1): the row length of `hard`
    double penalty, eps, inv_n;          // smoothing, 1 / (double)N
};

// the butterfly of rules N1 and 7: every lane ends with the same bits
__device__ __forceinline__ double loss_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// rule 1
__device__ __forceinline__ double loss_cosine(const LossParams& p, float zf, double ix, double iw) {
    return p.inv_x ? ((double)zf * ix) * iw : (double)zf;
}

__device__ __forceinline__ double loss_psi(const LossParams& p, double c) {
    if (p.kind == KTF_LOSS_AM) return c - p.margin;
    if (p.kind == KTF_LOSS_AAM) {
        if (c > -p.cm) {
            double s2 = 1.0 - c * c;
            s2 = s2 > KTF_LOSS_SIN2_FLOOR ? s2 : KTF_LOSS_SIN2_FLOOR;
            return c * p.cm - sqrt(s2) * p.sm;
        }
        return c - p.msm;
    }
    return c;
}

__device__ __forceinline__ double loss_dpsi(const LossParams& p, double c) {
    if (p.kind == KTF_LOSS_AAM && c > -p.cm) {
        const double s2 = 1.0 - c * c;
        return s2 > KTF_LOSS_SIN2_FLOOR ? p.cm + (p.sm * c) / sqrt(s2) : p.cm;
    }
    return 1.0;
}

// ------------------------------------------------------------------------------------ inverse norms
__device__ __forceinline__ double loss_row_sumsq(const float* __restrict__ row, int D, int lane) {
    double s = 0.0;
#pragma unroll 4
    for (int64_t d = lane; d < D; d += 64) {
        const double v = (double)row[d];
        s += v * v;
    }
    return loss_wave_sum(s);
}

__global__ __launch_bounds__(LOSS_NORM_ROWS * 64) void loss_inv_norm_kernel(const float* __restrict__ x, int64_t ldx, int rows, int D, double eps,
                                                                           float* __restrict__ inv) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * LOSS_NORM_ROWS + (threadIdx.x >> 6);
    if (r >= rows) return;
    const double nrm = sqrt(loss_row_sumsq(x + r * ldx, D, lane));
    if (lane == 0) inv[r] = (float)(1.0 / (nrm > eps ? nrm : eps));
}

__global__ __launch_bounds__(LOSS_NORM_ROWS * 64) void loss_inv_norm_bwd_kernel(const float* __restrict__ x, int64_t ldx, int rows, int D,
                                                                               double eps, const float* __restrict__ inv,
                                                                               const float* __restrict__ ginv, float* __restrict__ dx,
                                                                               int64_t lddx) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * LOSS_NORM_ROWS + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* xr = x + r * ldx;
    const bool clamped = sqrt(loss_row_sumsq(xr, D, lane)) < eps;      // the same in every lane
    double k = 0.0;
    if (!clamped) {
        const double iv = (double)inv[r];
        k = -(double)ginv[r] * ((iv * iv) * iv);
    }
    float* dr = dx + r * lddx;
#pragma unroll 4
    for (int64_t d = lane; d < lddx; d += 64) dr[d] = (d < D && !clamped) ? (float)(k * (double)xr[d]) : 0.0f;
}

// ------------------------------------------------------------------------------------ forward: a workgroup per row
// rule 1, H1: the cosine of class j of a row (zr its first element, ix its inverse norm), the centre that attains it and that centre's z
struct LossClass {
    double c;
    float z;
    int k;
};

template <bool FULL>
__device__ __forceinline__ LossClass loss_class(const LossParams& p, const float* __restrict__ zr, int64_t j, double ix) {
    const int K = FULL ? p.K : 1;
    const int64_t col = j * K;
    LossClass best;
    best.z = zr[col];
    best.k = 0;
    best.c = loss_cosine(p, best.z, ix, p.inv_w ? (double)p.inv_w[col] : 1.0);
    for (int k = 1; k < K; ++k) {                      // K > 1 only with a cosine head
        const float zf = zr[col + k];
        const double c = ((double)zf * ix) * (double)p.inv_w[col + k];
        if (c > best.c) {
            best.c = c;
            best.z = zf;
            best.k = k;
        }
    }
    return best;
}

// The cosines of the classes j0, j0 + 256, ... of a row, LOSS_UNROLL of them (-inf at and beyond N): the centre index is the outer
// loop, so the loads of all of them are in flight together.
__device__ __forceinline__ void loss_cosines(const LossParams& p, const float* __restrict__ zr, int64_t j0, double ix, double (&c)[LOSS_UNROLL]) {
#pragma unroll
    for (int u = 0; u < LOSS_UNROLL; ++u) {
        const int64_t j = j0 + (int64_t)u * LOSS_THREADS;
        c[u] = -INFINITY;
        if (j < p.N) c[u] = p.inv_x ? ((double)zr[j * p.K] * ix) * (double)p.inv_w[j * p.K] : (double)zr[j * p.K];
    }
    for (int k = 1; k < p.K; ++k) {                    // K > 1 only with a cosine head
#pragma unroll
        for (int u = 0; u < LOSS_UNROLL; ++u) {
            const int64_t j = j0 + (int64_t)u * LOSS_THREADS;
            if (j < p.N) {
                const double ck = ((double)zr[j * p.K + k] * ix) * (double)p.inv_w[j * p.K + k];
                c[u] = ck > c[u] ? ck : c[u];
            }
        }
    }
}

// f(j, c_j) on thread t's classes t, t + 256, ... of a row, in ascending order (rule 7, H5)
template <bool FULL, class F>
__device__ __forceinline__ void loss_for_classes(const LossParams& p, const float* __restrict__ zr, int t, double ix, F f) {
    if constexpr (FULL) {
        for (int64_t j0 = t; j0 < p.N; j0 += LOSS_UNROLL * LOSS_THREADS) {
            double cu[LOSS_UNROLL];
            loss_cosines(p, zr, j0, ix, cu);
#pragma unroll
            for (int u = 0; u < LOSS_UNROLL; ++u) {
                const int64_t j = j0 + (int64_t)u * LOSS_THREADS;
                if (j >= p.N) break;
                f(j, cu[u]);
            }
        }
    } else {
#pragma unroll 4
        for (int64_t j = t; j < p.N; j += LOSS_THREADS) f(j, loss_class<false>(p, zr, j, ix).c);
    }
}

// the total order of H2: (c, j) comes before (oc, oj)
__device__ __forceinline__ bool loss_before(double c, int j, double oc, int oj) { return c > oc || (c == oc && j < oj); }

template <bool FULL>
__global__ __launch_bounds__(LOSS_THREADS) void loss_forward_kernel(LossParams p, float* __restrict__ loss, int32_t* __restrict__ pred,
                                                                   double* __restrict__ lse, int32_t* __restrict__ hard,
                                                                   int32_t* __restrict__ sub_y) {
    __shared__ double red_m[LOSS_WAVES], red_c[LOSS_WAVES], red_s[LOSS_WAVES];
    __shared__ int red_i[LOSS_WAVES];
    __shared__ double red_l[LOSS_WAVES], sel_c[2][LOSS_WAVES];         // full only
    __shared__ int sel_i[2][LOSS_WAVES];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const float* __restrict__ zr = p.z + (int64_t)b * p.ldz;
    const int y = p.labels[b];
    const bool valid = y >= 0 && y < p.N;
    const double ix = p.inv_x ? (double)p.inv_x[b] : 1.0;
    double ly = 0.0;
    int ky = -1;
    if (valid) {
        const LossClass cy = loss_class<FULL>(p, zr, y, ix);
        ly = p.scale * loss_psi(p, cy.c);
        ky = cy.k;
    }

    // H2. A thread keeps the first LOSS_CAND of its own classes in the total order (j != y, beyond the last member so far) in
    // registers; a round is a workgroup-wide arg-max over the threads' first entries, and the winner's thread drops that entry. Only
    // a thread whose list runs empty while it had more classes reads its classes again. At the end (tc, ti) is the last of the row's
    // nh members: j is in H_b exactly when j != y and (c_j, j) does not come after (tc, ti).
    int nh = 0;
    double tc = INFINITY;
    int ti = -1;
    if constexpr (FULL) {
        const int want = valid ? (p.topk < p.N - 1 ? p.topk : p.N - 1) : 0;
        double lc[LOSS_CAND];
        int li[LOSS_CAND];                             // N: no entry (it comes after every class)
        bool more = want > 0;
        for (int r = 0; r < want; ++r) {
            if (r == 0 || li[0] == p.N) {              // the list is empty
                if (more) {
                    int seen = 0;
#pragma unroll
                    for (int q = 0; q < LOSS_CAND; ++q) {
                        lc[q] = -INFINITY;
                        li[q] = p.N;
                    }
                    loss_for_classes<true>(p, zr, t, ix, [&](int64_t j, double c) {
                        if (j == y || !loss_before(tc, ti, c, (int)j)) return;       // (false for a NaN)
                        ++seen;
                        int i = (int)j;
#pragma unroll
                        for (int q = 0; q < LOSS_CAND; ++q) {          // insertion: what an entry displaces moves on down the list
                            if (loss_before(c, i, lc[q], li[q])) {
                                const double oc = lc[q];
                                const int oi = li[q];
                                lc[q] = c;
                                li[q] = i;
                                c = oc;
                                i = oi;
                            }
                        }
                    });
                    more = seen > LOSS_CAND;
                }
            }
            double bc = lc[0];
            int bi = li[0];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const double oc = __shfl_xor(bc, d, 64);
                const int oi = __shfl_xor(bi, d, 64);
                if (oi < p.N && (bi == p.N || loss_before(oc, oi, bc, bi))) {
                    bc = oc;
                    bi = oi;
                }
            }
            if (lane == 0) {
                sel_c[r & 1][w] = bc;
                sel_i[r & 1][w] = bi;
            }
            __syncthreads();                           // one barrier a round: the buffers alternate
            bc = sel_c[r & 1][0];
            bi = sel_i[r & 1][0];
#pragma unroll
            for (int g = 1; g < LOSS_WAVES; ++g) {
                const double oc = sel_c[r & 1][g];
                const int oi = sel_i[r & 1][g];
                if (oi < p.N && (bi == p.N || loss_before(oc, oi, bc, bi))) {
                    bc = oc;
                    bi = oi;
                }
            }
            if (bi == p.N) break;                      // only NaN cosines are left (the same in every thread)
            tc = bc;
            ti = bi;
            if (li[0] == bi) {                         // the winner's thread: its next entry moves up
#pragma unroll
                for (int q = 0; q + 1 < LOSS_CAND; ++q) {
                    lc[q] = lc[q + 1];
                    li[q] = li[q + 1];
                }
                lc[LOSS_CAND - 1] = -INFINITY;
                li[LOSS_CAND - 1] = p.N;
            }
            if (t == 0) hard[(int64_t)b * p.width + r] = bi;
            nh = r + 1;
        }
        if (hard)
            for (int r = nh + t; r < p.width; r += LOSS_THREADS) hard[(int64_t)b * p.width + r] = -1;
    }
    // rule 4, H2: the logit of class j
    const auto logit = [&](int64_t j, double c) {
        if (valid && j == y) return ly;
        if constexpr (FULL)
            if (nh > 0 && !loss_before(tc, ti, c, (int)j) && c == c) return p.scale * (c + p.penalty);
        return p.scale * c;
    };

    // pass 1: the largest logit, and the first class of the largest cosine
    double m = -INFINITY, cb = -INFINITY;
    int ib = p.N;
    loss_for_classes<FULL>(p, zr, t, ix, [&](int64_t j, double c) {
        const double l = logit(j, c);
        m = l > m ? l : m;
        // ascending j: the lowest index of a thread's classes stays. (Selects: with an `if` around the two assignments the compiler
        // does not issue the loads of an unrolled step of the plain loop together.)
        const bool first = c > cb;
        cb = first ? c : cb;
        ib = first ? (int)j : ib;
    });
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double om = __shfl_xor(m, d, 64), oc = __shfl_xor(cb, d, 64);
        const int oi = __shfl_xor(ib, d, 64);
        m = om > m ? om : m;
        if (oc > cb || (oc == cb && oi < ib)) {
            cb = oc;
            ib = oi;
        }
    }
    if (lane == 0) {
        red_m[w] = m;
        red_c[w] = cb;
        red_i[w] = ib;
    }
    __syncthreads();
    m = red_m[0];
    cb = red_c[0];
    ib = red_i[0];
#pragma unroll
    for (int g = 1; g < LOSS_WAVES; ++g) {
        m = red_m[g] > m ? red_m[g] : m;
        if (red_c[g] > cb || (red_c[g] == cb && red_i[g] < ib)) {
            cb = red_c[g];
            ib = red_i[g];
        }
    }

    // pass 2: the row again (from the cache), the sums of rule 7 and H5
    const bool smooth = FULL && p.eps != 0.0;          // H3: without smoothing the sum of the logits is not formed
    double s = 0.0, sl = 0.0;
    loss_for_classes<FULL>(p, zr, t, ix, [&](int64_t j, double c) {
        const double l = logit(j, c);
        s += exp(l - m);
        if (smooth) sl += l;
    });
    s = loss_wave_sum(s);
    if (smooth) sl = loss_wave_sum(sl);
    if (lane == 0) {
        red_s[w] = s;
        if constexpr (FULL) red_l[w] = sl;
    }
    __syncthreads();
    if (t == 0) {
        double tot = red_s[0], totl = FULL ? red_l[0] : 0.0;
#pragma unroll
        for (int g = 1; g < LOSS_WAVES; ++g) {
            tot += red_s[g];
            if constexpr (FULL) totl += red_l[g];
        }
        const double v = m + log(tot);
        lse[b] = v;
        double out = v - ly;
        if (smooth) out = out + p.eps * (ly - totl / (double)p.N);
        loss[b] = valid ? (float)out : 0.0f;
        if (pred) pred[b] = ib < p.N ? ib : 0;         // no class compares (every cosine NaN or -inf): 0
        if constexpr (FULL)
            if (sub_y) sub_y[b] = ky;
    }
}

// ------------------------------------------------------------------------------------ backward: (block of rows) x (chunk of classes)
template <bool FULL>
__global__ __launch_bounds__(LOSS_THREADS) void loss_backward_kernel(LossParams p, const double* __restrict__ lse, const int32_t* __restrict__ hard,
                                                                    const float* __restrict__ gloss, float* dz, int64_t lddz, int nchunks,
                                                                    int nchunks_n, double* __restrict__ slots, double* __restrict__ rowpart) {
    constexpr int NK = FULL ? LOSS_KMAX : 1;           // running sums a thread keeps
    __shared__ double red[LOSS_WAVES][LOSS_ROWS];
    __shared__ unsigned char member[LOSS_ROWS][LOSS_THREADS];   // full only, H2: class j0 + t of row r is listed in `hard`
    const int K = FULL ? p.K : 1;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int chunk = blockIdx.x % nchunks, slot = blockIdx.x / nchunks;
    const int64_t j0 = (int64_t)chunk * LOSS_THREADS, j = j0 + t;
    const int64_t col = j * K, ncols = (int64_t)p.N * K;
    const bool in = j < p.N, cosine = p.inv_x != nullptr;
    const double iw0 = (in && cosine) ? (double)p.inv_w[col] : 1.0;    // centre 0 of the class
    const int b0 = slot * LOSS_ROWS;

    if constexpr (FULL) {
        if (p.topk > 0) {                              // the same in every thread
#pragma unroll
            for (int r = 0; r < LOSS_ROWS; ++r) member[r][t] = 0;
            __syncthreads();
            for (int e = t; e < LOSS_ROWS * p.topk; e += LOSS_THREADS) {
                const int r = e / p.topk, i = e - r * p.topk;
                if (b0 + r < p.B) {
                    const int64_t h = hard[(int64_t)(b0 + r) * p.width + i];
                    if (h >= j0 && h < j0 + LOSS_THREADS) member[r][h - j0] = 1;
                }
            }
            __syncthreads();
        }
    }

    // Every load of z before the first store of dz, and a thread reads only the columns it writes: dz may be z. Full: the selected centre
    // k* of every row (H1) is found here too, the rows' loads of a centre in flight together.
    float zf[LOSS_ROWS];
    int ys[LOSS_ROWS];
    int ks[LOSS_ROWS];                                 // full only: k*, its cosine, the row's inverse norm
    double cs[LOSS_ROWS], ixs[LOSS_ROWS];
#pragma unroll
    for (int r = 0; r < LOSS_ROWS; ++r) {
        const int b = b0 + r;
        ys[r] = -1;
        zf[r] = 0.0f;
        if constexpr (FULL) {
            ks[r] = -1;
            cs[r] = 0.0;
            ixs[r] = 1.0;
        }
        if (b < p.B) {
            const int y = p.labels[b];
            ys[r] = (y >= 0 && y < p.N) ? y : -1;
            if (ys[r] >= 0 && in) {
                if constexpr (FULL)
                    if (cosine) ixs[r] = (double)p.inv_x[b];
                zf[r] = p.z[(int64_t)b * p.ldz + col];
                if constexpr (FULL) {
                    ks[r] = 0;
                    cs[r] = cosine ? ((double)zf[r] * ixs[r]) * iw0 : (double)zf[r];
                }
            }
        }
    }
    if constexpr (FULL) {
        for (int k = 1; k < K; ++k) {                  // K > 1 only with a cosine head
            const double iwk = in ? (double)p.inv_w[col + k] : 1.0;
#pragma unroll
            for (int r = 0; r < LOSS_ROWS; ++r) {
                if (ks[r] >= 0) {
                    const float zk = p.z[(int64_t)(b0 + r) * p.ldz + col + k];
                    const double ck = ((double)zk * ixs[r]) * iwk;
                    if (ck > cs[r]) {
                        cs[r] = ck;
                        zf[r] = zk;
                        ks[r] = k;
                    }
                }
            }
        }
    }
    double acc[NK];                                    // dinv_w[j * K + k] of this block of rows
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[k] = 0.0;
#pragma unroll
    for (int r = 0; r < LOSS_ROWS; ++r) {
        const int b = b0 + r;
        if (b >= p.B) {                                // the same in every thread
            if (lane == 0) red[w][r] = 0.0;
            continue;
        }
        float out = 0.0f;
        double rowterm = 0.0;
        if (ys[r] >= 0 && in) {
            const double ix = FULL ? ixs[r] : cosine ? (double)p.inv_x[b] : 1.0;
            const double iw = !FULL ? iw0 : cosine ? (double)p.inv_w[col + ks[r]] : 1.0;
            const double c = FULL ? cs[r] : loss_cosine(p, zf[r], ix, iw);
            const bool tgt = j == ys[r];
            double l = tgt ? loss_psi(p, c) : c;
            if constexpr (FULL)
                if (!tgt && p.topk > 0 && member[r][t]) l = c + p.penalty;
            l = p.scale * l;
            const double pj = exp(l - lse[b]);
            const double g = gloss ? (double)gloss[b] : 1.0;
            const double hot = tgt ? 1.0 : 0.0;
            double dp = pj - hot;
            if constexpr (FULL) dp = dp + p.eps * (hot - p.inv_n);       // H3
            double dc = (g * p.scale) * dp;
            if (tgt) dc = dc * loss_dpsi(p, c);
            if (cosine) {
                out = (float)((dc * ix) * iw);
                const double dcz = dc * (double)zf[r];
                rowterm = dcz * iw;
                const double term = dcz * ix;
                if constexpr (FULL) {
#pragma unroll
                    for (int k = 0; k < NK; ++k)       // predicated adds: no indexing by k*
                        if (k == ks[r]) acc[k] += term;
                } else {
                    acc[0] += term;
                }
            } else {
                out = (float)dc;
            }
        }
        float* dr = dz + (int64_t)b * lddz;
        if constexpr (FULL) {
            if (in) {
                for (int k = 0; k < K; ++k) dr[col + k] = k == ks[r] ? out : 0.0f;
            } else {                                   // the pad columns: thread t takes K of the chunk's columns at and beyond N * K
                for (int k = 0; k < K; ++k)
                    if (col + k < lddz) dr[col + k] = 0.0f;
            }
        } else {
            if (j < lddz) dr[j] = out;
        }
        if (cosine) {
            const double rs = loss_wave_sum(rowterm);
            if (lane == 0) red[w][r] = rs;
        }
    }
    if (!cosine || chunk >= nchunks_n) return;         // the same in every thread
    if (in) {
        if constexpr (FULL) {
#pragma unroll
            for (int k = 0; k < NK; ++k)
                if (k < K) slots[(int64_t)slot * ncols + col + k] = acc[k];
        } else {
            slots[(int64_t)slot * ncols + col] = acc[0];
        }
    }
    __syncthreads();
    if (t < LOSS_ROWS && b0 + t < p.B) {
        double rs = red[0][t];
#pragma unroll
        for (int g = 1; g < LOSS_WAVES; ++g) rs += red[g][t];
        rowpart[(int64_t)chunk * p.B + b0 + t] = rs;
    }
}

// `count` partial sums `stride` doubles apart, added in ascending order, LOSS_FIN_BATCH loads in flight (a chain of dependent loads
// would cost a memory latency each); consecutive threads read consecutive doubles. Terms past the last are +0.0, which changes no sum.
__device__ __forceinline__ double loss_sum_strided(const double* __restrict__ first, int count, int64_t stride) {
    double sum = 0.0;
    for (int s0 = 0; s0 < count; s0 += LOSS_FIN_BATCH) {
        double v[LOSS_FIN_BATCH];
#pragma unroll
        for (int u = 0; u < LOSS_FIN_BATCH; ++u) v[u] = s0 + u < count ? first[(int64_t)(s0 + u) * stride] : 0.0;
#pragma unroll
        for (int u = 0; u < LOSS_FIN_BATCH; ++u) sum += v[u];
    }
    return sum;
}

// workgroups [0, col_blocks): dinv_w (ncols = N * K centres) from the slots; the rest: dinv_x from the rows' sums per chunk
__global__ __launch_bounds__(LOSS_THREADS) void loss_finalize_kernel(const double* __restrict__ slots, int nslots, const double* __restrict__ rowpart,
                                                                    int nchunks_n, int B, int64_t ncols, int col_blocks,
                                                                    float* __restrict__ dinv_x, float* __restrict__ dinv_w) {
    if ((int)blockIdx.x < col_blocks) {
        const int64_t j = (int64_t)blockIdx.x * LOSS_THREADS + threadIdx.x;
        if (j < ncols) dinv_w[j] = (float)loss_sum_strided(slots + j, nslots, ncols);
    } else {
        const int64_t b = (int64_t)(blockIdx.x - col_blocks) * LOSS_THREADS + threadIdx.x;
        if (b < B) dinv_x[b] = (float)loss_sum_strided(rowpart + b, nchunks_n, B);
    }
}

// ------------------------------------------------------------------------------------ host
bool loss_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na > 0 && nb > 0 && a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}

struct LossSizes {
    int64_t nslots, nchunks, slot_bytes, bytes;
};

int loss_sizes(const char* who, int64_t B, int64_t N, int64_t K, LossSizes* s) {
    KTF_REQUIRE(B >= 0, "%s: negative size", who);
    KTF_REQUIRE(N >= 1, "%s: N %lld below 1", who, (long long)N);
    KTF_REQUIRE(K >= 1 && K <= KTF_HEAD_MAX_CENTERS, "%s: K %lld outside [1, %d]", who, (long long)K, KTF_HEAD_MAX_CENTERS);
    KTF_REQUIRE(B < (1ll << 31) && N < (1ll << 31) && N * K < (1ll << 31), "%s: B or N * K reaches 2^31", who);
    s->nslots = (B + LOSS_ROWS - 1) / LOSS_ROWS;
    s->nchunks = (N + LOSS_THREADS - 1) / LOSS_THREADS;
    KTF_REQUIRE(s->nslots * s->nchunks < (1ll << 31), "%s: batch too large for one grid (2^31 workgroups)", who);
    s->slot_bytes = al256((s->nslots > 0 ? s->nslots : 1) * N * K * 8);
    s->bytes = s->slot_bytes + al256(s->nchunks * (B > 0 ? B : 1) * 8);
    return KTF_OK;
}

// What the forward and the backward call of either header are given alike. The calls of ktf_loss.h have K = 1, topk = 0, penalty = 0,
// smoothing = 0 and hard = NULL.
struct LossCall {
    const char* who;
    const float* z;
    int64_t ldz, B, N, K;
    const int32_t* labels;
    const float *inv_x, *inv_w;
    int32_t kind;
    double margin, scale;
    int32_t topk;
    double penalty, smoothing;
    const int32_t* hard;
    void* workspace;
    size_t workspace_bytes;
    void* stream;
};

// rule 10 and H7 for what both calls are given, the constants of rule 3; [ldmin, ldmax] spans the call's leading dimensions
int loss_check(const LossCall& c, int64_t ldmin, int64_t ldmax, LossSizes* s, LossParams* p) {
    const char* who = c.who;
    if (int rc = loss_sizes(who, c.B, c.N, c.K, s)) return rc;
    KTF_REQUIRE(ldmin >= c.N * c.K, "%s: leading dimension %lld below N * K %lld", who, (long long)ldmin, (long long)(c.N * c.K));
    KTF_REQUIRE(ldmax < (1ll << 31), "%s: leading dimension reaches 2^31", who);
    KTF_REQUIRE((c.inv_x != nullptr) == (c.inv_w != nullptr), "%s: inv_x and inv_w go together (both for a cosine head, neither for a plain one)",
                who);
    KTF_REQUIRE(c.kind == KTF_LOSS_SOFTMAX || c.kind == KTF_LOSS_AM || c.kind == KTF_LOSS_AAM, "%s: unknown kind %d", who, (int)c.kind);
    KTF_REQUIRE(c.kind == KTF_LOSS_SOFTMAX || c.inv_x, "%s: a margin kind needs a cosine head (inv_x, inv_w)", who);
    KTF_REQUIRE(c.scale > 0.0 && c.scale < INFINITY, "%s: scale must be positive and finite", who);
    KTF_REQUIRE(c.margin >= 0.0 && c.margin < INFINITY, "%s: margin must be finite and not negative", who);
    KTF_REQUIRE(c.kind != KTF_LOSS_SOFTMAX || c.margin == 0.0, "%s: margin must be 0 for KTF_LOSS_SOFTMAX", who);
    KTF_REQUIRE(c.kind != KTF_LOSS_AAM || c.margin < 1.5707963267948966, "%s: margin must be below pi / 2 for KTF_LOSS_AAM", who);
    KTF_REQUIRE(c.K == 1 || c.inv_x, "%s: sub-centres (K > 1) need a cosine head (inv_x, inv_w)", who);
    KTF_REQUIRE(c.topk >= 0 && c.topk <= KTF_HEAD_MAX_TOPK, "%s: topk %d outside [0, %d]", who, (int)c.topk, KTF_HEAD_MAX_TOPK);
    KTF_REQUIRE(c.topk == 0 || c.inv_x, "%s: topk > 0 needs a cosine head (inv_x, inv_w)", who);
    KTF_REQUIRE(c.penalty >= 0.0 && c.penalty < INFINITY, "%s: penalty must be finite and not negative", who);
    KTF_REQUIRE(c.topk > 0 || c.penalty == 0.0, "%s: penalty must be 0 when topk is 0", who);
    KTF_REQUIRE(c.smoothing >= 0.0 && c.smoothing < 1.0, "%s: smoothing must be in [0, 1)", who);
    KTF_REQUIRE(c.topk == 0 || c.hard, "%s: null hard with topk > 0", who);
    KTF_REQUIRE(c.workspace, "%s: null argument", who);
    if (int rc = ktf_check_workspace(who, c.workspace, c.workspace_bytes, s->bytes)) return rc;
    p->z = c.z;
    p->ldz = c.ldz;
    p->B = (int)c.B;
    p->N = (int)c.N;
    p->K = (int)c.K;
    p->labels = c.labels;
    p->inv_x = c.inv_x;
    p->inv_w = c.inv_w;
    p->kind = c.kind;
    p->margin = c.margin;
    p->scale = c.scale;
    p->cm = cos(c.margin);
    p->sm = sin(c.margin);
    p->msm = c.margin * p->sm;
    p->topk = c.topk;
    p->width = c.topk > 1 ? c.topk : 1;
    p->penalty = c.penalty;
    p->eps = c.smoothing;
    p->inv_n = 1.0 / (double)c.N;
    return KTF_OK;
}

template <bool FULL>
int loss_forward(const LossCall& c, float* loss, int32_t* pred, double* lse, int32_t* hard, int32_t* sub_y) {
    KTF_REQUIRE(c.z && c.labels && loss && lse, "%s: null argument", c.who);
    LossSizes s;
    LossParams p = {};
    if (int rc = loss_check(c, c.ldz, c.ldz, &s, &p)) return rc;
    if (c.B == 0) return KTF_OK;
    hipLaunchKernelGGL(loss_forward_kernel<FULL>, dim3((unsigned)c.B), dim3(LOSS_THREADS), 0, (hipStream_t)c.stream, p, loss, pred, lse, hard,
                       sub_y);
    KTF_CHECK_LAUNCH(c.who);
    return KTF_OK;
}

template <bool FULL>
int loss_backward(const LossCall& c, const double* lse, const float* gloss, float* dz, int64_t lddz, float* dinv_x, float* dinv_w) {
    const char* who = c.who;
    const int64_t ncols = c.N * c.K;
    KTF_REQUIRE(c.z && c.labels && lse && dz, "%s: null argument", who);
    LossSizes s;
    LossParams p = {};
    if (int rc = loss_check(c, c.ldz < lddz ? c.ldz : lddz, c.ldz > lddz ? c.ldz : lddz, &s, &p)) return rc;
    KTF_REQUIRE((dinv_x != nullptr) == (c.inv_x != nullptr) && (dinv_w != nullptr) == (c.inv_w != nullptr),
                "%s: dinv_x and dinv_w go with a cosine head (both), not with a plain one (neither)", who);
    KTF_REQUIRE((c.z == dz && c.ldz == lddz) || !loss_overlap(c.z, c.B > 0 ? (c.B - 1) * c.ldz + ncols : 0, dz, c.B * lddz),
                "%s: dz overlaps z (other than being z itself)", who);
    hipStream_t st = (hipStream_t)c.stream;
    if (c.B == 0) {                                    // rule 9, H6: no kernel; the sum over no row
        if (dinv_w && hipMemsetAsync(dinv_w, 0, (size_t)ncols * 4, st) != hipSuccess) {
            ktf_set_error("%s: hipMemsetAsync failed", who);
            return KTF_ELAUNCH;
        }
        return KTF_OK;
    }
    double* slots = reinterpret_cast<double*>(c.workspace);
    double* rowpart = reinterpret_cast<double*>(reinterpret_cast<char*>(c.workspace) + s.slot_bytes);
    const int64_t chunk_cols = (int64_t)LOSS_THREADS * c.K;                             // the pad columns of dz are written too
    const int64_t nchunks = (lddz + chunk_cols - 1) / chunk_cols;
    KTF_REQUIRE(s.nslots * nchunks < (1ll << 31), "%s: batch too large for one grid (2^31 workgroups)", who);
    hipLaunchKernelGGL(loss_backward_kernel<FULL>, dim3((unsigned)(s.nslots * nchunks)), dim3(LOSS_THREADS), 0, st, p, lse, c.hard, gloss, dz,
                       lddz, (int)nchunks, (int)s.nchunks, slots, rowpart);
    KTF_CHECK_LAUNCH(who);
    if (c.inv_x) {
        const int col_blocks = ktf_cdiv(ncols, LOSS_THREADS), row_blocks = ktf_cdiv(c.B, LOSS_THREADS);
        hipLaunchKernelGGL(loss_finalize_kernel, dim3((unsigned)(col_blocks + row_blocks)), dim3(LOSS_THREADS), 0, st, slots, (int)s.nslots,
                           rowpart, (int)s.nchunks, (int)c.B, ncols, col_blocks, dinv_x, dinv_w);
        KTF_CHECK_LAUNCH(who);
    }
    return KTF_OK;
}

int loss_norm_check(const char* who, int64_t ldmin, int64_t ldmax, int64_t rows, int64_t D, double eps) {
    KTF_REQUIRE(rows >= 0, "%s: negative size", who);
    KTF_REQUIRE(D >= 1, "%s: D %lld below 1", who, (long long)D);
    KTF_REQUIRE(rows < (1ll << 31) && D < (1ll << 31) && ldmax < (1ll << 31), "%s: rows, D or a leading dimension reaches 2^31", who);
    KTF_REQUIRE(ldmin >= D, "%s: leading dimension %lld below D %lld", who, (long long)ldmin, (long long)D);
    KTF_REQUIRE(eps > 0.0 && eps < INFINITY, "%s: eps must be positive and finite", who);
    return KTF_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------ entry points
extern "C" int32_t ktf_loss_slot_rows(void) { return KTF_LOSS_SLOT_ROWS; }
extern "C" int32_t ktf_head_slot_rows(void) { return KTF_HEAD_SLOT_ROWS; }

extern "C" int64_t ktf_loss_workspace_bytes(int64_t B, int64_t N) {
    LossSizes s;
    if (int rc = loss_sizes("ktf_loss_workspace_bytes", B, N, 1, &s)) return rc;
    return s.bytes;
}

extern "C" int64_t ktf_head_workspace_bytes(int64_t B, int64_t N, int64_t K) {
    LossSizes s;
    if (int rc = loss_sizes("ktf_head_workspace_bytes", B, N, K, &s)) return rc;
    return s.bytes;
}

extern "C" int ktf_loss_row_inv_norm(const float* x, int64_t ldx, int64_t rows, int64_t D, double eps, float* inv, void* stream) {
    const char* who = "ktf_loss_row_inv_norm";
    KTF_REQUIRE(x && inv, "%s: null argument", who);
    if (int rc = loss_norm_check(who, ldx, ldx, rows, D, eps)) return rc;
    if (rows == 0) return KTF_OK;
    hipLaunchKernelGGL(loss_inv_norm_kernel, dim3((unsigned)ktf_cdiv(rows, LOSS_NORM_ROWS)), dim3(LOSS_NORM_ROWS * 64), 0, (hipStream_t)stream, x,
                       ldx, (int)rows, (int)D, eps, inv);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_loss_row_inv_norm_backward(const float* x, int64_t ldx, int64_t rows, int64_t D, double eps, const float* inv,
                                              const float* ginv, float* dx, int64_t lddx, void* stream) {
    const char* who = "ktf_loss_row_inv_norm_backward";
    KTF_REQUIRE(x && inv && ginv && dx, "%s: null argument", who);
    if (int rc = loss_norm_check(who, ldx < lddx ? ldx : lddx, ldx > lddx ? ldx : lddx, rows, D, eps)) return rc;
    KTF_REQUIRE(!loss_overlap(x, rows > 0 ? (rows - 1) * ldx + D : 0, dx, rows * lddx), "%s: dx overlaps x", who);
    if (rows == 0) return KTF_OK;
    hipLaunchKernelGGL(loss_inv_norm_bwd_kernel, dim3((unsigned)ktf_cdiv(rows, LOSS_NORM_ROWS)), dim3(LOSS_NORM_ROWS * 64), 0,
                       (hipStream_t)stream, x, ldx, (int)rows, (int)D, eps, inv, ginv, dx, lddx);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

// ktf_loss_* always launch the plain instantiation, ktf_head_* always the full one, with every switch off included
extern "C" int ktf_loss_margin_softmax_forward(const float* z, int64_t ldz, int64_t B, int64_t N, const int32_t* labels, const float* inv_x,
                                               const float* inv_w, int32_t kind, double margin, double scale, float* loss, int32_t* pred,
                                               double* lse, void* workspace, size_t workspace_bytes, void* stream) {
    const LossCall c = {"ktf_loss_margin_softmax_forward", z, ldz, B, N, 1, labels, inv_x, inv_w, kind, margin, scale, 0, 0.0, 0.0, nullptr,
                        workspace, workspace_bytes, stream};
    return loss_forward<false>(c, loss, pred, lse, nullptr, nullptr);
}

extern "C" int ktf_loss_margin_softmax_backward(const float* z, int64_t ldz, int64_t B, int64_t N, const int32_t* labels, const float* inv_x,
                                                const float* inv_w, int32_t kind, double margin, double scale, const double* lse,
                                                const float* gloss, float* dz, int64_t lddz, float* dinv_x, float* dinv_w, void* workspace,
                                                size_t workspace_bytes, void* stream) {
    const LossCall c = {"ktf_loss_margin_softmax_backward", z, ldz, B, N, 1, labels, inv_x, inv_w, kind, margin, scale, 0, 0.0, 0.0, nullptr,
                        workspace, workspace_bytes, stream};
    return loss_backward<false>(c, lse, gloss, dz, lddz, dinv_x, dinv_w);
}

extern "C" int ktf_head_forward(const float* z, int64_t ldz, int64_t B, int64_t N, int64_t K, const int32_t* labels, const float* inv_x,
                                const float* inv_w, int32_t kind, double margin, double scale, int32_t topk, double penalty,
                                double smoothing, float* loss, int32_t* pred, double* lse, int32_t* hard, int32_t* sub_y, void* workspace,
                                size_t workspace_bytes, void* stream) {
    const LossCall c = {"ktf_head_forward", z, ldz, B, N, K, labels, inv_x, inv_w, kind, margin, scale, topk, penalty, smoothing, hard,
                        workspace, workspace_bytes, stream};
    return loss_forward<true>(c, loss, pred, lse, hard, sub_y);
}

extern "C" int ktf_head_backward(const float* z, int64_t ldz, int64_t B, int64_t N, int64_t K, const int32_t* labels, const float* inv_x,
                                 const float* inv_w, int32_t kind, double margin, double scale, int32_t topk, double penalty,
                                 double smoothing, const double* lse, const int32_t* hard, const float* gloss, float* dz, int64_t lddz,
                                 float* dinv_x, float* dinv_w, void* workspace, size_t workspace_bytes, void* stream) {
    const LossCall c = {"ktf_head_backward", z, ldz, B, N, K, labels, inv_x, inv_w, kind, margin, scale, topk, penalty, smoothing, hard,
                        workspace, workspace_bytes, stream};
    return loss_backward<true>(c, lse, gloss, dz, lddz, dinv_x, dinv_w);
}
