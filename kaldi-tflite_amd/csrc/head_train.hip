// The classification head's loss with sub-centres, an inter-top-k penalty and label smoothing (include/ktf_head.h, whose rule numbers
// the comments use; psi and the inverse norms are those of include/ktf_loss.h and csrc/loss_train.hip).
//   ktf_head_forward     head_forward_kernel: a workgroup per row -- the selection of H2 (a pass that leaves every thread's first classes
//                        in the total order in registers, then a workgroup-wide arg-max per member), then the two passes of the plain loss
//   ktf_head_backward    head_backward_kernel: a workgroup per (block of rows, chunk of classes), one pass that writes dz and the partial
//                        sums of dinv_x and dinv_w -> head_finalize_kernel adds them (cosine head only)
// A thread owns a class: it reads the K floats of the class's centres one at a time, so a wave covers 64 * K contiguous floats per
// step, four bytes per lane and access whatever the alignment (H5). With K = 1, topk = 0 and smoothing = 0 every operation on a value
// is that of loss_train.hip in the same order, which is what makes the outputs equal bit for bit.
#include "common.h"
#include "../../include/ktf_loss.h"
#include "../../include/ktf_head.h"

// every fp64 operation is rounded on its own: no contraction into fma
#pragma clang fp contract(off)

namespace {

constexpr int HEAD_THREADS = KTF_HEAD_CHUNK_CLASSES;
constexpr int HEAD_WAVES = HEAD_THREADS / 64;
constexpr int HEAD_ROWS = KTF_HEAD_SLOT_ROWS;
constexpr int HEAD_KMAX = KTF_HEAD_MAX_CENTERS;
constexpr int HEAD_UNROLL = 4;          // forward: classes a thread has in flight
constexpr int HEAD_CAND = 4;            // forward: classes a thread holds for the selection of H2
constexpr int HEAD_FIN_BATCH = 8;       // finalize: partial sums a thread has in flight

struct HeadParams {
    const float* z;
    int64_t ldz;
    int B, N, K;
    const int32_t* labels;
    const float* inv_x;     // both NULL: plain head
    const float* inv_w;
    int kind;
    double margin, scale, cm, sm, msm;   // cos m, sin m, m * sin m (ktf_loss.h, rule 3)
    int topk, width;                     // width = max(topk, 1): the row length of `hard`
    double penalty, eps, inv_n;          // smoothing, 1 / (double)N
};

__device__ __forceinline__ double head_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ double head_psi(const HeadParams& p, double c) {
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

__device__ __forceinline__ double head_dpsi(const HeadParams& p, double c) {
    if (p.kind == KTF_LOSS_AAM && c > -p.cm) {
        const double s2 = 1.0 - c * c;
        return s2 > KTF_LOSS_SIN2_FLOOR ? p.cm + (p.sm * c) / sqrt(s2) : p.cm;
    }
    return 1.0;
}

// H1: the cosine of class j of a row (zr its first element, ix its inverse norm), the centre that attains it and that centre's z
struct HeadClass {
    double c;
    float z;
    int k;
};

__device__ __forceinline__ HeadClass head_class(const HeadParams& p, const float* __restrict__ zr, int64_t j, double ix) {
    const int64_t col = j * p.K;
    HeadClass best;
    best.z = zr[col];
    best.k = 0;
    best.c = p.inv_x ? ((double)best.z * ix) * (double)p.inv_w[col] : (double)best.z;
    for (int k = 1; k < p.K; ++k) {                    // K > 1 only with a cosine head
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

// The cosines of the classes j0, j0 + 256, ... of a row, HEAD_UNROLL of them (-inf at and beyond N): the centre index is the outer
// loop, so the loads of all of them are in flight together.
__device__ __forceinline__ void head_cosines(const HeadParams& p, const float* __restrict__ zr, int64_t j0, double ix, double (&c)[HEAD_UNROLL]) {
#pragma unroll
    for (int u = 0; u < HEAD_UNROLL; ++u) {
        const int64_t j = j0 + (int64_t)u * HEAD_THREADS;
        c[u] = -INFINITY;
        if (j < p.N) c[u] = p.inv_x ? ((double)zr[j * p.K] * ix) * (double)p.inv_w[j * p.K] : (double)zr[j * p.K];
    }
    for (int k = 1; k < p.K; ++k) {                    // K > 1 only with a cosine head
#pragma unroll
        for (int u = 0; u < HEAD_UNROLL; ++u) {
            const int64_t j = j0 + (int64_t)u * HEAD_THREADS;
            if (j < p.N) {
                const double ck = ((double)zr[j * p.K + k] * ix) * (double)p.inv_w[j * p.K + k];
                c[u] = ck > c[u] ? ck : c[u];
            }
        }
    }
}

// the total order of H2: (c, j) comes before (oc, oj)
__device__ __forceinline__ bool head_before(double c, int j, double oc, int oj) { return c > oc || (c == oc && j < oj); }

// the logit of class j (H2, and rule 4 of ktf_loss.h): (tc, ti) is the last of the row's nh members in the total order
__device__ __forceinline__ double head_logit(const HeadParams& p, double c, int j, bool target, double ly, int nh, double tc, int ti) {
    if (target) return ly;
    if (nh > 0 && !head_before(tc, ti, c, j) && c == c) return p.scale * (c + p.penalty);
    return p.scale * c;
}

// ------------------------------------------------------------------------------------ forward: a workgroup per row
__global__ __launch_bounds__(HEAD_THREADS) void head_forward_kernel(HeadParams p, float* __restrict__ loss, int32_t* __restrict__ pred,
                                                                   double* __restrict__ lse, int32_t* __restrict__ hard,
                                                                   int32_t* __restrict__ sub_y) {
    __shared__ double red_m[HEAD_WAVES], red_c[HEAD_WAVES], red_s[HEAD_WAVES], red_l[HEAD_WAVES];
    __shared__ int red_i[HEAD_WAVES];
    __shared__ double sel_c[2][HEAD_WAVES];
    __shared__ int sel_i[2][HEAD_WAVES];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const float* __restrict__ zr = p.z + (int64_t)b * p.ldz;
    const int y = p.labels[b];
    const bool valid = y >= 0 && y < p.N;
    const double ix = p.inv_x ? (double)p.inv_x[b] : 1.0;
    double ly = 0.0;
    int ky = -1;
    if (valid) {
        const HeadClass cy = head_class(p, zr, y, ix);
        ly = p.scale * head_psi(p, cy.c);
        ky = cy.k;
    }

    // H2. A thread keeps the first HEAD_CAND of its own classes in the total order (j != y, beyond the last member so far) in
    // registers; a round is a workgroup-wide arg-max over the threads' first entries, and the winner's thread drops that entry. Only
    // a thread whose list runs empty while it had more classes reads its classes again. At the end (tc, ti) is the last member:
    // j is in H_b exactly when j != y and (c_j, j) does not come after (tc, ti).
    const int want = valid ? (p.topk < p.N - 1 ? p.topk : p.N - 1) : 0;
    int nh = 0;
    double tc = INFINITY;
    int ti = -1;
    double lc[HEAD_CAND];
    int li[HEAD_CAND];                                 // N: no entry (it comes after every class)
    bool more = want > 0;
    for (int r = 0; r < want; ++r) {
        if (r == 0 || li[0] == p.N) {                  // the list is empty
            if (more) {
                int seen = 0;
#pragma unroll
                for (int q = 0; q < HEAD_CAND; ++q) {
                    lc[q] = -INFINITY;
                    li[q] = p.N;
                }
                for (int64_t j0 = t; j0 < p.N; j0 += HEAD_UNROLL * HEAD_THREADS) {
                    double cu[HEAD_UNROLL];
                    head_cosines(p, zr, j0, ix, cu);
#pragma unroll
                    for (int u = 0; u < HEAD_UNROLL; ++u) {
                        const int64_t j = j0 + (int64_t)u * HEAD_THREADS;
                        if (j >= p.N || j == y || !head_before(tc, ti, cu[u], (int)j)) continue;     // (false for a NaN)
                        ++seen;
                        double c = cu[u];
                        int i = (int)j;
#pragma unroll
                        for (int q = 0; q < HEAD_CAND; ++q) {      // insertion: what an entry displaces moves on down the list
                            if (head_before(c, i, lc[q], li[q])) {
                                const double oc = lc[q];
                                const int oi = li[q];
                                lc[q] = c;
                                li[q] = i;
                                c = oc;
                                i = oi;
                            }
                        }
                    }
                }
                more = seen > HEAD_CAND;
            }
        }
        double bc = lc[0];
        int bi = li[0];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double oc = __shfl_xor(bc, d, 64);
            const int oi = __shfl_xor(bi, d, 64);
            if (oi < p.N && (bi == p.N || head_before(oc, oi, bc, bi))) {
                bc = oc;
                bi = oi;
            }
        }
        if (lane == 0) {
            sel_c[r & 1][w] = bc;
            sel_i[r & 1][w] = bi;
        }
        __syncthreads();                               // one barrier a round: the buffers alternate
        bc = sel_c[r & 1][0];
        bi = sel_i[r & 1][0];
#pragma unroll
        for (int g = 1; g < HEAD_WAVES; ++g) {
            const double oc = sel_c[r & 1][g];
            const int oi = sel_i[r & 1][g];
            if (oi < p.N && (bi == p.N || head_before(oc, oi, bc, bi))) {
                bc = oc;
                bi = oi;
            }
        }
        if (bi == p.N) break;                          // only NaN cosines are left (the same in every thread)
        tc = bc;
        ti = bi;
        if (li[0] == bi) {                             // the winner's thread: its next entry moves up
#pragma unroll
            for (int q = 0; q + 1 < HEAD_CAND; ++q) {
                lc[q] = lc[q + 1];
                li[q] = li[q + 1];
            }
            lc[HEAD_CAND - 1] = -INFINITY;
            li[HEAD_CAND - 1] = p.N;
        }
        if (t == 0) hard[(int64_t)b * p.width + r] = bi;
        nh = r + 1;
    }
    if (hard)
        for (int r = nh + t; r < p.width; r += HEAD_THREADS) hard[(int64_t)b * p.width + r] = -1;

    // pass 1: the largest logit, and the first class of the largest cosine
    double m = -INFINITY, cb = -INFINITY;
    int ib = p.N;
    for (int64_t j0 = t; j0 < p.N; j0 += HEAD_UNROLL * HEAD_THREADS) {
        double cu[HEAD_UNROLL];
        head_cosines(p, zr, j0, ix, cu);
#pragma unroll
        for (int u = 0; u < HEAD_UNROLL; ++u) {
            const int64_t j = j0 + (int64_t)u * HEAD_THREADS;
            if (j >= p.N) break;
            const double c = cu[u];
            const double l = head_logit(p, c, (int)j, valid && j == y, ly, nh, tc, ti);
            m = l > m ? l : m;
            if (c > cb) {                              // ascending j: the lowest index of a thread's classes stays
                cb = c;
                ib = (int)j;
            }
        }
    }
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
    for (int g = 1; g < HEAD_WAVES; ++g) {
        m = red_m[g] > m ? red_m[g] : m;
        if (red_c[g] > cb || (red_c[g] == cb && red_i[g] < ib)) {
            cb = red_c[g];
            ib = red_i[g];
        }
    }

    // pass 2: the row again (from the cache), the sums of H5
    const bool smooth = p.eps != 0.0;                  // H3: without smoothing the sum of the logits is not formed
    double s = 0.0, sl = 0.0;
    for (int64_t j0 = t; j0 < p.N; j0 += HEAD_UNROLL * HEAD_THREADS) {
        double cu[HEAD_UNROLL];
        head_cosines(p, zr, j0, ix, cu);
#pragma unroll
        for (int u = 0; u < HEAD_UNROLL; ++u) {
            const int64_t j = j0 + (int64_t)u * HEAD_THREADS;
            if (j >= p.N) break;
            const double l = head_logit(p, cu[u], (int)j, valid && j == y, ly, nh, tc, ti);
            s += exp(l - m);
            if (smooth) sl += l;
        }
    }
    s = head_wave_sum(s);
    if (smooth) sl = head_wave_sum(sl);
    if (lane == 0) {
        red_s[w] = s;
        red_l[w] = sl;
    }
    __syncthreads();
    if (t == 0) {
        double tot = red_s[0], totl = red_l[0];
#pragma unroll
        for (int g = 1; g < HEAD_WAVES; ++g) {
            tot += red_s[g];
            totl += red_l[g];
        }
        const double v = m + log(tot);
        lse[b] = v;
        double out = v - ly;
        if (smooth) out = out + p.eps * (ly - totl / (double)p.N);
        loss[b] = valid ? (float)out : 0.0f;
        if (pred) pred[b] = ib < p.N ? ib : 0;         // no class compares (every cosine NaN or -inf): 0
        if (sub_y) sub_y[b] = ky;
    }
}

// ------------------------------------------------------------------------------------ backward: (block of rows) x (chunk of classes)
__global__ __launch_bounds__(HEAD_THREADS) void head_backward_kernel(HeadParams p, const double* __restrict__ lse, const int32_t* __restrict__ hard,
                                                                    const float* __restrict__ gloss, float* dz, int64_t lddz, int nchunks,
                                                                    int nchunks_n, double* __restrict__ slots, double* __restrict__ rowpart) {
    __shared__ double red[HEAD_WAVES][HEAD_ROWS];
    __shared__ unsigned char member[HEAD_ROWS][HEAD_THREADS];   // H2: class j0 + t of row r is listed in `hard`
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int chunk = blockIdx.x % nchunks, slot = blockIdx.x / nchunks;
    const int64_t j0 = (int64_t)chunk * HEAD_THREADS, j = j0 + t;
    const int64_t col = j * p.K, ncols = (int64_t)p.N * p.K;
    const bool in = j < p.N, cosine = p.inv_x != nullptr;
    const int b0 = slot * HEAD_ROWS;

    if (p.topk > 0) {                                  // the same in every thread
#pragma unroll
        for (int r = 0; r < HEAD_ROWS; ++r) member[r][t] = 0;
        __syncthreads();
        for (int e = t; e < HEAD_ROWS * p.topk; e += HEAD_THREADS) {
            const int r = e / p.topk, i = e - r * p.topk;
            if (b0 + r < p.B) {
                const int64_t h = hard[(int64_t)(b0 + r) * p.width + i];
                if (h >= j0 && h < j0 + HEAD_THREADS) member[r][h - j0] = 1;
            }
        }
        __syncthreads();
    }

    // the selected centre of every row first: the loads are in flight together; a thread reads only the columns it writes (dz may be z)
    float zf[HEAD_ROWS];
    int ks[HEAD_ROWS], ys[HEAD_ROWS];
    double cs[HEAD_ROWS], ixs[HEAD_ROWS];
    {
        const double iw0 = (in && cosine) ? (double)p.inv_w[col] : 1.0;
#pragma unroll
        for (int r = 0; r < HEAD_ROWS; ++r) {
            const int b = b0 + r;
            ys[r] = -1;
            zf[r] = 0.0f;
            ks[r] = -1;
            cs[r] = 0.0;
            ixs[r] = 1.0;
            if (b < p.B) {
                const int y = p.labels[b];
                ys[r] = (y >= 0 && y < p.N) ? y : -1;
                if (ys[r] >= 0 && in) {
                    if (cosine) ixs[r] = (double)p.inv_x[b];
                    zf[r] = p.z[(int64_t)b * p.ldz + col];
                    ks[r] = 0;
                    cs[r] = cosine ? ((double)zf[r] * ixs[r]) * iw0 : (double)zf[r];
                }
            }
        }
    }
    for (int k = 1; k < p.K; ++k) {                    // K > 1 only with a cosine head; the rows' loads of a centre together
        const double iwk = in ? (double)p.inv_w[col + k] : 1.0;
#pragma unroll
        for (int r = 0; r < HEAD_ROWS; ++r) {
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
    double acc[HEAD_KMAX];                             // dinv_w[j * K + k] of this block of rows
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k) acc[k] = 0.0;
#pragma unroll
    for (int r = 0; r < HEAD_ROWS; ++r) {
        const int b = b0 + r;
        if (b >= p.B) {                                // the same in every thread
            if (lane == 0) red[w][r] = 0.0;
            continue;
        }
        float out = 0.0f;
        double rowterm = 0.0;
        if (ys[r] >= 0 && in) {
            const double ix = ixs[r];
            const double iw = cosine ? (double)p.inv_w[col + ks[r]] : 1.0;
            const double c = cs[r];
            const bool tgt = j == ys[r];
            double l;
            if (tgt)
                l = p.scale * head_psi(p, c);
            else if (p.topk > 0 && member[r][t])
                l = p.scale * (c + p.penalty);
            else
                l = p.scale * c;
            const double pj = exp(l - lse[b]);
            const double g = gloss ? (double)gloss[b] : 1.0;
            const double hot = tgt ? 1.0 : 0.0;
            double dc = (g * p.scale) * ((pj - hot) + p.eps * (hot - p.inv_n));
            if (tgt) dc = dc * head_dpsi(p, c);
            if (cosine) {
                out = (float)((dc * ix) * iw);
                const double dcz = dc * (double)zf[r];
                rowterm = dcz * iw;
                const double term = dcz * ix;
#pragma unroll
                for (int k = 0; k < HEAD_KMAX; ++k)
                    if (k == ks[r]) acc[k] += term;
            } else {
                out = (float)dc;
            }
        }
        float* dr = dz + (int64_t)b * lddz;
        if (in) {
            for (int k = 0; k < p.K; ++k) dr[col + k] = k == ks[r] ? out : 0.0f;
        } else {                                       // the pad columns: thread t takes K of the chunk's columns at and beyond N * K
            for (int k = 0; k < p.K; ++k)
                if (col + k < lddz) dr[col + k] = 0.0f;
        }
        if (cosine) {
            const double rs = head_wave_sum(rowterm);
            if (lane == 0) red[w][r] = rs;
        }
    }
    if (!cosine || chunk >= nchunks_n) return;         // the same in every thread
    if (in) {
#pragma unroll
        for (int k = 0; k < HEAD_KMAX; ++k)
            if (k < p.K) slots[(int64_t)slot * ncols + col + k] = acc[k];
    }
    __syncthreads();
    if (t < HEAD_ROWS && b0 + t < p.B) {
        double rs = red[0][t];
#pragma unroll
        for (int g = 1; g < HEAD_WAVES; ++g) rs += red[g][t];
        rowpart[(int64_t)chunk * p.B + b0 + t] = rs;
    }
}

// `count` partial sums `stride` doubles apart, added in ascending order, HEAD_FIN_BATCH loads in flight; terms past the last are +0.0
__device__ __forceinline__ double head_sum_strided(const double* __restrict__ first, int count, int64_t stride) {
    double sum = 0.0;
    for (int s0 = 0; s0 < count; s0 += HEAD_FIN_BATCH) {
        double v[HEAD_FIN_BATCH];
#pragma unroll
        for (int u = 0; u < HEAD_FIN_BATCH; ++u) v[u] = s0 + u < count ? first[(int64_t)(s0 + u) * stride] : 0.0;
#pragma unroll
        for (int u = 0; u < HEAD_FIN_BATCH; ++u) sum += v[u];
    }
    return sum;
}

// workgroups [0, col_blocks): dinv_w from the slots; the rest: dinv_x from the rows' sums per chunk
__global__ __launch_bounds__(HEAD_THREADS) void head_finalize_kernel(const double* __restrict__ slots, int nslots, const double* __restrict__ rowpart,
                                                                    int nchunks_n, int B, int64_t ncols, int col_blocks,
                                                                    float* __restrict__ dinv_x, float* __restrict__ dinv_w) {
    if ((int)blockIdx.x < col_blocks) {
        const int64_t j = (int64_t)blockIdx.x * HEAD_THREADS + threadIdx.x;
        if (j < ncols) dinv_w[j] = (float)head_sum_strided(slots + j, nslots, ncols);
    } else {
        const int64_t b = (int64_t)(blockIdx.x - col_blocks) * HEAD_THREADS + threadIdx.x;
        if (b < B) dinv_x[b] = (float)head_sum_strided(rowpart + b, nchunks_n, B);
    }
}

bool head_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na > 0 && nb > 0 && a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}

struct HeadSizes {
    int64_t nslots, nchunks, slot_bytes, bytes;
};

int head_sizes(const char* who, int64_t B, int64_t N, int64_t K, HeadSizes* s) {
    KTF_REQUIRE(B >= 0, "%s: negative size", who);
    KTF_REQUIRE(N >= 1, "%s: N %lld below 1", who, (long long)N);
    KTF_REQUIRE(K >= 1 && K <= KTF_HEAD_MAX_CENTERS, "%s: K %lld outside [1, %d]", who, (long long)K, KTF_HEAD_MAX_CENTERS);
    KTF_REQUIRE(B < (1ll << 31) && N < (1ll << 31) && N * K < (1ll << 31), "%s: B or N * K reaches 2^31", who);
    s->nslots = (B + KTF_HEAD_SLOT_ROWS - 1) / KTF_HEAD_SLOT_ROWS;
    s->nchunks = (N + KTF_HEAD_CHUNK_CLASSES - 1) / KTF_HEAD_CHUNK_CLASSES;
    KTF_REQUIRE(s->nslots * s->nchunks < (1ll << 31), "%s: batch too large for one grid (2^31 workgroups)", who);
    s->slot_bytes = al256((s->nslots > 0 ? s->nslots : 1) * N * K * 8);
    s->bytes = s->slot_bytes + al256(s->nchunks * (B > 0 ? B : 1) * 8);
    return KTF_OK;
}

// what both calls check alike (H7), and the constants of ktf_loss.h, rule 3
int head_check(const char* who, int64_t B, int64_t N, int64_t K, int64_t ldmin, int64_t ldmax, const float* inv_x, const float* inv_w,
               int32_t kind, double margin, double scale, int32_t topk, double penalty, double smoothing, const int32_t* hard,
               const void* workspace, size_t workspace_bytes, HeadSizes* s, HeadParams* p) {
    if (int rc = head_sizes(who, B, N, K, s)) return rc;
    KTF_REQUIRE(ldmin >= N * K, "%s: leading dimension %lld below N * K %lld", who, (long long)ldmin, (long long)(N * K));
    KTF_REQUIRE(ldmax < (1ll << 31), "%s: leading dimension reaches 2^31", who);
    KTF_REQUIRE((inv_x != nullptr) == (inv_w != nullptr), "%s: inv_x and inv_w go together (both for a cosine head, neither for a plain one)", who);
    KTF_REQUIRE(kind == KTF_LOSS_SOFTMAX || kind == KTF_LOSS_AM || kind == KTF_LOSS_AAM, "%s: unknown kind %d", who, (int)kind);
    KTF_REQUIRE(kind == KTF_LOSS_SOFTMAX || inv_x, "%s: a margin kind needs a cosine head (inv_x, inv_w)", who);
    KTF_REQUIRE(scale > 0.0 && scale < INFINITY, "%s: scale must be positive and finite", who);
    KTF_REQUIRE(margin >= 0.0 && margin < INFINITY, "%s: margin must be finite and not negative", who);
    KTF_REQUIRE(kind != KTF_LOSS_SOFTMAX || margin == 0.0, "%s: margin must be 0 for KTF_LOSS_SOFTMAX", who);
    KTF_REQUIRE(kind != KTF_LOSS_AAM || margin < 1.5707963267948966, "%s: margin must be below pi / 2 for KTF_LOSS_AAM", who);
    KTF_REQUIRE(K == 1 || inv_x, "%s: sub-centres (K > 1) need a cosine head (inv_x, inv_w)", who);
    KTF_REQUIRE(topk >= 0 && topk <= KTF_HEAD_MAX_TOPK, "%s: topk %d outside [0, %d]", who, (int)topk, KTF_HEAD_MAX_TOPK);
    KTF_REQUIRE(topk == 0 || inv_x, "%s: topk > 0 needs a cosine head (inv_x, inv_w)", who);
    KTF_REQUIRE(penalty >= 0.0 && penalty < INFINITY, "%s: penalty must be finite and not negative", who);
    KTF_REQUIRE(topk > 0 || penalty == 0.0, "%s: penalty must be 0 when topk is 0", who);
    KTF_REQUIRE(smoothing >= 0.0 && smoothing < 1.0, "%s: smoothing must be in [0, 1)", who);
    KTF_REQUIRE(topk == 0 || hard, "%s: null hard with topk > 0", who);
    KTF_REQUIRE(workspace, "%s: null argument", who);
    if (int rc = ktf_check_workspace(who, workspace, workspace_bytes, s->bytes)) return rc;
    p->B = (int)B;
    p->N = (int)N;
    p->K = (int)K;
    p->inv_x = inv_x;
    p->inv_w = inv_w;
    p->kind = kind;
    p->margin = margin;
    p->scale = scale;
    p->cm = cos(margin);
    p->sm = sin(margin);
    p->msm = margin * p->sm;
    p->topk = topk;
    p->width = topk > 1 ? topk : 1;
    p->penalty = penalty;
    p->eps = smoothing;
    p->inv_n = 1.0 / (double)N;
    return KTF_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------ entry points
extern "C" int32_t ktf_head_slot_rows(void) { return KTF_HEAD_SLOT_ROWS; }

extern "C" int64_t ktf_head_workspace_bytes(int64_t B, int64_t N, int64_t K) {
    HeadSizes s;
    if (int rc = head_sizes("ktf_head_workspace_bytes", B, N, K, &s)) return rc;
    return s.bytes;
}

extern "C" int ktf_head_forward(const float* z, int64_t ldz, int64_t B, int64_t N, int64_t K, const int32_t* labels, const float* inv_x,
                                const float* inv_w, int32_t kind, double margin, double scale, int32_t topk, double penalty,
                                double smoothing, float* loss, int32_t* pred, double* lse, int32_t* hard, int32_t* sub_y, void* workspace,
                                size_t workspace_bytes, void* stream) {
    const char* who = "ktf_head_forward";
    KTF_REQUIRE(z && labels && loss && lse, "%s: null argument", who);
    HeadSizes s;
    HeadParams p = {};
    if (int rc = head_check(who, B, N, K, ldz, ldz, inv_x, inv_w, kind, margin, scale, topk, penalty, smoothing, hard, workspace,
                            workspace_bytes, &s, &p))
        return rc;
    if (B == 0) return KTF_OK;
    p.z = z;
    p.ldz = ldz;
    p.labels = labels;
    hipLaunchKernelGGL(head_forward_kernel, dim3((unsigned)B), dim3(HEAD_THREADS), 0, (hipStream_t)stream, p, loss, pred, lse, hard, sub_y);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_head_backward(const float* z, int64_t ldz, int64_t B, int64_t N, int64_t K, const int32_t* labels, const float* inv_x,
                                 const float* inv_w, int32_t kind, double margin, double scale, int32_t topk, double penalty,
                                 double smoothing, const double* lse, const int32_t* hard, const float* gloss, float* dz, int64_t lddz,
                                 float* dinv_x, float* dinv_w, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_head_backward";
    KTF_REQUIRE(z && labels && lse && dz, "%s: null argument", who);
    HeadSizes s;
    HeadParams p = {};
    if (int rc = head_check(who, B, N, K, ldz < lddz ? ldz : lddz, ldz > lddz ? ldz : lddz, inv_x, inv_w, kind, margin, scale, topk, penalty,
                            smoothing, hard, workspace, workspace_bytes, &s, &p))
        return rc;
    KTF_REQUIRE((dinv_x != nullptr) == (inv_x != nullptr) && (dinv_w != nullptr) == (inv_w != nullptr),
                "%s: dinv_x and dinv_w go with a cosine head (both), not with a plain one (neither)", who);
    KTF_REQUIRE((z == dz && ldz == lddz) || !head_overlap(z, B > 0 ? (B - 1) * ldz + N * K : 0, dz, B * lddz),
                "%s: dz overlaps z (other than being z itself)", who);
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {                                      // H6: no kernel; the sum over no row
        if (dinv_w && hipMemsetAsync(dinv_w, 0, (size_t)(N * K) * 4, st) != hipSuccess) {
            ktf_set_error("%s: hipMemsetAsync failed", who);
            return KTF_ELAUNCH;
        }
        return KTF_OK;
    }
    p.z = z;
    p.ldz = ldz;
    p.labels = labels;
    double* slots = reinterpret_cast<double*>(workspace);
    double* rowpart = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + s.slot_bytes);
    const int64_t chunk_cols = (int64_t)KTF_HEAD_CHUNK_CLASSES * K;                     // the pad columns of dz are written too
    const int64_t nchunks = (lddz + chunk_cols - 1) / chunk_cols;
    KTF_REQUIRE(s.nslots * nchunks < (1ll << 31), "%s: batch too large for one grid (2^31 workgroups)", who);
    hipLaunchKernelGGL(head_backward_kernel, dim3((unsigned)(s.nslots * nchunks)), dim3(HEAD_THREADS), 0, st, p, lse, hard, gloss, dz, lddz,
                       (int)nchunks, (int)s.nchunks, slots, rowpart);
    KTF_CHECK_LAUNCH(who);
    if (inv_x) {
        const int64_t ncols = N * K;
        const int col_blocks = ktf_cdiv(ncols, HEAD_THREADS), row_blocks = ktf_cdiv(B, HEAD_THREADS);
        hipLaunchKernelGGL(head_finalize_kernel, dim3((unsigned)(col_blocks + row_blocks)), dim3(HEAD_THREADS), 0, st, slots, (int)s.nslots,
                           rowpart, (int)s.nchunks, (int)B, ncols, col_blocks, dinv_x, dinv_w);
        KTF_CHECK_LAUNCH(who);
    }
    return KTF_OK;
}
