// The classification head's loss in training (include/ktf_loss.h, whose rule numbers the comments use).
//   ktf_loss_row_inv_norm[_backward]    loss_inv_norm_kernel / loss_inv_norm_bwd_kernel: a wave per row
//   ktf_loss_margin_softmax_forward     loss_forward_kernel: a workgroup per row, two passes (maximum, then the sum of exponentials)
//   ktf_loss_margin_softmax_backward    loss_backward_kernel: a workgroup per (block of rows, chunk of columns), one pass that writes dz
//                                       and the partial sums of dinv_x and dinv_w -> loss_finalize_kernel adds them (cosine head only)
// One access pattern for every alignment (rule 8): a lane reads and writes one float, consecutive lanes consecutive columns. Every sum
// and every output value is fp64 arithmetic rounded once; the fp64 exponential per element is what these kernels spend their time on.
#include "common.h"
#include "../../include/ktf_loss.h"

// every fp64 operation is rounded on its own: no contraction into fma
#pragma clang fp contract(off)

namespace {

constexpr int LOSS_THREADS = KTF_LOSS_CHUNK_COLS;
constexpr int LOSS_WAVES = LOSS_THREADS / 64;
constexpr int LOSS_NORM_ROWS = 4;       // inverse norms: rows (waves) per workgroup
constexpr int LOSS_FIN_BATCH = 8;       // finalize: partial sums a thread has in flight

struct LossParams {
    const float* z;
    int64_t ldz;
    int B, N;
    const int32_t* labels;
    const float* inv_x;     // both NULL: plain head
    const float* inv_w;
    int kind;
    double margin, scale, cm, sm, msm;   // cos m, sin m, m * sin m (rule 3)
};

// the butterfly of rules N1 and 7: every lane ends with the same bits
__device__ __forceinline__ double loss_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

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
__global__ __launch_bounds__(LOSS_THREADS) void loss_forward_kernel(LossParams p, float* __restrict__ loss, int32_t* __restrict__ pred,
                                                                   double* __restrict__ lse) {
    __shared__ double red_m[LOSS_WAVES], red_c[LOSS_WAVES], red_s[LOSS_WAVES];
    __shared__ int red_i[LOSS_WAVES];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const float* __restrict__ zr = p.z + (int64_t)b * p.ldz;
    const int y = p.labels[b];
    const bool valid = y >= 0 && y < p.N;
    const double ix = p.inv_x ? (double)p.inv_x[b] : 1.0;
    double ly = 0.0;
    if (valid) ly = p.scale * loss_psi(p, loss_cosine(p, zr[y], ix, p.inv_w ? (double)p.inv_w[y] : 1.0));

    // pass 1: the largest logit, and the first column of the largest cosine
    double m = -INFINITY, cb = -INFINITY;
    int ib = p.N;
#pragma unroll 4
    for (int64_t j = t; j < p.N; j += LOSS_THREADS) {
        const double c = loss_cosine(p, zr[j], ix, p.inv_w ? (double)p.inv_w[j] : 1.0);
        const double l = (valid && j == y) ? ly : p.scale * c;
        m = l > m ? l : m;
        if (c > cb) {                                  // ascending j: the lowest index of a thread's columns stays
            cb = c;
            ib = (int)j;
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
    for (int g = 1; g < LOSS_WAVES; ++g) {
        m = red_m[g] > m ? red_m[g] : m;
        if (red_c[g] > cb || (red_c[g] == cb && red_i[g] < ib)) {
            cb = red_c[g];
            ib = red_i[g];
        }
    }

    // pass 2: the row again (from the cache), the sum of rule 7
    double s = 0.0;
#pragma unroll 4
    for (int64_t j = t; j < p.N; j += LOSS_THREADS) {
        const double c = loss_cosine(p, zr[j], ix, p.inv_w ? (double)p.inv_w[j] : 1.0);
        const double l = (valid && j == y) ? ly : p.scale * c;
        s += exp(l - m);
    }
    s = loss_wave_sum(s);
    if (lane == 0) red_s[w] = s;
    __syncthreads();
    if (t == 0) {
        double tot = red_s[0];
#pragma unroll
        for (int g = 1; g < LOSS_WAVES; ++g) tot += red_s[g];
        const double v = m + log(tot);
        lse[b] = v;
        loss[b] = valid ? (float)(v - ly) : 0.0f;
        if (pred) pred[b] = ib < p.N ? ib : 0;         // no column compares (every cosine NaN or -inf): 0
    }
}

// ------------------------------------------------------------------------------------ backward: (block of rows) x (chunk of columns)
__global__ __launch_bounds__(LOSS_THREADS) void loss_backward_kernel(LossParams p, const double* __restrict__ lse, const float* __restrict__ gloss,
                                                                    float* dz, int64_t lddz, int nchunks, int nchunks_n,
                                                                    double* __restrict__ slots, double* __restrict__ rowpart) {
    __shared__ double red[LOSS_WAVES][KTF_LOSS_SLOT_ROWS];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int chunk = blockIdx.x % nchunks, slot = blockIdx.x / nchunks;
    const int64_t j = (int64_t)chunk * LOSS_THREADS + t;
    const bool in = j < p.N, cosine = p.inv_x != nullptr;
    const double iw = (in && cosine) ? (double)p.inv_w[j] : 1.0;
    const int b0 = slot * KTF_LOSS_SLOT_ROWS;

    // every load of z before the first store of dz: dz may be z
    float zf[KTF_LOSS_SLOT_ROWS];
    int ys[KTF_LOSS_SLOT_ROWS];
#pragma unroll
    for (int r = 0; r < KTF_LOSS_SLOT_ROWS; ++r) {
        const int b = b0 + r;
        ys[r] = -1;
        zf[r] = 0.0f;
        if (b < p.B) {
            const int y = p.labels[b];
            ys[r] = (y >= 0 && y < p.N) ? y : -1;
            if (ys[r] >= 0 && in) zf[r] = p.z[(int64_t)b * p.ldz + j];
        }
    }
    double acc = 0.0;                                  // dinv_w[j] of this block of rows
#pragma unroll
    for (int r = 0; r < KTF_LOSS_SLOT_ROWS; ++r) {
        const int b = b0 + r;
        if (b >= p.B) {                                // the same in every thread
            if (lane == 0) red[w][r] = 0.0;
            continue;
        }
        float out = 0.0f;
        double rowterm = 0.0;
        if (ys[r] >= 0 && in) {
            const double ix = cosine ? (double)p.inv_x[b] : 1.0;
            const double c = loss_cosine(p, zf[r], ix, iw);
            const bool tgt = j == ys[r];
            const double l = p.scale * (tgt ? loss_psi(p, c) : c);
            const double pj = exp(l - lse[b]);
            const double g = gloss ? (double)gloss[b] : 1.0;
            double dc = (g * p.scale) * (pj - (tgt ? 1.0 : 0.0));
            if (tgt) dc = dc * loss_dpsi(p, c);
            if (cosine) {
                out = (float)((dc * ix) * iw);
                const double dcz = dc * (double)zf[r];
                rowterm = dcz * iw;
                acc += dcz * ix;
            } else {
                out = (float)dc;
            }
        }
        if (j < lddz) dz[(int64_t)b * lddz + j] = out;
        if (cosine) {
            const double rs = loss_wave_sum(rowterm);
            if (lane == 0) red[w][r] = rs;
        }
    }
    if (!cosine || chunk >= nchunks_n) return;         // the same in every thread
    if (in) slots[(int64_t)slot * p.N + j] = acc;
    __syncthreads();
    if (t < KTF_LOSS_SLOT_ROWS && b0 + t < p.B) {
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

// workgroups [0, col_blocks): dinv_w from the slots; the rest: dinv_x from the rows' sums per chunk
__global__ __launch_bounds__(LOSS_THREADS) void loss_finalize_kernel(const double* __restrict__ slots, int nslots, const double* __restrict__ rowpart,
                                                                    int nchunks_n, int B, int N, int col_blocks, float* __restrict__ dinv_x,
                                                                    float* __restrict__ dinv_w) {
    if ((int)blockIdx.x < col_blocks) {
        const int64_t j = (int64_t)blockIdx.x * LOSS_THREADS + threadIdx.x;
        if (j < N) dinv_w[j] = (float)loss_sum_strided(slots + j, nslots, N);
    } else {
        const int64_t b = (int64_t)(blockIdx.x - col_blocks) * LOSS_THREADS + threadIdx.x;
        if (b < B) dinv_x[b] = (float)loss_sum_strided(rowpart + b, nchunks_n, B);
    }
}

bool loss_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na > 0 && nb > 0 && a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}

struct LossSizes {
    int64_t nslots, nchunks, slot_bytes, bytes;
};

int loss_sizes(const char* who, int64_t B, int64_t N, LossSizes* s) {
    KTF_REQUIRE(B >= 0, "%s: negative size", who);
    KTF_REQUIRE(N >= 1, "%s: N %lld below 1", who, (long long)N);
    KTF_REQUIRE(B < (1ll << 31) && N < (1ll << 31), "%s: B or N reaches 2^31", who);
    s->nslots = (B + KTF_LOSS_SLOT_ROWS - 1) / KTF_LOSS_SLOT_ROWS;
    s->nchunks = (N + KTF_LOSS_CHUNK_COLS - 1) / KTF_LOSS_CHUNK_COLS;
    KTF_REQUIRE(s->nslots * s->nchunks < (1ll << 31), "%s: batch too large for one grid (2^31 workgroups)", who);
    s->slot_bytes = al256((s->nslots > 0 ? s->nslots : 1) * N * 8);
    s->bytes = s->slot_bytes + al256(s->nchunks * (B > 0 ? B : 1) * 8);
    return KTF_OK;
}

// what both loss calls check alike, and the constants of rule 3
int loss_check(const char* who, int64_t B, int64_t N, int64_t ldmin, int64_t ldmax, const float* inv_x, const float* inv_w, int32_t kind,
               double margin, double scale, const void* workspace, size_t workspace_bytes, LossSizes* s, LossParams* p) {
    if (int rc = loss_sizes(who, B, N, s)) return rc;
    KTF_REQUIRE(ldmin >= N, "%s: leading dimension %lld below N %lld", who, (long long)ldmin, (long long)N);
    KTF_REQUIRE(ldmax < (1ll << 31), "%s: leading dimension reaches 2^31", who);
    KTF_REQUIRE((inv_x != nullptr) == (inv_w != nullptr), "%s: inv_x and inv_w go together (both for a cosine head, neither for a plain one)", who);
    KTF_REQUIRE(kind == KTF_LOSS_SOFTMAX || kind == KTF_LOSS_AM || kind == KTF_LOSS_AAM, "%s: unknown kind %d", who, (int)kind);
    KTF_REQUIRE(kind == KTF_LOSS_SOFTMAX || inv_x, "%s: a margin kind needs a cosine head (inv_x, inv_w)", who);
    KTF_REQUIRE(scale > 0.0 && scale < INFINITY, "%s: scale must be positive and finite", who);
    KTF_REQUIRE(margin >= 0.0 && margin < INFINITY, "%s: margin must be finite and not negative", who);
    KTF_REQUIRE(kind != KTF_LOSS_SOFTMAX || margin == 0.0, "%s: margin must be 0 for KTF_LOSS_SOFTMAX", who);
    KTF_REQUIRE(kind != KTF_LOSS_AAM || margin < 1.5707963267948966, "%s: margin must be below pi / 2 for KTF_LOSS_AAM", who);
    KTF_REQUIRE(workspace, "%s: null argument", who);
    if (int rc = ktf_check_workspace(who, workspace, workspace_bytes, s->bytes)) return rc;
    p->B = (int)B;
    p->N = (int)N;
    p->inv_x = inv_x;
    p->inv_w = inv_w;
    p->kind = kind;
    p->margin = margin;
    p->scale = scale;
    p->cm = cos(margin);
    p->sm = sin(margin);
    p->msm = margin * p->sm;
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

extern "C" int64_t ktf_loss_workspace_bytes(int64_t B, int64_t N) {
    LossSizes s;
    if (int rc = loss_sizes("ktf_loss_workspace_bytes", B, N, &s)) return rc;
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

extern "C" int ktf_loss_margin_softmax_forward(const float* z, int64_t ldz, int64_t B, int64_t N, const int32_t* labels, const float* inv_x,
                                               const float* inv_w, int32_t kind, double margin, double scale, float* loss, int32_t* pred,
                                               double* lse, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_loss_margin_softmax_forward";
    KTF_REQUIRE(z && labels && loss && lse, "%s: null argument", who);
    LossSizes s;
    LossParams p = {};
    if (int rc = loss_check(who, B, N, ldz, ldz, inv_x, inv_w, kind, margin, scale, workspace, workspace_bytes, &s, &p)) return rc;
    if (B == 0) return KTF_OK;
    p.z = z;
    p.ldz = ldz;
    p.labels = labels;
    hipLaunchKernelGGL(loss_forward_kernel, dim3((unsigned)B), dim3(LOSS_THREADS), 0, (hipStream_t)stream, p, loss, pred, lse);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_loss_margin_softmax_backward(const float* z, int64_t ldz, int64_t B, int64_t N, const int32_t* labels, const float* inv_x,
                                                const float* inv_w, int32_t kind, double margin, double scale, const double* lse,
                                                const float* gloss, float* dz, int64_t lddz, float* dinv_x, float* dinv_w, void* workspace,
                                                size_t workspace_bytes, void* stream) {
    const char* who = "ktf_loss_margin_softmax_backward";
    KTF_REQUIRE(z && labels && lse && dz, "%s: null argument", who);
    LossSizes s;
    LossParams p = {};
    if (int rc = loss_check(who, B, N, ldz < lddz ? ldz : lddz, ldz > lddz ? ldz : lddz, inv_x, inv_w, kind, margin, scale, workspace,
                            workspace_bytes, &s, &p))
        return rc;
    KTF_REQUIRE((dinv_x != nullptr) == (inv_x != nullptr) && (dinv_w != nullptr) == (inv_w != nullptr),
                "%s: dinv_x and dinv_w go with a cosine head (both), not with a plain one (neither)", who);
    KTF_REQUIRE((z == dz && ldz == lddz) || !loss_overlap(z, B > 0 ? (B - 1) * ldz + N : 0, dz, B * lddz),
                "%s: dz overlaps z (other than being z itself)", who);
    hipStream_t st = (hipStream_t)stream;
    if (B == 0) {                                      // rule 9: no kernel; the sum over no row
        if (dinv_w && hipMemsetAsync(dinv_w, 0, (size_t)N * 4, st) != hipSuccess) {
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
    const int64_t nchunks = (lddz + KTF_LOSS_CHUNK_COLS - 1) / KTF_LOSS_CHUNK_COLS;      // the pad columns of dz are written too
    KTF_REQUIRE(s.nslots * nchunks < (1ll << 31), "%s: batch too large for one grid (2^31 workgroups)", who);
    hipLaunchKernelGGL(loss_backward_kernel, dim3((unsigned)(s.nslots * nchunks)), dim3(LOSS_THREADS), 0, st, p, lse, gloss, dz, lddz,
                       (int)nchunks, (int)s.nchunks, slots, rowpart);
    KTF_CHECK_LAUNCH(who);
    if (inv_x) {
        const int col_blocks = (int)s.nchunks, row_blocks = ktf_cdiv(B, LOSS_THREADS);
        hipLaunchKernelGGL(loss_finalize_kernel, dim3((unsigned)(col_blocks + row_blocks)), dim3(LOSS_THREADS), 0, st, slots, (int)s.nslots,
                           rowpart, (int)s.nchunks, (int)B, (int)N, col_blocks, dinv_x, dinv_w);
        KTF_CHECK_LAUNCH(who);
    }
    return KTF_OK;
}
