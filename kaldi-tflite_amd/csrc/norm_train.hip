// ReLU + batch normalisation in training, forward and backward (include/ktf_norm.h, whose rule numbers the comments use).
//   ktf_norm_relu_bn_forward    norm_stats_kernel<.., false> -> norm_fwd_finalize_kernel -> norm_apply_kernel<.., false>
//   ktf_norm_relu_bn_backward   norm_stats_kernel<.., true>  -> norm_bwd_finalize_kernel -> norm_apply_kernel<.., true>
// Rows across workgroups, columns across lanes: a workgroup takes NORM_COLS columns (64 lanes x 4) of a block of rows, its waves
// take the block's rows round robin. Memory bound: the forward reads z twice and writes y once, the backward reads gy and z twice
// each and writes dz once; every sum and every output value is fp64 arithmetic rounded once.
#include "common.h"
#include "../../include/ktf_norm.h"

// every fp64 operation is rounded on its own (rules 1, 3, 4): no contraction into fma
#pragma clang fp contract(off)

namespace {

constexpr int NORM_COLS = 256;          // columns per workgroup: 64 lanes x 4
constexpr int NORM_STAT_WAVES = 8;      // statistics pass: the groups of rule 5
constexpr int NORM_STAT_UNROLL = 4;     // ... rows a wave has in flight
constexpr int NORM_APPLY_WAVES = 4;     // normalise pass
constexpr int NORM_APPLY_ROWS = 32;     // ... rows per workgroup, all of a wave's 8 in flight

struct NormParams {
    const float* z;
    const float* gy;        // backward only
    float* out;             // y / dz
    int64_t ldz, ldg, ldo;
    int rows, T, D, nchunks, nslots;
    const int32_t* lens;
    int relu, training;
    const float* gamma;
    const double* saved;    // (2, D): mean, invstd
    double* slots;          // (nslots, 2, D)
    double* tot;            // backward: s1 / n, s2 / n (2, D)
};

// columns of lane `lane` in a chunk: four neighbours for the 16-byte path, four strided by the wave for the scalar one
template <bool VEC>
__device__ __forceinline__ int norm_col(int lane, int j) { return VEC ? lane * 4 + j : j * 64 + lane; }

__device__ __forceinline__ bool norm_row_valid(const NormParams& p, int r) {
    if (r >= p.rows) return false;
    if (!p.lens) return true;
    const int b = r / p.T;
    int len = p.lens[b];
    len = len > p.T ? p.T : len;
    return r - b * p.T < len;
}

// four columns of row `row` (columns at and beyond D are not read: zero)
template <bool VEC>
__device__ __forceinline__ void norm_load4(const float* __restrict__ row, int c0, int lane, int D, float v[4]) {
    if (VEC && c0 + lane * 4 + 4 <= D) {
        const float4 q = *reinterpret_cast<const float4*>(row + c0 + lane * 4);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + norm_col<VEC>(lane, j);
            v[j] = c < D ? row[c] : 0.0f;
        }
    }
}

// four columns of an output row of `ld` elements
template <bool VEC>
__device__ __forceinline__ void norm_store4(float* __restrict__ row, int c0, int lane, int64_t ld, const float v[4]) {
    if (VEC) {
        if (c0 + lane * 4 < ld) *reinterpret_cast<float4*>(row + c0 + lane * 4) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + norm_col<VEC>(lane, j);
            if (c < ld) row[c] = v[j];
        }
    }
}

// ------------------------------------------------------------------------------------ pass 1: partial sums of one slot
// Forward: sum a, sum a^2. Backward: sum gy, sum gy * ahat. Wave w adds the slot's rows w, w + 8, ... in ascending order; the eight
// waves are then added in ascending order through LDS.
template <bool VEC, bool BWD>
__global__ __launch_bounds__(NORM_STAT_WAVES * 64) void norm_stats_kernel(NormParams p) {
    __shared__ double red[NORM_STAT_WAVES][2][NORM_COLS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int chunk = blockIdx.x % p.nchunks, slot = blockIdx.x / p.nchunks;
    const int c0 = chunk * NORM_COLS;
    const int r0 = slot * KTF_NORM_SLOT_ROWS;
    double mean[4], inv[4];
    if (BWD) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + norm_col<VEC>(lane, j);
            mean[j] = c < p.D ? p.saved[c] : 0.0;
            inv[j] = c < p.D ? p.saved[p.D + c] : 0.0;
        }
    }
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = w; i < KTF_NORM_SLOT_ROWS; i += NORM_STAT_WAVES * NORM_STAT_UNROLL) {
        float vz[NORM_STAT_UNROLL][4], vg[NORM_STAT_UNROLL][4];
        bool ok[NORM_STAT_UNROLL];
#pragma unroll
        for (int u = 0; u < NORM_STAT_UNROLL; ++u) {
            const int r = r0 + i + u * NORM_STAT_WAVES;
            ok[u] = norm_row_valid(p, r);                 // the same in every lane
            if (ok[u]) {
                norm_load4<VEC>(p.z + (int64_t)r * p.ldz, c0, lane, p.D, vz[u]);
                if (BWD) norm_load4<VEC>(p.gy + (int64_t)r * p.ldg, c0, lane, p.D, vg[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < NORM_STAT_UNROLL; ++u) {
            if (!ok[u]) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float zf = vz[u][j];
                const double a = (double)((p.relu && !(zf > 0.0f)) ? 0.0f : zf);
                if (BWD) {
                    const double g = (double)vg[u][j];
                    s[j] += g;
                    q[j] += g * ((a - mean[j]) * inv[j]);
                } else {
                    s[j] += a;
                    q[j] += a * a;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[w][0][norm_col<VEC>(lane, j)] = s[j];
        red[w][1][norm_col<VEC>(lane, j)] = q[j];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * NORM_COLS; i += NORM_STAT_WAVES * 64) {
        const int k = i / NORM_COLS, lc = i % NORM_COLS;
        if (c0 + lc >= p.D) continue;
        double t = red[0][k][lc];
#pragma unroll
        for (int g = 1; g < NORM_STAT_WAVES; ++g) t += red[g][k][lc];
        p.slots[((int64_t)slot * 2 + k) * p.D + c0 + lc] = t;
    }
}

// The slots of NORM_FIN_COLS columns from c0 on, added in ascending order; all NORM_FIN_THREADS threads of the workgroup call it and
// thread tid < NORM_FIN_COLS gets the two sums of column c0 + tid. A column's slots lie 2 D doubles apart and a chain of dependent
// loads would cost a memory latency each, so the workgroup fetches NORM_FIN_TILE slots at a time, eight per thread in flight, into
// LDS, and one thread per (column, sum) adds them from there. Slots past the last are staged as +0.0, which changes no sum.
constexpr int NORM_FIN_COLS = 32;
constexpr int NORM_FIN_TILE = 64;
constexpr int NORM_FIN_THREADS = 256;

__device__ __forceinline__ void norm_sum_slots(const double* __restrict__ slots, int nslots, int D, int c0,
                                               double (*stage)[2][NORM_FIN_COLS], double& S1, double& S2) {
    constexpr int GROUPS = NORM_FIN_THREADS / NORM_FIN_COLS, PER = NORM_FIN_TILE / GROUPS;
    const int tid = threadIdx.x, cl = tid % NORM_FIN_COLS, sg = tid / NORM_FIN_COLS;
    const int c = c0 + cl;
    double sum = 0.0;                                  // tid < 2 * NORM_FIN_COLS: sum tid / NORM_FIN_COLS of column cl
    for (int s0 = 0; s0 < nslots; s0 += NORM_FIN_TILE) {
        double v[PER][2];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int s = s0 + sg + u * GROUPS;
            const bool ok = s < nslots && c < D;
            v[u][0] = ok ? slots[((int64_t)s * 2) * D + c] : 0.0;
            v[u][1] = ok ? slots[((int64_t)s * 2 + 1) * D + c] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            stage[sg + u * GROUPS][0][cl] = v[u][0];
            stage[sg + u * GROUPS][1][cl] = v[u][1];
        }
        __syncthreads();
        if (tid < 2 * NORM_FIN_COLS) {
#pragma unroll 8
            for (int j = 0; j < NORM_FIN_TILE; ++j) sum += stage[j][sg][cl];
        }
        __syncthreads();
    }
    const double other = __shfl_xor(sum, NORM_FIN_COLS, 64);   // the first wave holds both sums of a column, 32 lanes apart
    S1 = sum;
    S2 = other;
}

// n of rule 1 (below 2^31: B * T is)
__device__ __forceinline__ int norm_count(const int32_t* __restrict__ lens, int B, int T) {
    if (!lens) return B * T;
    int n = 0;
    for (int b = 0; b < B; ++b) {
        const int len = lens[b];
        n += len < 0 ? 0 : (len > T ? T : len);
    }
    return n;
}

// ------------------------------------------------------------------------------------ pass 2: slots -> per-feature constants
__global__ __launch_bounds__(NORM_FIN_THREADS) void norm_fwd_finalize_kernel(const double* __restrict__ slots, int nslots, int D,
                                                                             const int32_t* __restrict__ lens, int B, int T, int training,
                                                                             float* __restrict__ moving_mean, float* __restrict__ moving_var,
                                                                             double momentum, double eps, double* __restrict__ saved) {
    __shared__ double stage[NORM_FIN_TILE][2][NORM_FIN_COLS];
    const int n = norm_count(lens, B, T);
    double S1 = 0.0, S2 = 0.0;
    if (training && n > 0) norm_sum_slots(slots, nslots, D, blockIdx.x * NORM_FIN_COLS, stage, S1, S2);   // the same for the whole grid
    const int c = blockIdx.x * NORM_FIN_COLS + threadIdx.x;
    if (threadIdx.x >= NORM_FIN_COLS || c >= D) return;
    if (n == 0) {                                      // rule 7
        saved[c] = 0.0;
        saved[D + c] = 0.0;
        return;
    }
    double mean, var;
    if (training) {
        mean = S1 / (double)n;
        var = S2 / (double)n - mean * mean;
        var = var > 0.0 ? var : 0.0;
        moving_mean[c] = (float)((double)moving_mean[c] * momentum + mean * (1.0 - momentum));
        moving_var[c] = (float)((double)moving_var[c] * momentum + var * (1.0 - momentum));
    } else {
        mean = (double)moving_mean[c];
        var = (double)moving_var[c];
    }
    saved[c] = mean;
    saved[D + c] = 1.0 / sqrt(var + eps);
}

__global__ __launch_bounds__(NORM_FIN_THREADS) void norm_bwd_finalize_kernel(const double* __restrict__ slots, int nslots, int D,
                                                                             const int32_t* __restrict__ lens, int B, int T,
                                                                             double* __restrict__ tot, float* __restrict__ dgamma) {
    __shared__ double stage[NORM_FIN_TILE][2][NORM_FIN_COLS];
    const int n = norm_count(lens, B, T);
    double S1, S2;
    norm_sum_slots(slots, nslots, D, blockIdx.x * NORM_FIN_COLS, stage, S1, S2);     // n = 0: no valid row, every slot holds zero
    const int c = blockIdx.x * NORM_FIN_COLS + threadIdx.x;
    if (threadIdx.x >= NORM_FIN_COLS || c >= D) return;
    tot[c] = n > 0 ? S1 / (double)n : 0.0;
    tot[D + c] = n > 0 ? S2 / (double)n : 0.0;
    if (dgamma) dgamma[c] = (float)S2;
}

// ------------------------------------------------------------------------------------ pass 3: y / dz
template <bool VEC, bool BWD>
__global__ __launch_bounds__(NORM_APPLY_WAVES * 64) void norm_apply_kernel(NormParams p) {
    constexpr int PER_WAVE = NORM_APPLY_ROWS / NORM_APPLY_WAVES;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int chunk = blockIdx.x % p.nchunks;
    const int c0 = chunk * NORM_COLS;
    const int r0 = (blockIdx.x / p.nchunks) * NORM_APPLY_ROWS;
    double mean[4], inv[4], gam[4], c1[4], c2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = c0 + norm_col<VEC>(lane, j);
        const bool in = c < p.D;
        mean[j] = in ? p.saved[c] : 0.0;
        inv[j] = in ? p.saved[p.D + c] : 0.0;
        gam[j] = in ? (double)p.gamma[c] : 0.0;
        c1[j] = (BWD && in && p.training) ? p.tot[c] : 0.0;
        c2[j] = (BWD && in && p.training) ? p.tot[p.D + c] : 0.0;
    }
    float vz[PER_WAVE][4], vg[PER_WAVE][4];
    bool ok[PER_WAVE];
#pragma unroll
    for (int u = 0; u < PER_WAVE; ++u) {
        const int r = r0 + w + u * NORM_APPLY_WAVES;
        ok[u] = norm_row_valid(p, r);
        if (ok[u]) {
            norm_load4<VEC>(p.z + (int64_t)r * p.ldz, c0, lane, p.D, vz[u]);
            if (BWD) norm_load4<VEC>(p.gy + (int64_t)r * p.ldg, c0, lane, p.D, vg[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < PER_WAVE; ++u) {
        const int r = r0 + w + u * NORM_APPLY_WAVES;
        if (r >= p.rows) continue;
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (ok[u]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (c0 + norm_col<VEC>(lane, j) >= p.D) continue;
                const float zf = vz[u][j];
                const bool off = p.relu && !(zf > 0.0f);
                const double a = (double)(off ? 0.0f : zf);
                if (!BWD) {
                    o[j] = (float)(((a - mean[j]) * gam[j]) * inv[j]);
                } else if (!off) {
                    const double g = (double)vg[u][j];
                    const double k = gam[j] * inv[j];
                    o[j] = p.training ? (float)(k * ((g - c1[j]) - ((a - mean[j]) * inv[j]) * c2[j])) : (float)(k * g);
                }
            }
        }
        norm_store4<VEC>(p.out + (int64_t)r * p.ldo, c0, lane, p.ldo, o);
    }
}

bool norm_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return na > 0 && nb > 0 && a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}

struct NormSizes {
    int64_t rows, nslots, slot_bytes, bytes;
};

int norm_sizes(const char* who, int64_t B, int64_t T, int32_t D, NormSizes* s) {
    KTF_REQUIRE(B >= 0 && T >= 0, "%s: negative size", who);
    KTF_REQUIRE(D >= 1, "%s: D %d below 1", who, (int)D);
    KTF_REQUIRE(B < (1ll << 31) && T < (1ll << 31) && B * T < (1ll << 31), "%s: B * T reaches 2^31", who);
    s->rows = B * T;
    s->nslots = (s->rows + KTF_NORM_SLOT_ROWS - 1) / KTF_NORM_SLOT_ROWS;
    s->slot_bytes = al256((s->nslots > 0 ? s->nslots : 1) * 2 * (int64_t)D * 8);
    s->bytes = s->slot_bytes + al256((2 * (int64_t)D + 1) * 8);
    return KTF_OK;
}

// sizes, strides, the workspace and the grids of both calls; `maxld` the largest leading dimension of the call
int norm_check(const char* who, int64_t B, int64_t T, int32_t D, int64_t ldmin, int64_t maxld, const void* workspace, size_t workspace_bytes,
               NormSizes* s) {
    if (int rc = norm_sizes(who, B, T, D, s)) return rc;
    KTF_REQUIRE(ldmin >= D, "%s: leading dimension %lld below D %d", who, (long long)ldmin, (int)D);
    KTF_REQUIRE(workspace, "%s: null argument", who);
    if (int rc = ktf_check_workspace(who, workspace, workspace_bytes, s->bytes)) return rc;
    const int64_t chunks = (maxld + NORM_COLS - 1) / NORM_COLS;
    const int64_t blocks = (s->rows + NORM_APPLY_ROWS - 1) / NORM_APPLY_ROWS;
    KTF_REQUIRE(maxld < (1ll << 30) && chunks * blocks < (1ll << 31), "%s: batch too large for one grid", who);
    return KTF_OK;
}

bool norm_vec(std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> lds) {
    for (const void* q : ptrs)
        if ((uintptr_t)q & 15) return false;
    for (int64_t ld : lds)
        if (ld % 4) return false;
    return true;
}

}  // namespace

// ------------------------------------------------------------------------------------ entry points
extern "C" int32_t ktf_norm_slot_rows(void) { return KTF_NORM_SLOT_ROWS; }

extern "C" int64_t ktf_norm_workspace_bytes(int64_t B, int64_t T, int32_t D) {
    NormSizes s;
    if (int rc = norm_sizes("ktf_norm_workspace_bytes", B, T, D, &s)) return rc;
    return s.bytes;
}

extern "C" int ktf_norm_relu_bn_forward(const float* z, int64_t ldz, int64_t B, int64_t T, int32_t D, const int32_t* lens, int32_t relu,
                                        int32_t training, const float* gamma, float* moving_mean, float* moving_var, double momentum,
                                        double eps, float* y, int64_t ldy, double* saved, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    const char* who = "ktf_norm_relu_bn_forward";
    KTF_REQUIRE(z && gamma && moving_mean && moving_var && y && saved, "%s: null argument", who);
    KTF_REQUIRE(eps > 0.0 && eps < INFINITY, "%s: eps must be positive and finite", who);
    KTF_REQUIRE(momentum >= 0.0 && momentum <= 1.0, "%s: momentum outside [0, 1]", who);
    NormSizes s;
    if (int rc = norm_check(who, B, T, D, ldz < ldy ? ldz : ldy, ldz > ldy ? ldz : ldy, workspace, workspace_bytes, &s)) return rc;
    KTF_REQUIRE(!norm_overlap(z, s.rows * ldz, y, s.rows * ldy), "%s: y overlaps z (the backward call reads z again)", who);
    hipStream_t st = (hipStream_t)stream;
    NormParams p = {};
    p.z = z; p.out = y; p.ldz = ldz; p.ldo = ldy;
    p.rows = (int)s.rows; p.T = (int)T; p.D = D; p.nslots = (int)s.nslots;
    p.lens = lens; p.relu = relu != 0; p.training = training != 0; p.gamma = gamma; p.saved = saved;
    p.slots = reinterpret_cast<double*>(workspace);
    const bool vec = norm_vec({z, y}, {ldz, ldy});
    if (p.training && s.nslots > 0) {
        p.nchunks = ktf_cdiv(D, NORM_COLS);
        const dim3 grid((unsigned)(s.nslots * p.nchunks));
        if (vec) hipLaunchKernelGGL((norm_stats_kernel<true, false>), grid, dim3(NORM_STAT_WAVES * 64), 0, st, p);
        else hipLaunchKernelGGL((norm_stats_kernel<false, false>), grid, dim3(NORM_STAT_WAVES * 64), 0, st, p);
        KTF_CHECK_LAUNCH(who);
    }
    hipLaunchKernelGGL(norm_fwd_finalize_kernel, dim3((unsigned)ktf_cdiv(D, NORM_FIN_COLS)), dim3(NORM_FIN_THREADS), 0, st, p.slots,
                       p.nslots, D, lens, (int)B, (int)T, p.training, moving_mean, moving_var, momentum, eps, saved);
    KTF_CHECK_LAUNCH(who);
    if (s.rows > 0) {
        p.nchunks = ktf_cdiv(ldy, NORM_COLS);
        const dim3 grid((unsigned)(ktf_cdiv(s.rows, NORM_APPLY_ROWS) * (int64_t)p.nchunks));
        if (vec) hipLaunchKernelGGL((norm_apply_kernel<true, false>), grid, dim3(NORM_APPLY_WAVES * 64), 0, st, p);
        else hipLaunchKernelGGL((norm_apply_kernel<false, false>), grid, dim3(NORM_APPLY_WAVES * 64), 0, st, p);
        KTF_CHECK_LAUNCH(who);
    }
    return KTF_OK;
}

extern "C" int ktf_norm_relu_bn_backward(const float* gy, int64_t ldg, const float* z, int64_t ldz, int64_t B, int64_t T, int32_t D,
                                         const int32_t* lens, int32_t relu, int32_t training, const float* gamma, const double* saved,
                                         float* dz, int64_t ld_dz, float* dgamma, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_norm_relu_bn_backward";
    KTF_REQUIRE(gy && z && gamma && saved && dz, "%s: null argument", who);
    NormSizes s;
    const int64_t ldmin = ldg < ldz ? (ldg < ld_dz ? ldg : ld_dz) : (ldz < ld_dz ? ldz : ld_dz);
    const int64_t ldmax = ldg > ldz ? (ldg > ld_dz ? ldg : ld_dz) : (ldz > ld_dz ? ldz : ld_dz);
    if (int rc = norm_check(who, B, T, D, ldmin, ldmax, workspace, workspace_bytes, &s)) return rc;
    KTF_REQUIRE(!norm_overlap(z, s.rows * ldz, dz, s.rows * ld_dz) && !norm_overlap(gy, s.rows * ldg, dz, s.rows * ld_dz),
                "%s: dz overlaps z or gy", who);
    hipStream_t st = (hipStream_t)stream;
    NormParams p = {};
    p.z = z; p.gy = gy; p.out = dz; p.ldz = ldz; p.ldg = ldg; p.ldo = ld_dz;
    p.rows = (int)s.rows; p.T = (int)T; p.D = D; p.nslots = (int)s.nslots;
    p.lens = lens; p.relu = relu != 0; p.training = training != 0; p.gamma = gamma; p.saved = saved;
    p.slots = reinterpret_cast<double*>(workspace);
    p.tot = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + s.slot_bytes);
    const bool vec = norm_vec({gy, z, dz}, {ldg, ldz, ld_dz});
    if (p.training || dgamma) {                       // evaluation without dgamma needs no sum
        if (s.nslots > 0) {
            p.nchunks = ktf_cdiv(D, NORM_COLS);
            const dim3 grid((unsigned)(s.nslots * p.nchunks));
            if (vec) hipLaunchKernelGGL((norm_stats_kernel<true, true>), grid, dim3(NORM_STAT_WAVES * 64), 0, st, p);
            else hipLaunchKernelGGL((norm_stats_kernel<false, true>), grid, dim3(NORM_STAT_WAVES * 64), 0, st, p);
            KTF_CHECK_LAUNCH(who);
        }
        hipLaunchKernelGGL(norm_bwd_finalize_kernel, dim3((unsigned)ktf_cdiv(D, NORM_FIN_COLS)), dim3(NORM_FIN_THREADS), 0, st, p.slots,
                           p.nslots, D, lens, (int)B, (int)T, p.tot, dgamma);
        KTF_CHECK_LAUNCH(who);
    }
    if (s.rows > 0) {
        p.nchunks = ktf_cdiv(ld_dz, NORM_COLS);
        const dim3 grid((unsigned)(ktf_cdiv(s.rows, NORM_APPLY_ROWS) * (int64_t)p.nchunks));
        if (vec) hipLaunchKernelGGL((norm_apply_kernel<true, true>), grid, dim3(NORM_APPLY_WAVES * 64), 0, st, p);
        else hipLaunchKernelGGL((norm_apply_kernel<false, true>), grid, dim3(NORM_APPLY_WAVES * 64), 0, st, p);
        KTF_CHECK_LAUNCH(who);
    }
    return KTF_OK;
}
