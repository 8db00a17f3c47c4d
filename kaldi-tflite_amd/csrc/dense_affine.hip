// The dense affine of the classification head and its gradients (include/ktf_dense.h states the contract as numbered rules,
// INTEGRATION.md section 2o the use, DESIGN.md section 7 the design and the measurements): M = 1 .. ~1000 rows against a weight of
// N = 10^3 .. 6 10^4 rows, D = 64 .. 512, on operands as they stand in memory -- no padded copy, no 16-bit copy.
//
//   ktf_dense_forward        dense_gemm_kernel<mode, false, false>   z  = x w^T + bias     grid (M-tiles, N-tiles)
//   ktf_dense_grad_data      dense_gemm_kernel<mode, false, true>    dx = g w             grid (D-tiles, M-tiles, slots)
//                            dense_slot_sum_kernel                   the slots added in ascending order (more than one slot)
//   ktf_dense_grad_weights   dense_gemm_kernel<mode, true, true>     dw = g^T x, dbias    grid (D-tiles, N-tiles)
//
// One kernel: C[i,j] = sum_k A(i,k) B(j,k). An operand is K-contiguous in memory (A(i,k) = a[i * lda + k]) or, with TA / TB, K-strided
// (A(i,k) = a[k * lda + i]) and then transposed on its way into LDS. A workgroup of WM x WN waves owns a (32 WM) x (32 WN) tile of C,
// one 32 x 32 accumulator block per wave; the reduction runs in steps of DN_BK = 32 through two LDS stages that are refilled from
// registers (the loads of step s + 1 fly under the matrix instructions of step s, one barrier per step).
//
// LDS holds fp32 in every mode: an image is [tile row][32 k] with rows of DN_PITCH = 36 floats (144 bytes: the sixteen lanes of a
// ds_read_b128 group fall on sixteen disjoint sets of four banks). Lane (r = lane & 31, h = lane >> 5) reads the eight consecutive
// floats 8 h .. 8 h + 7 of each half step of 16 as two 16-byte fragments. BF16 / BF16X3 round (and split) them in registers into the
// lane's fragment of v_mfma_f32_32x32x16_bf16, whose lane (r, h) supplies k = 8 h .. 8 h + 7. F32 issues eight v_mfma_f32_32x32x2_f32,
// whose lane (r, h) supplies k = h: for the chain to run in ascending k the image is written with k permuted inside every 16
// (dn_kpos: the even k first, then the odd ones), so that float 8 h + i of a lane is k = 2 i + h.
//
// Staging. A K-contiguous operand puts its lanes on consecutive k (a wave's load is two rows of 128 contiguous bytes) and stores
// single floats. A K-strided operand puts its lanes on consecutive tile rows (256 or 128 contiguous bytes per load), a thread holds 8
// or 16 consecutive k of ONE tile row and stores them as 16-byte pieces: the transposition costs no LDS pass. Every load is 4 bytes
// per lane whatever the alignment (rule 5), and elements outside the operand are 0.0f and never loaded (rule 6).
#include <type_traits>

#include "tdnn_common.h"
#include "../../include/ktf_dense.h"

#define DN_BK 32
#define DN_PITCH 36

struct DenseParams {
    const float* a;         // rows x K (K-contiguous) or K x rows (K-strided)
    const float* b;         // cols x K or K x cols
    const float* bias;      // cols floats or NULL: the start of every column's chain
    float* c;               // (rows, ldc): columns [cols, ldc) are written as zero
    float* dbias;           // rows floats or NULL: fp64 sums over k of the staged A image (rule 3)
    int64_t lda, ldb, ldc;
    int64_t slot_stride;    // floats between the C tiles of consecutive slots (blockIdx.z)
    int32_t rows, cols, K;
    int32_t slot_k;         // reduction elements per slot
    int32_t i_on_x;         // the tile's row index is blockIdx.x (forward: M-tiles fastest), otherwise blockIdx.y
};

// position inside a tile row's 32 floats of reduction element k of the step
template <int MODE>
__device__ __forceinline__ int dn_kpos(int k) {
    return MODE == KTF_GEMM_F32 ? (k & 16) + ((k & 1) << 3) + ((k & 15) >> 1) : k;
}

// eight consecutive k from k0 (a multiple of 8) of one tile row, as two 16-byte stores
template <int MODE>
__device__ __forceinline__ void dn_store8(float* row, int k0, const float* v) {
    if (MODE == KTF_GEMM_F32) {
        float* at = row + (k0 & 16) + ((k0 & 8) >> 1);
        *reinterpret_cast<fv4*>(at) = fv4{v[0], v[2], v[4], v[6]};
        *reinterpret_cast<fv4*>(at + 8) = fv4{v[1], v[3], v[5], v[7]};
    } else {
        *reinterpret_cast<fv4*>(row + k0) = fv4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<fv4*>(row + k0 + 4) = fv4{v[4], v[5], v[6], v[7]};
    }
}

// R tile rows x DN_BK of an operand whose k is contiguous in memory, in the registers of NT threads
template <int MODE, int R, int NT>
struct DnRows {
    static constexpr int E = R * DN_BK / NT;
    float v[E];
    __device__ __forceinline__ void load(const float* ptr, int64_t ld, int64_t row0, int64_t rows, int64_t k0, int64_t kend, int tid) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int q = e * NT + tid;
            const int64_t row = row0 + (q >> 5), k = k0 + (q & 31);
            v[e] = (row < rows && k < kend) ? ptr[row * ld + k] : 0.0f;
        }
    }
    __device__ __forceinline__ void store(float* s, int tid) const {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int q = e * NT + tid;
            s[(q >> 5) * DN_PITCH + dn_kpos<MODE>(q & 31)] = v[e];
        }
    }
};

// ... of an operand whose k is the row axis in memory: thread -> tile row tid % R and the KPT consecutive k from (tid / R) * KPT
template <int MODE, int R, int NT>
struct DnCols {
    static constexpr int KPT = R * DN_BK / NT;
    static_assert(NT % R == 0 && KPT % 8 == 0, "a thread holds whole groups of eight k of one tile row");
    float v[KPT];
    __device__ __forceinline__ void load(const float* ptr, int64_t ld, int64_t row0, int64_t rows, int64_t k0, int64_t kend, int tid) {
        const int64_t row = row0 + tid % R, kk = k0 + (tid / R) * KPT;
#pragma unroll
        for (int e = 0; e < KPT; ++e) v[e] = (row < rows && kk + e < kend) ? ptr[(kk + e) * ld + row] : 0.0f;
    }
    __device__ __forceinline__ void store(float* s, int tid) const {
        float* row = s + (tid % R) * DN_PITCH;
#pragma unroll
        for (int q = 0; q < KPT; q += 8) dn_store8<MODE>(row, (tid / R) * KPT + q, v + q);
    }
};

// eight fp32 -> the lane's bf16 fragment: hi = bf16(v), round to nearest even; X3: lo = bf16(v - hi)
template <bool X3>
__device__ __forceinline__ void dn_split8(const float (&v)[8], bfrag8& hi, bfrag8& lo) {
    u32x4 h, l = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned short h0 = f2bf(v[2 * i]), h1 = f2bf(v[2 * i + 1]);
        h[i] = (unsigned)h0 | ((unsigned)h1 << 16);
        if (X3) l[i] = (unsigned)f2bf(v[2 * i] - bf2f(h0)) | ((unsigned)f2bf(v[2 * i + 1] - bf2f(h1)) << 16);
    }
    hi = __builtin_bit_cast(bfrag8, h);
    lo = __builtin_bit_cast(bfrag8, l);
}

// one half step (16 k) of a 32 x 32 block from the lane's eight floats of either operand
template <int MODE>
__device__ __forceinline__ void dn_mma(f32x16& acc, const float (&a)[8], const float (&b)[8]) {
    if constexpr (MODE == KTF_GEMM_F32) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[i], acc, 0, 0, 0);
    } else {
        constexpr bool X3 = MODE == KTF_GEMM_BF16X3;
        bfrag8 ah, al, bh, bl;
        dn_split8<X3>(a, ah, al);
        dn_split8<X3>(b, bh, bl);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
        if (X3) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
        }
    }
}

template <int MODE, bool TA, bool TB, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void dense_gemm_kernel(DenseParams p) {
    constexpr int NT = 64 * WM * WN, BM = 32 * WM, BN = 32 * WN;
    using StageA = std::conditional_t<TA, DnCols<MODE, BM, NT>, DnRows<MODE, BM, NT>>;
    using StageB = std::conditional_t<TB, DnCols<MODE, BN, NT>, DnRows<MODE, BN, NT>>;
    __shared__ __attribute__((aligned(16))) float As[2][BM * DN_PITCH];
    __shared__ __attribute__((aligned(16))) float Bs[2][BN * DN_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int64_t i0 = (int64_t)(p.i_on_x ? blockIdx.x : blockIdx.y) * BM;
    const int64_t j0 = (int64_t)(p.i_on_x ? blockIdx.y : blockIdx.x) * BN;
    const int64_t kbeg = (int64_t)blockIdx.z * p.slot_k;
    const int64_t kend = kbeg + p.slot_k < p.K ? kbeg + p.slot_k : p.K;
    float* c = p.c + (int64_t)blockIdx.z * p.slot_stride;
    const int nk = j0 < p.cols ? (int)((kend - kbeg + DN_BK - 1) / DN_BK) : 0;      // a tile of pad columns writes zeros only

    // accumulator layout: column = lane & 31, row = acc32_row(0, reg, lane)
    const int64_t j = j0 + wn * 32 + (lane & 31);
    const float start = (p.bias && j < p.cols) ? p.bias[j] : 0.0f;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = start;

    const bool with_dbias = p.dbias && j0 == 0;
    double bsum = 0.0;
    StageA sa;
    StageB sb;
    if (nk > 0) {
        sa.load(p.a, p.lda, i0, p.rows, kbeg, kend, tid);
        sb.load(p.b, p.ldb, j0, p.cols, kbeg, kend, tid);
        sa.store(As[0], tid);
        sb.store(Bs[0], tid);
    }
    __syncthreads();
    for (int ks = 0; ks < nk; ++ks) {
        const int buf = ks & 1;
        if (ks + 1 < nk) {
            sa.load(p.a, p.lda, i0, p.rows, kbeg + (int64_t)(ks + 1) * DN_BK, kend, tid);
            sb.load(p.b, p.ldb, j0, p.cols, kbeg + (int64_t)(ks + 1) * DN_BK, kend, tid);
        }
        const float* ar = As[buf] + (wm * 32 + (lane & 31)) * DN_PITCH + 8 * (lane >> 5);
        const float* br = Bs[buf] + (wn * 32 + (lane & 31)) * DN_PITCH + 8 * (lane >> 5);
#pragma unroll
        for (int kk = 0; kk < DN_BK; kk += 16) {
            const fv4 a0 = *reinterpret_cast<const fv4*>(ar + kk), a1 = *reinterpret_cast<const fv4*>(ar + kk + 4);
            const fv4 b0 = *reinterpret_cast<const fv4*>(br + kk), b1 = *reinterpret_cast<const fv4*>(br + kk + 4);
            const float fa[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
            const float fb[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
            dn_mma<MODE>(acc, fa, fb);
        }
        if (with_dbias && tid < BM) {                // the unrounded fp32 of tile row tid, k ascending (elements past K are +0)
            const float* g = As[buf] + tid * DN_PITCH;
#pragma unroll
            for (int k = 0; k < DN_BK; ++k) bsum += (double)g[dn_kpos<MODE>(k)];
        }
        if (ks + 1 < nk) {
            sa.store(As[buf ^ 1], tid);
            sb.store(Bs[buf ^ 1], tid);
        }
        __syncthreads();
    }

    if (j < p.ldc) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int64_t i = i0 + wm * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);      // acc32_row
            if (i < p.rows) c[i * p.ldc + j] = j < p.cols ? acc[reg] : 0.0f;
        }
    }
    if (with_dbias && tid < BM && i0 + tid < p.rows) p.dbias[i0 + tid] = (float)bsum;
}

// dx[m, d] = the slots' partial tiles (M, D) added in ascending slot order; columns [D, lddx) zero
__global__ __launch_bounds__(256) void dense_slot_sum_kernel(const float* __restrict__ ws, int nslots, int64_t slot_stride, int64_t M, int64_t D,
                                                             float* __restrict__ dx, int64_t lddx) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= M * lddx) return;
    const int64_t m = idx / lddx, d = idx - m * lddx;
    float v = 0.0f;
    if (d < D) {
        const float* s = ws + m * D + d;
        v = s[0];
        for (int i = 1; i < nslots; ++i) v += s[(int64_t)i * slot_stride];
    }
    dx[idx] = v;
}

// ------------------------------------------------------------------------------------ host
static const int64_t DN_LIMIT = 1ll << 31;

// The tile: 64 x 64 outputs per workgroup where that still gives 512 workgroups, 32 x 32 otherwise -- a rule on the sizes alone, and
// one that no bit depends on (every element's chain is the same in both).
template <int MODE, bool TA, bool TB>
static void dn_launch_mode(const DenseParams& p, int64_t slots, hipStream_t st) {
    const bool big = (int64_t)ktf_cdiv(p.rows, 64) * ktf_cdiv(p.cols, 64) * slots >= 512;       // (pad columns do not count)
    const int t = big ? 64 : 32;
    const unsigned gi = (unsigned)ktf_cdiv(p.rows, t), gj = (unsigned)ktf_cdiv(p.ldc, t);
    const dim3 grid = p.i_on_x ? dim3(gi, gj, (unsigned)slots) : dim3(gj, gi, (unsigned)slots);
    if (big)
        hipLaunchKernelGGL((dense_gemm_kernel<MODE, TA, TB, 2, 2>), grid, dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL((dense_gemm_kernel<MODE, TA, TB, 1, 1>), grid, dim3(64), 0, st, p);
}

template <bool TA, bool TB>
static void dn_launch(int32_t gemm, const DenseParams& p, int64_t slots, hipStream_t st) {
    if (gemm == KTF_GEMM_F32) dn_launch_mode<KTF_GEMM_F32, TA, TB>(p, slots, st);
    else if (gemm == KTF_GEMM_BF16) dn_launch_mode<KTF_GEMM_BF16, TA, TB>(p, slots, st);
    else dn_launch_mode<KTF_GEMM_BF16X3, TA, TB>(p, slots, st);
}

// `na` floats at a against `nb` floats at b
static bool dn_overlap(const float* a, int64_t na, const float* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && na > 0 && nb > 0 && a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}
// floats from the first to the last element read of a (rows, ld) operand with `cols` columns
static int64_t dn_span(int64_t rows, int64_t ld, int64_t cols) { return rows > 0 ? (rows - 1) * ld + cols : 0; }

static int dn_check_sizes(const char* who, int64_t M, int64_t N, int64_t D, int32_t gemm) {
    KTF_REQUIRE(M >= 0 && N >= 1 && D >= 1, "%s: M >= 0, N >= 1 and D >= 1 are required (M %lld, N %lld, D %lld)", who, (long long)M, (long long)N,
                (long long)D);
    KTF_REQUIRE(M < DN_LIMIT && N < DN_LIMIT && D < DN_LIMIT, "%s: M, N or D reaches 2^31", who);
    KTF_REQUIRE(gemm == KTF_GEMM_F32 || gemm == KTF_GEMM_BF16 || gemm == KTF_GEMM_BF16X3, "%s: gemm %d is not KTF_GEMM_F32, _BF16 or _BF16X3", who,
                (int)gemm);
    return KTF_OK;
}

static int dn_check_ld(const char* who, const char* name, int64_t ld, int64_t need) {
    KTF_REQUIRE(ld >= need, "%s: %s %lld below the row length %lld", who, name, (long long)ld, (long long)need);
    KTF_REQUIRE(ld < DN_LIMIT, "%s: %s reaches 2^31", who, name);
    return KTF_OK;
}

extern "C" int32_t ktf_dense_slot_cols(void) { return KTF_DENSE_SLOT_COLS; }

extern "C" int64_t ktf_dense_workspace_bytes(int64_t M, int64_t N, int64_t D) {
    const char* who = "ktf_dense_workspace_bytes";
    if (int rc = dn_check_sizes(who, M, N, D, KTF_GEMM_F32)) return rc;
    const int64_t slots = (N + KTF_DENSE_SLOT_COLS - 1) / KTF_DENSE_SLOT_COLS;
    int64_t bytes = 0;
    KTF_REQUIRE(!__builtin_mul_overflow(slots * 4, (M > 0 ? M : 1) * D, &bytes) && bytes < (1ll << 62), "%s: the workspace does not fit 63 bits", who);
    return al256(bytes);
}

extern "C" int ktf_dense_forward(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, int64_t M, int64_t N, int64_t D,
                                 int32_t gemm, float* z, int64_t ldz, void* stream) {
    const char* who = "ktf_dense_forward";
    KTF_REQUIRE(x && w && z, "%s: null argument", who);
    if (int rc = dn_check_sizes(who, M, N, D, gemm)) return rc;
    if (int rc = dn_check_ld(who, "ldx", ldx, D)) return rc;
    if (int rc = dn_check_ld(who, "ldw", ldw, D)) return rc;
    if (int rc = dn_check_ld(who, "ldz", ldz, N)) return rc;
    KTF_REQUIRE(ldz <= KTF_DENSE_MAX_COLS, "%s: ldz %lld above %d", who, (long long)ldz, KTF_DENSE_MAX_COLS);
    KTF_REQUIRE(!dn_overlap(z, M * ldz, x, dn_span(M, ldx, D)) && !dn_overlap(z, M * ldz, w, dn_span(N, ldw, D)) && !dn_overlap(z, M * ldz, bias, N),
                "%s: z overlaps x, w or bias", who);
    if (M == 0) return KTF_OK;
    DenseParams p = {x, w, bias, z, nullptr, ldx, ldw, ldz, 0, (int32_t)M, (int32_t)N, (int32_t)D, (int32_t)D, 1};
    dn_launch<false, false>(gemm, p, 1, (hipStream_t)stream);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_dense_grad_data(const float* g, int64_t ldg, const float* w, int64_t ldw, int64_t M, int64_t N, int64_t D, int32_t gemm,
                                   float* dx, int64_t lddx, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_dense_grad_data";
    KTF_REQUIRE(g && w && dx && workspace, "%s: null argument", who);
    if (int rc = dn_check_sizes(who, M, N, D, gemm)) return rc;
    if (int rc = dn_check_ld(who, "ldg", ldg, N)) return rc;
    if (int rc = dn_check_ld(who, "ldw", ldw, D)) return rc;
    if (int rc = dn_check_ld(who, "lddx", lddx, D)) return rc;
    KTF_REQUIRE(M <= KTF_DENSE_MAX_COLS, "%s: M %lld above %d", who, (long long)M, KTF_DENSE_MAX_COLS);
    KTF_REQUIRE(M * lddx < (1ll << 38), "%s: M * lddx reaches 2^38", who);
    const int64_t slots = (N + KTF_DENSE_SLOT_COLS - 1) / KTF_DENSE_SLOT_COLS;
    KTF_REQUIRE(slots <= 65535, "%s: N %lld above 65535 slots of %d columns", who, (long long)N, KTF_DENSE_SLOT_COLS);
    const int64_t need = ktf_dense_workspace_bytes(M, N, D);
    if (need < 0) return (int)need;
    if (int rc = ktf_check_workspace(who, workspace, workspace_bytes, need)) return rc;
    float* ws = reinterpret_cast<float*>(workspace);
    KTF_REQUIRE(!dn_overlap(dx, M * lddx, g, dn_span(M, ldg, N)) && !dn_overlap(dx, M * lddx, w, dn_span(N, ldw, D)) &&
                    !dn_overlap(dx, M * lddx, ws, need / 4) && !dn_overlap(ws, need / 4, g, dn_span(M, ldg, N)) &&
                    !dn_overlap(ws, need / 4, w, dn_span(N, ldw, D)),
                "%s: dx or the workspace overlaps g, w or each other", who);
    if (M == 0) return KTF_OK;
    hipStream_t st = (hipStream_t)stream;
    DenseParams p = {g, w, nullptr, dx, nullptr, ldg, ldw, lddx, 0, (int32_t)M, (int32_t)D, (int32_t)N, KTF_DENSE_SLOT_COLS, 0};
    if (slots > 1) {                                 // dense partial tiles (M, D), one per slot
        p.c = ws;
        p.ldc = D;
        p.slot_stride = M * D;
    }
    dn_launch<false, true>(gemm, p, slots, st);
    if (slots > 1)
        hipLaunchKernelGGL(dense_slot_sum_kernel, dim3((unsigned)ktf_cdiv(M * lddx, 256)), dim3(256), 0, st, ws, (int)slots, M * D, M, D, dx, lddx);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_dense_grad_weights(const float* g, int64_t ldg, const float* x, int64_t ldx, int64_t M, int64_t N, int64_t D, int32_t gemm,
                                      float* dw, int64_t lddw, float* dbias, void* stream) {
    const char* who = "ktf_dense_grad_weights";
    KTF_REQUIRE(g && x && dw, "%s: null argument", who);
    if (int rc = dn_check_sizes(who, M, N, D, gemm)) return rc;
    if (int rc = dn_check_ld(who, "ldg", ldg, N)) return rc;
    if (int rc = dn_check_ld(who, "ldx", ldx, D)) return rc;
    if (int rc = dn_check_ld(who, "lddw", lddw, D)) return rc;
    KTF_REQUIRE(N <= KTF_DENSE_MAX_COLS, "%s: N %lld above %d", who, (long long)N, KTF_DENSE_MAX_COLS);
    const int64_t ng = dn_span(M, ldg, N), nx = dn_span(M, ldx, D);
    KTF_REQUIRE(!dn_overlap(dw, N * lddw, g, ng) && !dn_overlap(dw, N * lddw, x, nx) && !dn_overlap(dbias, N, g, ng) && !dn_overlap(dbias, N, x, nx) &&
                    !dn_overlap(dw, N * lddw, dbias, N),
                "%s: dw or dbias overlaps g, x or each other", who);
    DenseParams p = {g, x, nullptr, dw, dbias, ldg, ldx, lddw, 0, (int32_t)N, (int32_t)D, (int32_t)M, (int32_t)M, 0};
    dn_launch<true, true>(gemm, p, 1, (hipStream_t)stream);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
