// Shared by the TDNN GEMM kernel families (tdnn_f32.hip, tdnn_pair.hip, tdnn_grad.hip, tdnn_bf16.hip, tdnn_split.hip) and their dispatcher
// (tdnn_gemm.hip): the kernel parameter block, the output-length rule, the tile headers, activations, the epilogue value and typed stores
// of the fp32 / pair families, the register-staged 32x32x2 main loop, and the per-family launchers.
//
//   y[b,t,u] = post(act(bias[u] + sum_k sum_d x[b, row(t,k), d] * W[u, k*Dp + d]))
//   row(t,k) = clip(start + t*sub + ctx[k], 0, len_b - 1)
//
// The (T, K*D) im2col matrix of the reference (tf.gather, tdnn.py:258) is never built: the A-tile rows of one K-step all come
// from ONE context offset (Dp is a multiple of the K-step), so staging a tile is a row gather of contiguous 64/128-byte pieces
// straight from the activation matrix, clamped per utterance. M-tiles never straddle utterances (activations are
// utterance-strided), so edge replication needs no row->utterance map.
// Replaces: layers/tdnn/tdnn.py:251-280 (+ keras ReLU, batchnorm.py:78-88) of the reference.
#pragma once
#include <stdlib.h>
#include <type_traits>

#include "common.h"
#include "pooled_stats.h"

// Fixed choices of the split-plane kernel (each was an A/B in round 2; DESIGN.md section 5 has the numbers)
#define KTF_X3_Y_NT 1         // the 16-bit activation planes are written with non-temporal stores (the XCD's L2 keeps weights / shared tiles)
#define KTF_X3_WFIRST 1       // the W half of stage 0 is issued before the utterance length is loaded

typedef __attribute__((address_space(3))) void lds_ptr_t;
typedef __attribute__((address_space(1))) const void glb_ptr_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bfrag8;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(4))) float fv4;
typedef __attribute__((ext_vector_type(2))) unsigned uv2;

struct TdnnParams {
    const void* x;
    const int32_t* lens;
    const void* w;
    const void* w_lo;
    const float* bias;
    const float* scale;
    const float* shift;
    void* y;
    const void* x_lo;       // split-bf16 planes (KTF_GEMM_BF16X3 with bf16 x): x = hi plane, x_lo = lo plane
    void* y_lo;             // ... and the same for the output (y = hi plane) when non-null
    int32_t* out_lens;
    int64_t T, ldx, ldy, Tout;
    int32_t units, din_pad, nctx, sub, valid, act, y_dtype, ktot;
    int32_t ctx[16];
    int32_t wtiled;         // KTF_TDNN_W_TILED: W stored as the kernel's LDS images, one contiguous 16 KiB block per (N-tile, K-step)
    int32_t kinter;         // KTF_TDNN_K_INTERLEAVED: K runs (32-wide feature chunk, context, feature) instead of (context, feature)
    int32_t stat_slots;     // fused pooling: 0 = fp64 atomics into (B, 2, units); > 0 = the kernel's PoolSlots::slots (KTF_TDNN_DET_STATS)
    int32_t y_pair;         // fp32-sized output slots hold the KTF_BF16P pair of the value (y_dtype is KTF_F32 to the store paths)
    const int32_t* row_starts;  // ktf_tdnn_split_flat: (B + 1) exclusive prefix sums of lens (flat row tiling of tdnn_x3s_kernel), else NULL
    const int32_t* row_map;     // ... and optionally ktf_flat_row_map's table: (output row or -1, frame, utterance length, utterance) per flat row
};

// KTF_BF16P: bf16(v) in the low half, bf16(v - bf16(v)) in the high half of a 32-bit slot (tdnn_pair.hip), returned as the float
// with that bit pattern so that the fp32 store paths carry it
__device__ __forceinline__ float ktf_pair(float v) {
    const unsigned hi = f2bf(v);
    const unsigned lo = f2bf(v - bf2f((unsigned short)hi));
    return __uint_as_float(hi | (lo << 16));
}

__device__ __forceinline__ int tdnn_out_len(int len, const TdnnParams& p, int& start) {
    start = 0;
    int end = len;
    if (p.valid) {
        if (p.ctx[0] < 0) start = -p.ctx[0];
        if (p.ctx[p.nctx - 1] > 0) end = len - p.ctx[p.nctx - 1];
    }
    const int n = end - start;
    return n <= 0 ? 0 : (n + p.sub - 1) / p.sub;
}

// The tile header of the kernels on the grouped 1-D walk (grouped_blocks below): block ID -> (xcd = ID % 8, slot = ID / 8); an XCD
// walks its own M-tiles and runs all N-tiles of one M-tile back to back, so the gathered activation rows are fetched into that XCD's
// L2 once. Declares the BM x BN tile's b (utterance), len, start (first input row: VALID padding), out_len, t0 / n0 (first output
// row / unit) and nt (N-tile) from the kernel's p, mtiles, ntiles, gtiles; the utterance's first tile writes out_lens[b]; returns
// from the kernel where no tile stands behind the block or the tile holds no valid row.
// (A macro: as an inlined function filling a struct it changed the register allocation and the code of every ring kernel.)
#define TDNN_TILE_HEADER(BM, BN, ID)                                                                   \
    const int tile_id_ = (ID), tile_xcd_ = tile_id_ & 7, tile_slot_ = tile_id_ >> 3;                   \
    const int tile_g_ = (tile_slot_ / ntiles) * 8 + tile_xcd_;     /* global M-tile index */           \
    const int nt = tile_slot_ - (tile_slot_ / ntiles) * ntiles;                                        \
    if (tile_g_ >= gtiles) return;                                                                     \
    const int b = tile_g_ / mtiles, tile_mt_ = tile_g_ - b * mtiles;                                   \
    const int len = p.lens ? p.lens[b] : (int)p.T;                                                     \
    int start;                                                                                         \
    const int out_len = tdnn_out_len(len, p, start);                                                   \
    if (p.out_lens && nt == 0 && tile_mt_ == 0 && threadIdx.x == 0) p.out_lens[b] = out_len;           \
    const int t0 = tile_mt_ * (BM);                                                                    \
    if (t0 >= out_len || len <= 0) return;                                                             \
    const int n0 = nt * (BN);

// The tile header of the kernels on a 3-D grid (x = N-tile, y = M-tile, z = utterance): tdnn_f32_kernel, tdnn_f32s_kernel,
// tdnn_f32t_kernel, tdnn_x4s_kernel, tdnn_bf16_kernel and, with BM = 1 (t0 is its output row), tdnn_f32_rowvec_kernel. Declares b, len,
// start, out_len, t0, n0 as TDNN_TILE_HEADER does, and tid / lane; the utterance's first tile writes out_lens[b]; returns from the kernel
// where the tile holds no valid row. (`wave` stays with the kernels: the DMA-staged ones take it through readfirstlane.)
// (A macro for the reason given at TDNN_TILE_HEADER; the early return has to be the kernel's own.)
#define TDNN_TILE3D_HEADER(BM, BN)                                                                     \
    const int b = blockIdx.z;                                                                          \
    const int len = p.lens ? p.lens[b] : (int)p.T;                                                     \
    int start;                                                                                         \
    const int out_len = tdnn_out_len(len, p, start);                                                   \
    if (p.out_lens && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.out_lens[b] = out_len; \
    const int t0 = blockIdx.y * (BM);                                                                  \
    if (t0 >= out_len || len <= 0) return;                                                             \
    const int n0 = blockIdx.x * (BN);                                                                  \
    const int tid = threadIdx.x, lane = tid & 63;

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == KTF_ACT_RELU) return v < 0.0f ? 0.0f : v;      // tf.nn.relu propagates NaN (Eigen cwiseMax<PropagateNaN>): the pooled row of an
                                                              // utterance without a frame stays NaN through the layers behind the pooling; fmaxf would return 0
    if (act == KTF_ACT_SIGMOID) return 1.0f / (1.0f + expf(-v));
    if (act == KTF_ACT_TANH) return tanhf(v);
    return v;
}

// The rest of tf.keras.activations (TF 2.8: the names layers/tdnn/tdnn.py:117-118 resolves), elementwise ones; the GEMM epilogues
// fuse KTF_ACT_NONE .. KTF_ACT_TANH only, these run as a pass over the layer's output rows (act_rows_kernel, tdnn_gemm.hip).
__device__ __forceinline__ float apply_act_ext(float v, int act) {
    switch (act) {
        case KTF_ACT_ELU: return v > 0.0f ? v : expm1f(v);
        case KTF_ACT_SELU: return 1.05070098735548049342f * (v > 0.0f ? v : 1.67326324235437728481f * expm1f(v));
        case KTF_ACT_SOFTPLUS: return fmaxf(v, 0.0f) + log1pf(expf(-fabsf(v)));
        case KTF_ACT_SOFTSIGN: return v / (fabsf(v) + 1.0f);
        case KTF_ACT_SWISH: return v / (1.0f + expf(-v));
        case KTF_ACT_GELU: return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
        case KTF_ACT_EXPONENTIAL: return expf(v);
        case KTF_ACT_HARD_SIGMOID: return fminf(fmaxf(0.2f * v + 0.5f, 0.0f), 1.0f);
        default: return apply_act(v, act);
    }
}

// The epilogue value of the fp32 and pair families: bias -> activation -> BatchNorm affine (not applied at all without one). A sibling
// of tdnn_ring.h's EPI_VALUE, which differs in both: its ReLU is fmaxf (NaN -> 0) and it always multiplies. TDNN_EPI_ROW: ... as it is
// stored in a row, i.e. as its KTF_BF16P pair where the launch asks for pairs (the pooled form of tdnn_x4s_kernel sums the value itself).
// TDNN_STORE_Y / TDNN_STORE_Y4: the store by the rows' type, of element OFF of y / of the four consecutive units N .. N + 3 whose first
// is element OFF (one 16-byte store for fp32 rows where VEC_OK -- TDNN_Y_VEC_OK -- and all four are units). All read the kernel's `p`.
// (Macros: as inlined functions each of them, the one-line TDNN_Y_VEC_OK included, changed the registers and the instruction count of
// every kernel that uses it -- tdnn_bf16_kernel 108 -> 124 VGPRs; as macros tdnn_bf16_kernel's code is the text it was.)
#define TDNN_EPI_VALUE(ACC, BIAS, SC, SH, ACT)                                                         \
    ({                                                                                                 \
        float v_ = apply_act((ACC) + (BIAS), ACT);                                                     \
        if (p.scale) v_ = v_ * (SC) + (SH);                                                            \
        v_;                                                                                            \
    })
#define TDNN_EPI_ROW(ACC, BIAS, SC, SH, ACT)                                                           \
    ({                                                                                                 \
        float r_ = TDNN_EPI_VALUE(ACC, BIAS, SC, SH, ACT);                                             \
        if (p.y_pair) r_ = ktf_pair(r_);                                                               \
        r_;                                                                                            \
    })
#define TDNN_STORE_Y(OFF, V)                                                                           \
    {                                                                                                  \
        if (p.y_dtype == KTF_F32) reinterpret_cast<float*>(p.y)[OFF] = (V);                            \
        else reinterpret_cast<unsigned short*>(p.y)[OFF] = f2bf(V);                                    \
    }
#define TDNN_STORE_Y4(OFF, N, V, VEC_OK)                                                               \
    {                                                                                                  \
        if (p.y_dtype == KTF_F32) {                                                                    \
            float* yp_ = reinterpret_cast<float*>(p.y) + (OFF);                                        \
            if ((VEC_OK) && (N) + 4 <= p.units) {                                                      \
                *reinterpret_cast<fv4*>(yp_) = fv4{V[0], V[1], V[2], V[3]};                            \
            } else {                                                                                   \
                _Pragma("unroll") for (int e = 0; e < 4; ++e)                                          \
                    if ((N) + e < p.units) yp_[e] = V[e];                                              \
            }                                                                                          \
        } else {                                                                                       \
            unsigned short* yp_ = reinterpret_cast<unsigned short*>(p.y) + (OFF);                      \
            _Pragma("unroll") for (int e = 0; e < 4; ++e)                                              \
                if ((N) + e < p.units) yp_[e] = f2bf(V[e]);                                            \
        }                                                                                              \
    }
#define TDNN_Y_VEC_OK ((p.ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(p.y) & 15) == 0)

// Row of register `reg` in the 32x32 accumulator layout of the block whose first row is `base` (column = lane & 31)
// (base is an argument because the sum's association is part of the generated code: base + acc32_row(...) moved every caller's registers)
__device__ __forceinline__ int acc32_row(int base, int reg, int lane) { return base + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// Epilogue for the 32x32 accumulator layout: col = lane&31, row = acc32_row(0, reg, lane).
__device__ __forceinline__ void store_tile32(const f32x16& acc, const TdnnParams& p, int64_t out_row0, int rows_valid,
                                             int m_base, int n_base, int lane) {
    const int n = n_base + (lane & 31);
    if (n >= p.units) return;
    const float bias = p.bias ? p.bias[n] : 0.0f;
    const float sc = p.scale ? p.scale[n] : 1.0f;
    const float sh = p.shift ? p.shift[n] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = acc32_row(m_base, r, lane);
        if (m < rows_valid) {
            const float v = TDNN_EPI_ROW(acc[r], bias, sc, sh, p.act);
            const int64_t off = (out_row0 + m) * p.ldy + n;
            TDNN_STORE_Y(off, v)
        }
    }
}

// Same tile with the MFMA operands swapped (W block as A, x block as B): the accumulator is the transposed tile,
//   time row = lane&31, unit = acc32_row(0, reg, lane),
// so a lane owns four CONSECUTIVE units per register quad and the store is 16 bytes instead of four 4-byte stores (the
// 64 scalar stores per lane of store_tile32 cost the fp32 tile kernel ~20 % of its time). Products commute and the K
// order is unchanged: bit-identical values.
template <int ACT>
__device__ __forceinline__ void store_tile32_t(const f32x16& acc, const TdnnParams& p, int64_t out_row0, int rows_valid,
                                               int m_base, int n_base, int lane) {
    const int m = m_base + (lane & 31);
    if (m >= rows_valid) return;
    const int64_t rowoff = (out_row0 + m) * p.ldy;
    const bool vec_ok = TDNN_Y_VEC_OK;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int n = n_base + 8 * q + 4 * (lane >> 5);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool nv = n + e < p.units;
            v[e] = TDNN_EPI_ROW(acc[q * 4 + e], (nv && p.bias) ? p.bias[n + e] : 0.0f, nv ? p.scale[n + e] : 1.0f, nv ? p.shift[n + e] : 0.0f, ACT);
        }
        TDNN_STORE_Y4(rowoff + n, n, v, vec_ok)
    }
}

// The register-staged, double-buffered main loop of the 32x32x2 fp32 tile GEMMs (tdnn_f32_kernel: the KTF_TDNN_REF_TILES bitwise
// reference; grad_dx_kernel, grad_dw_kernel in tdnn_grad.hip): four waves as 2 x 2, wave (wm, wn) owns MTM x MTN blocks of 32 x 32; As /
// Bs are the two stages of (64 MTM) / (64 MTN) rows of BK + 1 floats. load_global(ks) fetches step ks into the caller's registers,
// store_lds(buf) writes them to stage buf (each caller's own gather and transposition), step(buf) runs once per step between the MFMAs
// and the refill of the other stage (grad_dw_kernel's bias sum). SWAP: the b fragment is the MFMA's first operand (the transposed tile
// of store_tile32_t). nk >= 1.
template <int MTM, int MTN, int BK, bool SWAP, typename LoadGlobal, typename StoreLds, typename Step>
__device__ __forceinline__ void tile32_mainloop(f32x16 (&acc)[MTM][MTN], const float* As, const float* Bs, int nk, int wm, int wn, int lane,
                                                LoadGlobal&& load_global, StoreLds&& store_lds, Step&& step) {
    constexpr int PITCH = BK + 1;
#pragma unroll
    for (int i = 0; i < MTM; ++i)
#pragma unroll
        for (int j = 0; j < MTN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    load_global(0);
    store_lds(0);
    __syncthreads();
    for (int ks = 0; ks < nk; ++ks) {
        const int buf = ks & 1;
        if (ks + 1 < nk) load_global(ks + 1);
        const float* a_base = As + buf * (64 * MTM * PITCH) + (wm * 32 * MTM + (lane & 31)) * PITCH + (lane >> 5);
        const float* b_base = Bs + buf * (64 * MTN * PITCH) + (wn * 32 * MTN + (lane & 31)) * PITCH + (lane >> 5);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            float av[MTM], bv[MTN];
#pragma unroll
            for (int i = 0; i < MTM; ++i) av[i] = a_base[i * 32 * PITCH + kk];
#pragma unroll
            for (int j = 0; j < MTN; ++j) bv[j] = b_base[j * 32 * PITCH + kk];
#pragma unroll
            for (int i = 0; i < MTM; ++i)
#pragma unroll
                for (int j = 0; j < MTN; ++j)
                    acc[i][j] = SWAP ? __builtin_amdgcn_mfma_f32_32x32x2f32(bv[j], av[i], acc[i][j], 0, 0, 0)
                                     : __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        step(buf);
        if (ks + 1 < nk) store_lds(buf ^ 1);
        __syncthreads();
    }
}

// name of the kernel family the calling thread's last ktf_tdnn* call launched (ktf_tdnn_last_kernel; dispatch tests)
extern thread_local const char* g_ktf_last_kernel;

// Opts kernel K in to `bytes` of dynamic LDS, once per kernel and device. K is a template argument so that every kernel has a flag
// of its own: most of them share one signature.
template <auto K>
static void tdnn_lds_once(int bytes) {
    KTF_LDS_ONCE(bytes, K);
}

// Every TDNN GEMM launch: records `name` for ktf_tdnn_last_kernel(), opts K in to `lds_attr` bytes of dynamic LDS (0: no opt-in,
// for kernels within the default 64 KiB) and launches it with `lds` bytes (MX: the opt-in covers the largest K, the launch its own).
template <auto K, typename... Args>
static void tdnn_launch_kernel(const char* name, dim3 grid, dim3 block, int lds, int lds_attr, hipStream_t st, Args... args) {
    g_ktf_last_kernel = name;
    if (lds_attr > 0) tdnn_lds_once<K>(lds_attr);
    hipLaunchKernelGGL(K, grid, block, lds, st, args...);
}

// Compile-time dispatch: f(std::integral_constant<T, V>{}) for the first V of the list that equals v, else for the last one (the
// launchers pass values they have validated, so the last entry is the remaining case). Template arguments keep the list's type.
template <auto V, auto... Vs, typename F>
static void tdnn_pick(decltype(V) v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<decltype(V), V>{});
    else if (v == V) f(std::integral_constant<decltype(V), V>{});
    else tdnn_pick<Vs...>(v, f);
}

// Blocks of a grouped tile walk: the M-tiles (gtiles over the batch) in groups of 8, times the N-tiles
static inline int64_t grouped_blocks(int64_t gtiles, int64_t ntiles) { return ((gtiles + 7) / 8) * 8 * ntiles; }

// Column width of the 64-row small tiles with K-step 64 (tdnn_f32s_kernel, tdnn_x4s_kernel): one workgroup per CU (the ring takes most
// of the LDS), so the cost is (rounds of 256 workgroups) x (time of one, ~ width + fixed part); 96 columns only where W's rows, padded to
// a multiple of 128, cover the last tile. `mtiles`: 64-row tiles over the batch.
static inline int small_tile_width(int units, int64_t mtiles) {
    int best = 32;
    int64_t best_cost = INT64_MAX;
    for (int bn = 32; bn <= 96; bn += 32) {
        if (bn == 96 && (int64_t)ktf_cdiv(units, 96) * 96 > (int64_t)ktf_cdiv(units, 128) * 128) continue;
        const int64_t cost = ktf_cdiv(ktf_cdiv(units, bn) * mtiles, 256) * (bn + 16);
        if (cost < best_cost) best_cost = cost, best = bn;
    }
    return best;
}

// The descriptor checks of ktf_tdnn* and ktf_tdnn_mx*; each adds the limits of its own kernels. `who` names the entry point.
static inline int tdnn_check_desc(const KtfTdnnDesc* d, const float* scale, const float* shift, const char* who) {
    KTF_REQUIRE(d->units > 0 && d->din > 0, "%s: units/din must be > 0", who);
    KTF_REQUIRE(d->din_pad >= d->din && d->din_pad % 32 == 0, "%s: din_pad %d must be a multiple of 32 with din <= din_pad", who, d->din_pad);
    KTF_REQUIRE(d->nctx >= 1 && d->nctx <= 16, "%s: nctx %d outside [1,16]", who, d->nctx);
    for (int i = 1; i < d->nctx; ++i) KTF_REQUIRE(d->ctx[i] > d->ctx[i - 1], "%s: context must be strictly ascending", who);
    KTF_REQUIRE(d->subsampling > 0, "%s: subsampling_factor should be > 0", who);
    KTF_REQUIRE((scale == nullptr) == (shift == nullptr), "%s: scale and shift go together", who);
    return KTF_OK;
}

// The alignment of y / y_lo that the vector stores of the 256 x 256 ring epilogues and of tdnn_bf16g_kernel assume (with ldy % 4 == 0, which
// their dispatch tests): 16 bytes for fp32 rows, 8 bytes for 16-bit rows. (tdnn_bf16h_kernel, the bf16 rows of tdnn_bf16r16_kernel and the
// 128 x 128 tdnn_bf16_kernel test or need none; include/ktf_hip.h has the table.) Pooled launches write no y.
#define TDNN_REQUIRE_Y_ALIGNED(p, pooled)                                                                                       \
    if (!(pooled)) {                                                                                                            \
        const uintptr_t ymask_ = (p).y_dtype == KTF_F32 ? 15 : 7;                                                               \
        KTF_REQUIRE(((reinterpret_cast<uintptr_t>((p).y) | reinterpret_cast<uintptr_t>((p).y_lo)) & ymask_) == 0,               \
                    "ktf_tdnn: y (and y_lo) must be %d-byte aligned for this layer's kernel (units > 128 or a 64-multiple input width, ldy %% 4 == 0)", \
                    (int)ymask_ + 1);                                                                                           \
    }

// per-family launchers (validation of the family's own constraints + launch); `p` is filled by tdnn_gemm.hip
int tdnn_launch_f32(const TdnnParams& p, const KtfTdnnDesc* d, int64_t B, int64_t Tout, hipStream_t st);
int tdnn_launch_x4(const TdnnParams& p, const KtfTdnnDesc* d, int64_t B, int64_t Tout, double* stats, hipStream_t st);   // tdnn_pair.hip
int tdnn_launch_16(const TdnnParams& p, const KtfTdnnDesc* d, int64_t B, int64_t Tout, int64_t ldy, double* stats_sums, hipStream_t st);
int tdnn_launch_split(const TdnnParams& p, const KtfTdnnDesc* d, int64_t B, int64_t Tout, int64_t ldy, bool split_in, double* stats_sums,
                      hipStream_t st);
