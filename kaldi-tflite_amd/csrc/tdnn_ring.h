// What the 16-bit "ring" GEMM kernels (tdnn_bf16.hip, tdnn_split.hip) share, each with one definition: the 256 x 256 tile constants,
// the feed of the LDS ring (context iterator + operand DMAs), the epilogue value (bias -> activation -> BatchNorm affine), the column
// constants in registers and in LDS, the bf16 packs, and the epilogues of the 32x32 and the 16x16 accumulator layouts (LDS-staged
// coalesced stores, direct and packed stores of the swapped-operand layout, fused pooling sums).
// (The tile header every one of these kernels starts with is TDNN_TILE_HEADER, tdnn_common.h.)
#pragma once
#include "tdnn_common.h"

#define R_BM 256
#define R_BN 256
#define R_BK 32
#define R_NSTAGE 4
#define R_TILE_BYTES (256 * R_BK * 2)           // 16 KiB per operand
#define R_STAGE_BYTES (2 * R_TILE_BYTES)        // 32 KiB
#define R_EPI_PITCH 260
#define R_LDS_BYTES (R_NSTAGE * R_STAGE_BYTES)  // 131,072 B (epilogue staging needs 64*260*4 = 66,560 B)

// cache policy bits of the operand DMAs (aux of global_load_lds: 1 = sc0, 2 = nt, 16 = sc1); A = activations, W = weights.
// Measured (tools/gemm_layers.py): nt on the activations -10..-20 %, nt on the weights -10..-40 %, sc0 no change: both
// streams live on L2 hits (other N-tiles / context offsets re-read the activations, every CU re-reads the weights).
#ifndef KTF_AUX_A
#define KTF_AUX_A 0
#endif
#ifndef KTF_AUX_W
#define KTF_AUX_W 0
#endif

// ------------------------------------------------------------------------------------ feeding the ring
// The stage being issued and the DMAs that fill it. A stage is one K-step (R_BK columns of ONE context offset) of both operands.
// A thread issues its pieces of a tile 16 bytes per lane, PIECE bytes apart (its wave's 1 KiB at wave * 1024); the stages lie STAGE
// bytes apart, the kernel names the SLOT (is_ks & (NSTAGE - 1), or a wrap counter of its own). EB: bytes per activation element.
// The kernel provides the staging map: a_t[i] = input row of piece i's tile row before the context offset, a_cb[i] = byte offset of
// its (permuted) 16-byte chunk in the K-step's columns, w_ob[i] = byte offset of piece i's row and chunk in W.
// Every DMA address is a uniform 64-bit base + a per-lane 32-bit byte offset, so the K-loop carries no 64-bit vector arithmetic (an
// utterance's activations and a layer's weights are both < 4 GiB).
// (Macros over the kernel's locals b, len, rsm, wave: as an inlined struct with the same statements the compiler orders the tile
// setup differently and allocates other registers in every ring kernel.)
#define RING_FEED_BASES(EB)                                                                                            \
    const char* xb = reinterpret_cast<const char*>(p.x) + ((int64_t)b * p.T * p.ldx) * (EB);                           \
    const char* wb = reinterpret_cast<const char*>(p.w);                                                               \
    const unsigned ldxb = (unsigned)p.ldx * (EB);
// iterator over the stage being issued: K-step index, context, byte offset inside the context's columns, row offset of the context
#define RING_FEED_ITER(EB)                                                                                             \
    const int nk = p.ktot / R_BK;                                                                                      \
    const int lenm1 = len - 1;                                                                                         \
    int is_ks = 0, is_c = 0, is_db = 0, is_off = p.ctx[0];                                                             \
    const int dpad_b = p.din_pad * (EB);
// piece i of the A tile: its row of the stage's context, clamped to the utterance
#define RING_DMA_A(i, SLOT, STAGE, PIECE)                                                                              \
    {                                                                                                                  \
        int r_ = a_t[i] + is_off;                                                                                      \
        r_ = r_ < 0 ? 0 : (r_ > lenm1 ? lenm1 : r_);                                                                   \
        const unsigned vo_ = (unsigned)r_ * ldxb + a_cb[i] + (unsigned)is_db;                                          \
        __builtin_amdgcn_global_load_lds((glb_ptr_t*)(xb + vo_),                                                       \
            (lds_ptr_t*)(rsm + (SLOT) * (STAGE) + wave * 1024 + (i) * (PIECE)), 16, 0, KTF_AUX_A);                     \
    }
// piece i of the tile of weight plane W (bf16) that sits WOFF bytes into the stage
#define RING_DMA_W(i, W, SLOT, STAGE, WOFF, PIECE)                                                                     \
    {                                                                                                                  \
        const unsigned vo_ = w_ob[i] + (unsigned)(is_ks * (R_BK * 2));                                                 \
        __builtin_amdgcn_global_load_lds((glb_ptr_t*)((W) + vo_),                                                      \
            (lds_ptr_t*)(rsm + (SLOT) * (STAGE) + (WOFF) + wave * 1024 + (i) * (PIECE)), 16, 0, KTF_AUX_W);            \
    }
// on to the next K-step: the next R_BK columns of the context, or the next context
#define RING_ADVANCE(EB)                                                                                               \
    {                                                                                                                  \
        ++is_ks;                                                                                                       \
        is_db += R_BK * (EB);                                                                                          \
        if (is_db == dpad_b) {                                                                                         \
            is_db = 0;                                                                                                 \
            ++is_c;                                                                                                    \
            is_off = (is_c < p.nctx) ? p.ctx[is_c] : 0;                                                                \
        }                                                                                                              \
    }
// the ring of tdnn_bf16r_kernel and tdnn_bf16r16_kernel: R_NSTAGE stages of A | W, two pieces of each per thread
#define R_DMA_A(i) RING_DMA_A(i, is_ks & (R_NSTAGE - 1), R_STAGE_BYTES, 8192)
#define R_DMA_B(i) RING_DMA_W(i, wb, is_ks & (R_NSTAGE - 1), R_STAGE_BYTES, R_TILE_BYTES, 8192)

// ------------------------------------------------------------------------------------ epilogue value, column constants, packs
// (Macros where a function, inlined, changed the code of the kernels: the compiler simplifies a function's body on its own first.)
// The epilogue value: bias -> activation -> BatchNorm affine. ReLU is fmaxf here (NaN -> 0), not apply_act's NaN-propagating form.
// EPI_VALUE_NB: for accumulators that were preloaded with the bias.
#define EPI_VALUE_NB(ACT, V, SC, SH)                                                                                   \
    ({                                                                                                                 \
        float v_ = (V);                                                                                                \
        if (ACT == KTF_ACT_RELU) v_ = fmaxf(v_, 0.0f);                                                                 \
        else if (ACT != KTF_ACT_NONE) v_ = apply_act(v_, ACT);                                                         \
        v_ = v_ * (SC) + (SH);                                                                                         \
        v_;                                                                                                            \
    })
#define EPI_VALUE(ACT, ACC, BIAS, SC, SH) EPI_VALUE_NB(ACT, (ACC) + (BIAS), SC, SH)
// ... one or the other by the compile-time flag HAS_BIAS
#define EPI_VALUE_IF(ACT, HAS_BIAS, ACC, BIAS, SC, SH) (HAS_BIAS ? EPI_VALUE(ACT, ACC, BIAS, SC, SH) : EPI_VALUE_NB(ACT, ACC, SC, SH))

// BIAS, SC, SH = bias / BatchNorm scale / shift of unit N (0 / 1 / 0 for the pad columns of the last N-tile and for absent vectors):
// into a lane's registers, one column or four consecutive ones at a time, or -- thread tid, column n0 + tid -- into the LDS image
// bias[BN] | scale[BN] | shift[BN] that the swapped-operand epilogues read (COL_PRM_PARK)
#define COL_PRM(N, BIAS, SC, SH)                                                                                       \
    {                                                                                                                  \
        const int n = (N);                                                                                             \
        const bool nv = n < p.units;                                                                                   \
        BIAS = (nv && p.bias) ? p.bias[n] : 0.0f;                                                                      \
        SC = (nv && p.scale) ? p.scale[n] : 1.0f;                                                                      \
        SH = (nv && p.shift) ? p.shift[n] : 0.0f;                                                                      \
    }
#define COL_PRM_PARK(PRM, BN) COL_PRM(n0 + tid, (PRM)[tid], (PRM)[(BN) + tid], (PRM)[2 * (BN) + tid])

// two / four values as packed bf16; PACK_BF16X2_LO: the residual (lo) plane of split-bf16 values, bf16(v - hi), from the values
// and their bf16 HA, HB (the hi plane)
#define PACK_BF16X2(A, B) ((unsigned)f2bf(A) | ((unsigned)f2bf(B) << 16))
#define PACK_BF16X2_LO(A, B, HA, HB) PACK_BF16X2((A) - bf2f(HA), (B) - bf2f(HB))
#define PACK_BF16X4(A, B, C, D)                                                                                        \
    ({                                                                                                                 \
        uint2 pk_;                                                                                                     \
        pk_.x = PACK_BF16X2(A, B);                                                                                     \
        pk_.y = PACK_BF16X2(C, D);                                                                                     \
        pk_;                                                                                                           \
    })

// ------------------------------------------------------------------------------------ 32x32 accumulator layout
// Epilogue shared by the 256x256 kernels: bias -> activation -> BatchNorm affine on the 4x2 accumulator tiles of each wave,
// then either (STATS) fp64 column sums / sums of squares into stats[b][0|1][unit], or four passes of LDS-staged,
// fully coalesced row stores (one 256-column row per wave-instruction).
template <int ACT, bool STATS>
__device__ __forceinline__ void ring_epilogue(f32x16 (&acc)[4][2], const TdnnParams& p, double* __restrict__ stats,
                                              unsigned char* rsm, int b, int t0, int n0, int out_len, int wm, int wn,
                                              int wave, int lane) {
    // ---- epilogue: four passes of 64 staged rows (wave (wm, wn) contributes its 32 x 64 block of pass i)
    float* et = reinterpret_cast<float*>(rsm);
    float bias[2], sc[2], sh[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) COL_PRM(n0 + wn * 64 + j * 32 + (lane & 31), bias[j], sc[j], sh[j])
    const int rows_valid = out_len - t0;
    if (STATS) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double s = 0.0, q = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = wm * 128 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    const float v = EPI_VALUE(ACT, acc[i][j][r], bias[j], sc[j], sh[j]);
                    if (m < rows_valid) {
                        s += (double)v;
                        q += (double)v * (double)v;
                    }
                }
            }
            s += __shfl_xor(s, 32, 64);      // the two half-waves hold the same column
            q += __shfl_xor(q, 32, 64);
            const int n = n0 + wn * 64 + j * 32 + (lane & 31);
            if (lane < 32 && n < p.units) stats_out(stats, p, b, pool_block128().slot_of(t0 + wm * 128), n, s, q);
        }
        return;
    }
    const int64_t out_row0 = (int64_t)b * p.Tout + t0;
    const int nl = lane * 4;                      // this lane's 4 columns of the 256-wide staged row
    const int n = n0 + nl;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = wn * 64 + j * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int srow = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                et[srow * R_EPI_PITCH + col] = EPI_VALUE(ACT, acc[i][j][r], bias[j], sc[j], sh[j]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int sp = 0; sp < 8; ++sp) {
            const int srow = sp * 8 + wave;          // one staged row per wave: 256 contiguous columns
            const int m = (srow >> 5) * 128 + i * 32 + (srow & 31);
            if (m < rows_valid) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(et + srow * R_EPI_PITCH + nl);
                const int64_t off = (out_row0 + m) * p.ldy + n;
                if (n + 4 <= p.units) {
                    if (p.y_dtype == KTF_F32) {
                        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.y) + off) = v;
                    } else {
                        const unsigned short h0 = f2bf(v.x), h1 = f2bf(v.y), h2 = f2bf(v.z), h3 = f2bf(v.w);
                        *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(p.y) + off) = PACK_BF16X4(v.x, v.y, v.z, v.w);
                        if (p.y_lo) {            // split-bf16 output: the residual plane, the next layer's lo operand
                            uint2 pl;
                            pl.x = PACK_BF16X2_LO(v.x, v.y, h0, h1);
                            pl.y = PACK_BF16X2_LO(v.z, v.w, h2, h3);
                            *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(p.y_lo) + off) = pl;
                        }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (n + e < p.units) {
                            if (p.y_dtype == KTF_F32) {
                                reinterpret_cast<float*>(p.y)[off + e] = v[e];
                            } else {
                                const unsigned short h = f2bf(v[e]);
                                reinterpret_cast<unsigned short*>(p.y)[off + e] = h;
                                if (p.y_lo) reinterpret_cast<unsigned short*>(p.y_lo)[off + e] = f2bf(v[e] - bf2f(h));
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------ 16x16 accumulator layout
// STATS: instead of storing y, the epilogue adds every column's sum and sum of squares over the tile's valid rows (fp64)
// into stats[b][0|1][unit] — statistics pooling fused into the producing GEMM, the (B,T,units) activation never exists.
// The wave's 128 x 64 block is 8 x 4 tiles of v_mfma_f32_16x16x32_bf16: one MFMA consumes the whole 32-deep K-step, and the chip
// holds a higher clock on this shape under load (MI355X_MICROARCH.md, DVFS item 7). Fragment lane map: row = lane&15, 16-B chunk =
// lane>>4, so the conflict-free chunk permutation is c ^ ((4 - (row>>2)) & 3) (each ds_read_b128 lane group then covers all 16 slots).
// Natural operand order (x fragment as A):  acc[i][j][r] = out[row i*16 + (lane>>4)*4 + r][col j*16 + (lane&15)]  of the block;
// swapped (W fragment as A, the non-reducing epilogues): acc[i][j][e] = out[row i*16 + (lane&15)][col j*16 + (lane>>4)*4 + e],
// four CONSECUTIVE output columns of one row per lane. Products commute and the K order is the same: the values are the same bits.
typedef __attribute__((ext_vector_type(4))) float f32x4v;
typedef __attribute__((ext_vector_type(8))) _Float16 hfrag8;
__device__ __forceinline__ f32x4v mfma16x16x32(const bfrag8& a, const bfrag8& b, const f32x4v& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// per-lane epilogue constants of the natural layout: bias / BatchNorm scale / shift of the lane's four columns
struct Epi16Prm { float bias[4], sc[4], sh[4]; };
__device__ __forceinline__ Epi16Prm epi16_load(const TdnnParams& p, int n0, int wn, int lane) {
    Epi16Prm e;
#pragma unroll
    for (int j = 0; j < 4; ++j) COL_PRM(n0 + wn * 64 + j * 16 + (lane & 15), e.bias[j], e.sc[j], e.sh[j])
    return e;
}
// ... and of the swapped layout: of the lane's 4 x 4 consecutive columns, from global memory or from the LDS image of COL_PRM_PARK
// (BIAS false: the accumulators were preloaded with it)
struct Epi16Cols { f32x4v bias[4], sc[4], sh[4]; };
__device__ __forceinline__ void epi16_cols_load(Epi16Cols& c, const TdnnParams& p, int n0, int wn, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) COL_PRM(n0 + wn * 64 + j * 16 + (lane >> 4) * 4 + e, c.bias[j][e], c.sc[j][e], c.sh[j][e])
    }
}
template <int BN, bool BIAS>
__device__ __forceinline__ void epi16_cols_lds(Epi16Cols& c, const float* prm, int wn, int lane) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int nl = wn * 64 + j * 16 + (lane >> 4) * 4;
        if (BIAS) c.bias[j] = *reinterpret_cast<const f32x4v*>(prm + nl);
        c.sc[j] = *reinterpret_cast<const f32x4v*>(prm + BN + nl);
        c.sh[j] = *reinterpret_cast<const f32x4v*>(prm + 2 * BN + nl);
    }
}
// the lane's four values of accumulator tile (i, j)
#define EPI16_VALUE4(ACT, BIAS, V, A, C, j)                                                                            \
    _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                                      \
        V[e] = EPI_VALUE_IF(ACT, BIAS, (A)[e], (C).bias[j][e], (C).sc[j][e], (C).sh[j][e]);

// 16-byte store of a piece of a 16-bit activation plane. The plane (1 GB per layer at 1024 utterances) is read by the NEXT
// launch only: written non-temporally it does not push the weights and the activation tiles two workgroups share out of the
// XCD's L2 (+1.2 % on the whole step; non-temporal operand LOADS cost 3-6 %).
__device__ __forceinline__ void st16(u32x4* dst, const u32x4& v) {
    if (KTF_X3_Y_NT) __builtin_nontemporal_store(v, dst);
    else *dst = v;
}

// FLAT (tdnn_x3s_kernel's flat row tiling; row-major outputs only): tile row m is output row rowmap[m] of the (B * Tout)-row output
// (an LDS table behind the staging image), t0 = 0 and out_len = the tile's valid rows.
template <int ACT, bool STATS, bool FLAT = false>
__device__ __forceinline__ void ring_epilogue16(f32x4v (&acc)[8][4], const TdnnParams& p, double* __restrict__ stats,
                                                unsigned char* rsm, int b, int t0, int n0, int out_len, int wm, int wn,
                                                int wave, int lane, const Epi16Prm& prm, const int* rowmap = nullptr) {
    float* et = reinterpret_cast<float*>(rsm);
    const float (&bias)[4] = prm.bias;
    const float (&sc)[4] = prm.sc;
    const float (&sh)[4] = prm.sh;
    const int rows_valid = out_len - t0;
    if (STATS) {
        const int rv = rows_valid - wm * 128;                  // valid rows of this wave's block (may be <= 0)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const PooledSums t = pooled_sums16<8, false>(lane, rv, [&](int i, int r) { return EPI_VALUE(ACT, acc[i][j][r], bias[j], sc[j], sh[j]); });
            const int n = n0 + wn * 64 + j * 16 + (lane & 15);
            if (lane < 16 && n < p.units) stats_out(stats, p, b, pool_block128().slot_of(t0 + wm * 128), n, t.s, t.q);
        }
        return;
    }
    const int64_t out_row0 = (int64_t)b * p.Tout + t0;
    const int nl = lane * 4;
    const int n = n0 + nl;
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {          // rows wm*128 + pass*32 .. +31 of both wave rows -> 64 staged rows
#pragma unroll
        for (int ih = 0; ih < 2; ++ih) {
            const int i = pass * 2 + ih;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = wn * 64 + j * 16 + (lane & 15);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int srow = wm * 32 + ih * 16 + (lane >> 4) * 4 + r;
                    et[srow * R_EPI_PITCH + col] = EPI_VALUE(ACT, acc[i][j][r], bias[j], sc[j], sh[j]);
                }
            }
        }
        __syncthreads();
        if (p.y_dtype != KTF_F32) {
            // bf16 output: 16-byte stores (8 columns per lane, two staged rows per wave instruction)
            const int n8 = n0 + (lane & 31) * 8;
#pragma unroll
            for (int sp = 0; sp < 4; ++sp) {
                const int srow = sp * 16 + wave * 2 + (lane >> 5);
                const int m = (srow >> 5) * 128 + pass * 32 + (srow & 31);
                if (m < rows_valid) {
                    const f32x4 v0 = *reinterpret_cast<const f32x4*>(et + srow * R_EPI_PITCH + (lane & 31) * 8);
                    const f32x4 v1 = *reinterpret_cast<const f32x4*>(et + srow * R_EPI_PITCH + (lane & 31) * 8 + 4);
                    const int64_t off = (FLAT ? (int64_t)rowmap[m] : out_row0 + m) * p.ldy + n8;
                    unsigned short* yp = reinterpret_cast<unsigned short*>(p.y) + off;
                    const float vv[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                    unsigned short hh[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) hh[e] = f2bf(vv[e]);
                    if (n8 + 8 <= p.units) {
                        u32x4 pk;
                        pk.x = (unsigned)hh[0] | ((unsigned)hh[1] << 16);
                        pk.y = (unsigned)hh[2] | ((unsigned)hh[3] << 16);
                        pk.z = (unsigned)hh[4] | ((unsigned)hh[5] << 16);
                        pk.w = (unsigned)hh[6] | ((unsigned)hh[7] << 16);
                        st16(reinterpret_cast<u32x4*>(yp), pk);
                        if (p.y_lo) {            // split-bf16 output: the residual plane, the next layer's lo operand
                            u32x4 pl;
                            pl.x = PACK_BF16X2_LO(vv[0], vv[1], hh[0], hh[1]); pl.y = PACK_BF16X2_LO(vv[2], vv[3], hh[2], hh[3]);
                            pl.z = PACK_BF16X2_LO(vv[4], vv[5], hh[4], hh[5]); pl.w = PACK_BF16X2_LO(vv[6], vv[7], hh[6], hh[7]);
                            st16(reinterpret_cast<u32x4*>(reinterpret_cast<unsigned short*>(p.y_lo) + off), pl);
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (n8 + e < p.units) {
                                yp[e] = hh[e];
                                if (p.y_lo) reinterpret_cast<unsigned short*>(p.y_lo)[off + e] = f2bf(vv[e] - bf2f(hh[e]));
                            }
                    }
                }
            }
        } else
#pragma unroll
        for (int sp = 0; sp < 8; ++sp) {
            const int srow = sp * 8 + wave;
            const int m = (srow >> 5) * 128 + pass * 32 + (srow & 31);
            if (m < rows_valid) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(et + srow * R_EPI_PITCH + nl);
                const int64_t off = (FLAT ? (int64_t)rowmap[m] : out_row0 + m) * p.ldy + n;
                if (n + 4 <= p.units) {
                    if (p.y_dtype == KTF_F32) {
                        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.y) + off) = v;
                    } else {
                        *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(p.y) + off) = PACK_BF16X4(v.x, v.y, v.z, v.w);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (n + e < p.units) {
                            if (p.y_dtype == KTF_F32) reinterpret_cast<float*>(p.y)[off + e] = v[e];
                            else reinterpret_cast<unsigned short*>(p.y)[off + e] = f2bf(v[e]);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// Non-reducing fp32 epilogue of the swapped layout: bias/ReLU/BatchNorm and the store need no LDS staging and no barrier; the four
// stores of one i (j = 0..3) complete a 128-byte line of each of the 16 rows. `row0`: first tile row of the wave's block. VEC_TEST: the
// 16-byte store also asks for an aligned y and ldy % 4 == 0 (a kernel whose launcher does not promise them).
template <int ACT, bool BIAS, bool VEC_TEST>
__device__ __forceinline__ void ring_epilogue16_direct(f32x4v (&acc)[8][4], const TdnnParams& p, const Epi16Cols& cols, int b, int t0,
                                                       int n0, int out_len, int row0, int wn, int lane) {
    const int c = lane & 15, g = lane >> 4;
    const int rows_valid = out_len - t0;
    const int64_t out_row0 = (int64_t)b * p.Tout + t0;
    float* ybase = reinterpret_cast<float*>(p.y);
    const bool vec_ok = !VEC_TEST || (((p.ldy & 3) == 0) && ((reinterpret_cast<uintptr_t>(p.y) & 15) == 0));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = row0 + i * 16 + c;
        if (m >= rows_valid) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4v v;
            EPI16_VALUE4(ACT, BIAS, v, acc[i][j], cols, j)
            const int n = n0 + wn * 64 + j * 16 + g * 4;
            float* yp = ybase + (out_row0 + m) * p.ldy + n;
            if (vec_ok && n + 4 <= p.units) {
                *reinterpret_cast<f32x4v*>(yp) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (n + e < p.units) yp[e] = v[e];
            }
        }
    }
}

// bf16-output epilogue of the swapped layout: bias/ReLU/BatchNorm and the bf16 pack happen in registers, each lane stages its four
// consecutive columns with one ds_write_b64 (row pitch 520 B: the 16 lanes of a store group cover all 32 banks), and after ONE
// barrier every wave streams 32 staged rows out with 16-byte stores (two 512-byte rows per wave instruction). The stores are
// issue-bound per instruction (T21), hence the wide form.
#define R16_PK_PITCH 520
// stages the wave's 128 x 64 block (first tile row `row0`) of the BM x 256 16-bit image
template <int ACT, bool BIAS>
__device__ __forceinline__ void r16_stage_pk(f32x4v (&acc)[8][4], const Epi16Cols& cols, unsigned char* rsm, int row0, int wn, int lane) {
    unsigned char* stg = rsm + (row0 + (lane & 15)) * R16_PK_PITCH + (wn * 64 + (lane >> 4) * 4) * 2;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4v v;
            EPI16_VALUE4(ACT, BIAS, v, acc[i][j], cols, j)
            *reinterpret_cast<uint2*>(stg + i * 16 * R16_PK_PITCH + j * 32) = PACK_BF16X4(v[0], v[1], v[2], v[3]);
        }
    }
}
// wave `wave` streams rows wave * 32 .. + 31 of the staged image out with 16-byte stores (two 512-byte rows per instruction)
__device__ __forceinline__ void r16_store_staged(const TdnnParams& p, const unsigned char* rsm, unsigned short* ybase, int b,
                                                 int t0, int n0, int out_len, int wave, int lane) {
    const int rows_valid = out_len - t0;
    const int64_t out_row0 = (int64_t)b * p.Tout + t0;
    const int n8 = n0 + (lane & 31) * 8;
    const bool wide = (n8 + 8 <= p.units) && ((p.ldy & 7) == 0) && ((reinterpret_cast<uintptr_t>(ybase) & 15) == 0);
#pragma unroll 4
    for (int sp = 0; sp < 16; ++sp) {
        const int m = wave * 32 + sp * 2 + (lane >> 5);
        if (m < rows_valid) {
            const unsigned char* src = rsm + m * R16_PK_PITCH + (lane & 31) * 16;
            const uint2 lo = *reinterpret_cast<const uint2*>(src);
            const uint2 hi = *reinterpret_cast<const uint2*>(src + 8);
            unsigned short* yp = ybase + (out_row0 + m) * p.ldy + n8;
            if (wide) {
                u32x4 o;
                o.x = lo.x; o.y = lo.y; o.z = hi.x; o.w = hi.y;
                *reinterpret_cast<u32x4*>(yp) = o;
            } else {
                const unsigned w4[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (n8 + e < p.units) yp[e] = (unsigned short)(w4[e >> 1] >> ((e & 1) * 16));
            }
        }
    }
}
