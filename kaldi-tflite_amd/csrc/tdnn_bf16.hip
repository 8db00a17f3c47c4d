// KTF_GEMM_BF16 (one bf16 MFMA pass; outside the 1e-4 tolerance, BASELINE config 3's precision) and the small-layer
// forms of KTF_GEMM_BF16X3: 128 x 128 register-/DMA-staged tiles, the 256 x 256 ring kernels on 32x32x16 (sigmoid / tanh) and
// 16x16x32 MFMAs, and the 128 x 256 two-workgroups-per-CU kernel for K <= 768. The ring kernels keep their tile setup and their
// K-loops here; the ring's feed, the epilogue value, the column constants and the epilogues are tdnn_ring.h's.
#include "tdnn_ring.h"

// ------------------------------------------------------------------------------------ BF16 / BF16X3
// 128x128 block tile, K-step BK (bf16), 4 waves as 2x2, each wave 64x64 = 2x2 tiles of 32x32x16 MFMA.
// LDS rows are padded by 16 B so that the 16-lane groups of ds_read_b128 hit 16 distinct 16-B slots.
#define BF_BM 128
#define BF_BN 128

template <int BK>
struct BfCfg {
    static constexpr int PITCH = BK + 8;                    // bf16 elements per LDS row
    static constexpr int CHUNKS = BK / 8;                   // 16-B chunks per row
    static constexpr int PER_THREAD = (128 * CHUNKS) / 256; // chunks each thread stages per operand
};

__device__ __forceinline__ u32x4 pack_bf16x8(const fv4& lo, const fv4& hi) {
    u32x4 r;
    r.x = PACK_BF16X2(lo.x, lo.y);
    r.y = PACK_BF16X2(lo.z, lo.w);
    r.z = PACK_BF16X2(hi.x, hi.y);
    r.w = PACK_BF16X2(hi.z, hi.w);
    return r;
}
__device__ __forceinline__ fv4 bf_residual(const fv4& v, unsigned p01, unsigned p23) {
    fv4 r;
    r.x = v.x - bf2f((unsigned short)(p01 & 0xffff)); r.y = v.y - bf2f((unsigned short)(p01 >> 16));
    r.z = v.z - bf2f((unsigned short)(p23 & 0xffff)); r.w = v.w - bf2f((unsigned short)(p23 >> 16));
    return r;
}

// XF32: activations are fp32 in memory (converted while staging); X3: split-bf16 3-pass mode (needs XF32).
template <int BK, bool XF32, bool X3>
__global__ __launch_bounds__(256) void tdnn_bf16_kernel(TdnnParams p) {
    using C = BfCfg<BK>;
    constexpr int NBUF_A = X3 ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) unsigned short smem[];
    // layout: [stage 2][A hi (,A lo)][B hi (,B lo)] each 128 x PITCH
    constexpr int TILE = 128 * C::PITCH;
    constexpr int STAGE = TILE * 2 * NBUF_A;

    TDNN_TILE3D_HEADER(BF_BM, BF_BN)
    const int wave = tid >> 6, wm = wave >> 1, wn = wave & 1;

    const int64_t xbase = (int64_t)b * p.T * p.ldx;
    const unsigned short* wb = reinterpret_cast<const unsigned short*>(p.w);
    const unsigned short* wlo = reinterpret_cast<const unsigned short*>(p.w_lo);

    int ld_row[C::PER_THREAD], ld_chunk[C::PER_THREAD], a_t[C::PER_THREAD];
#pragma unroll
    for (int i = 0; i < C::PER_THREAD; ++i) {
        const int id = tid + 256 * i;
        ld_row[i] = id / C::CHUNKS;
        ld_chunk[i] = id % C::CHUNKS;
        a_t[i] = start + (t0 + ld_row[i]) * p.sub;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int nk = p.ktot / BK;
    const int steps_per_ctx = p.din_pad / BK;
    u32x4 ra[C::PER_THREAD], ralo[C::PER_THREAD], rb[C::PER_THREAD], rblo[C::PER_THREAD];

#define BF_LOAD_GLOBAL(KS)                                                                                        \
    {                                                                                                             \
        const int ks_ = (KS);                                                                                     \
        const int c_ = ks_ / steps_per_ctx;                                                                       \
        const int d0_ = (ks_ - c_ * steps_per_ctx) * BK;                                                          \
        const int off_ = p.ctx[c_];                                                                               \
        _Pragma("unroll") for (int i = 0; i < C::PER_THREAD; ++i) {                                               \
            int r = a_t[i] + off_;                                                                                \
            r = r < 0 ? 0 : (r > len - 1 ? len - 1 : r);                                                          \
            const int64_t e = xbase + (int64_t)r * p.ldx + d0_ + ld_chunk[i] * 8;                                 \
            if (XF32) {                                                                                           \
                const fv4* src = reinterpret_cast<const fv4*>(reinterpret_cast<const float*>(p.x) + e);           \
                const fv4 v0 = src[0], v1 = src[1];                                                               \
                ra[i] = pack_bf16x8(v0, v1);                                                                      \
                if (X3) ralo[i] = pack_bf16x8(bf_residual(v0, ra[i].x, ra[i].y), bf_residual(v1, ra[i].z, ra[i].w)); \
            } else {                                                                                              \
                ra[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned short*>(p.x) + e);        \
            }                                                                                                     \
            const int64_t we = (int64_t)(n0 + ld_row[i]) * p.ktot + (int64_t)ks_ * BK + ld_chunk[i] * 8;          \
            rb[i] = *reinterpret_cast<const u32x4*>(wb + we);                                                     \
            if (X3) rblo[i] = *reinterpret_cast<const u32x4*>(wlo + we);                                          \
        }                                                                                                         \
    }
#define BF_STORE_LDS(STG)                                                                      \
    {                                                                                          \
        unsigned short* base = smem + (STG) * STAGE;                                           \
        _Pragma("unroll") for (int i = 0; i < C::PER_THREAD; ++i) {                            \
            const int o = ld_row[i] * C::PITCH + ld_chunk[i] * 8;                              \
            *reinterpret_cast<u32x4*>(base + o) = ra[i];                                       \
            if (X3) *reinterpret_cast<u32x4*>(base + TILE + o) = ralo[i];                      \
            *reinterpret_cast<u32x4*>(base + NBUF_A * TILE + o) = rb[i];                       \
            if (X3) *reinterpret_cast<u32x4*>(base + NBUF_A * TILE + TILE + o) = rblo[i];      \
        }                                                                                      \
    }

    BF_LOAD_GLOBAL(0);
    BF_STORE_LDS(0);
    __syncthreads();
    // fragment base offsets: lane (r = lane&31, h = lane>>5) reads row r, k = 16*kstep + 8*h .. +7
    const int a_off = (wm * 64 + (lane & 31)) * C::PITCH + (lane >> 5) * 8;
    const int b_off = (wn * 64 + (lane & 31)) * C::PITCH + (lane >> 5) * 8;
    for (int ks = 0; ks < nk; ++ks) {
        const int stage = ks & 1;
        if (ks + 1 < nk) BF_LOAD_GLOBAL(ks + 1);
        const unsigned short* sa = smem + stage * STAGE;
        const unsigned short* sb = sa + NBUF_A * TILE;
#pragma unroll
        for (int kk = 0; kk < BK; kk += 16) {
            bfrag8 a[2], bq[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = *reinterpret_cast<const bfrag8*>(sa + a_off + i * 32 * C::PITCH + kk);
                bq[i] = *reinterpret_cast<const bfrag8*>(sb + b_off + i * 32 * C::PITCH + kk);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], bq[j], acc[i][j], 0, 0, 0);
            if (X3) {
                bfrag8 al[2], bl[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    al[i] = *reinterpret_cast<const bfrag8*>(sa + TILE + a_off + i * 32 * C::PITCH + kk);
                    bl[i] = *reinterpret_cast<const bfrag8*>(sb + TILE + b_off + i * 32 * C::PITCH + kk);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bq[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], bl[j], acc[i][j], 0, 0, 0);
                    }
            }
        }
        if (ks + 1 < nk) BF_STORE_LDS(stage ^ 1);
        __syncthreads();
    }

    const int rows_valid = out_len - t0;
    const int64_t out_row0 = (int64_t)b * p.Tout + t0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            store_tile32(acc[i][j], p, out_row0, rows_valid, wm * 64 + i * 32, n0 + wn * 64 + j * 32, lane);
}

// ------------------------------------------------------------------------------------ BF16, direct-to-LDS staging
// The throughput kernel for bf16 activations: 128x128 tile, K-step 64, both operands staged with
// global_load_lds_dwordx4 (no VGPR round trip, no ds_write). The LDS image is lane-linear ([row][64] bf16, 128-B rows),
// so bank conflicts of the ds_read_b128 fragment reads are removed by permuting the 16-B chunks of each row on the
// SOURCE address (chunk' = chunk ^ ((row>>1)&7)) and applying the same involution on the read address.
// 1-D grid, XCD-aware (TDNN_TILE_HEADER). The epilogue stages the fp32 accumulators through LDS and writes whole 256-B row segments.


#define G_BM 128
#define G_BN 128
#define G_BK 64
#define G_TILE_BYTES (128 * G_BK * 2)          // one operand tile: 16 KiB
#define G_STAGE_BYTES (2 * G_TILE_BYTES)       // A + B
#define G_EPI_PITCH 132                         // floats per staged output row
#define G_LDS_BYTES (128 * G_EPI_PITCH * 4)    // 67,584 B >= 2 stages (65,536 B)

__global__ __launch_bounds__(256) void tdnn_bf16g_kernel(TdnnParams p, int mtiles, int ntiles, int gtiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gsm[];
    TDNN_TILE_HEADER(G_BM, G_BN, blockIdx.x)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    const unsigned short* xb = reinterpret_cast<const unsigned short*>(p.x) + (int64_t)b * p.T * p.ldx;
    const unsigned short* wb = reinterpret_cast<const unsigned short*>(p.w);

    // staging map: chunk q = i*256 + tid -> row q/8, LDS position q%8, global chunk (q%8) ^ ((row>>1)&7)
    int a_t[4];
    int src_chunk[4];
    const unsigned short* wrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = i * 256 + tid;
        const int row = q >> 3;
        src_chunk[i] = ((q & 7) ^ ((row >> 1) & 7)) * 8;
        a_t[i] = start + (t0 + row) * p.sub;
        wrow[i] = wb + (int64_t)(n0 + row) * p.ktot + src_chunk[i];
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    const int nk = p.ktot / G_BK;
    const int steps_per_ctx = p.din_pad / G_BK;

#define G_STAGE(STG, KS)                                                                                              \
    {                                                                                                                 \
        const int ks_ = (KS);                                                                                         \
        const int c_ = ks_ / steps_per_ctx;                                                                           \
        const int d0_ = (ks_ - c_ * steps_per_ctx) * G_BK;                                                            \
        const int off_ = p.ctx[c_];                                                                                   \
        unsigned char* sa_ = gsm + (STG) * G_STAGE_BYTES + wave * 1024;                                               \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                               \
            int r = a_t[i] + off_;                                                                                    \
            r = r < 0 ? 0 : (r > len - 1 ? len - 1 : r);                                                              \
            const unsigned short* ga = xb + (int64_t)r * p.ldx + d0_ + src_chunk[i];                                  \
            __builtin_amdgcn_global_load_lds((glb_ptr_t*)ga, (lds_ptr_t*)(sa_ + i * 4096), 16, 0, 0);                  \
            const unsigned short* gb = wrow[i] + (int64_t)ks_ * G_BK;                                                 \
            __builtin_amdgcn_global_load_lds((glb_ptr_t*)gb, (lds_ptr_t*)(sa_ + G_TILE_BYTES + i * 4096), 16, 0, 0);  \
        }                                                                                                             \
    }

    G_STAGE(0, 0);
    __syncthreads();
    // fragment addressing: lane (r = lane&31, h = lane>>5) reads row R, k = kk + 8h .. +7  ->  chunk (kk/8 + h) ^ ((R>>1)&7)
    const int rsw = ((lane & 31) >> 1) & 7;
    const int a_row_off = (wm * 64 + (lane & 31)) * 128;   // bytes
    const int b_row_off = (wn * 64 + (lane & 31)) * 128;
    const int hsel = lane >> 5;
    for (int ks = 0; ks < nk; ++ks) {
        const int stage = ks & 1;
        if (ks + 1 < nk) G_STAGE(stage ^ 1, ks + 1);
        const unsigned char* sa = gsm + stage * G_STAGE_BYTES;
        const unsigned char* sb = sa + G_TILE_BYTES;
#pragma unroll
        for (int kk = 0; kk < G_BK / 16; ++kk) {
            const int coff = (((kk * 2 + hsel) ^ rsw) << 4);
            bfrag8 a[2], bq[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = *reinterpret_cast<const bfrag8*>(sa + a_row_off + i * 32 * 128 + coff);
                bq[i] = *reinterpret_cast<const bfrag8*>(sb + b_row_off + i * 32 * 128 + coff);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], bq[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#undef G_STAGE

    // ---- epilogue: bias / activation / BN affine on the accumulators, stage fp32 tile in LDS, coalesced row stores
    float* et = reinterpret_cast<float*>(gsm);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int nl = wn * 64 + j * 32 + (lane & 31);
        float bias, sc, sh;
        COL_PRM(n0 + nl, bias, sc, sh)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                float v = apply_act(acc[i][j][r] + bias, p.act);
                if (p.scale) v = v * sc + sh;
                et[m * G_EPI_PITCH + nl] = v;
            }
        }
    }
    __syncthreads();
    const int rows_valid = out_len - t0;
    const int64_t out_row0 = (int64_t)b * p.Tout + t0;
    const int cl = (tid & 15) * 4;                 // 4 columns at cl and 4 at 64 + cl
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
        const int m = pass * 16 + (tid >> 4);
        if (m >= rows_valid) continue;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int nl = half * 64 + cl;
            const int n = n0 + nl;
            const f32x4 v = *reinterpret_cast<const f32x4*>(et + m * G_EPI_PITCH + nl);
            const int64_t off = (out_row0 + m) * p.ldy + n;
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
}

// ------------------------------------------------------------------------------------ BF16, 256x256 tile, 4-deep LDS ring
// The large-layer throughput kernel. One workgroup = 8 waves (2 x 4, each 128 x 64 = 4 x 2 MFMA 32x32 tiles) owns a
// 256 x 256 output tile: 32 B of staged operand per MFMA-cycle-pair instead of 64 (the 128x128 kernel is L2->LDS bound).
// Operands are staged with global_load_lds_dwordx4 into a ring of four 32 KiB stages (K-step 32: 64-B rows, chunk
// permutation chunk ^ ((row>>2)&3) on the source, same involution on the read). Loads run THREE K-steps ahead and stay
// in flight across the single raw s_barrier per K-step: the wait before the barrier is a counted s_waitcnt vmcnt(8|4|0)
// (4 DMA instructions per thread per stage), never a drain.
template <int ACT, bool STATS>
__global__ __launch_bounds__(512) void tdnn_bf16r_kernel(TdnnParams p, int mtiles, int ntiles, int gtiles,
                                                         double* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rsm[];
    TDNN_TILE_HEADER(R_BM, R_BN, blockIdx.x)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform: LDS-DMA bases stay in SGPRs
    const int wm = wave >> 2, wn = wave & 3;

    RING_FEED_BASES(2)

    // staging map: chunk q = i*512 + tid -> row q/4, LDS position q%4, global chunk (q%4) ^ ((row>>2)&3)
    int a_t[2];
    unsigned a_cb[2], w_ob[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = i * 512 + tid;
        const int row = q >> 2;
        const unsigned chunk = (unsigned)(((q & 3) ^ ((row >> 2) & 3)) * 16);   // bytes
        a_cb[i] = chunk;
        a_t[i] = start + (t0 + row) * p.sub;
        w_ob[i] = (unsigned)(n0 + row) * (unsigned)p.ktot * 2u + chunk;
    }

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    RING_FEED_ITER(2)

    // prologue: three stages in flight
    for (int s_ = 0; s_ < 3 && s_ < nk; ++s_) {
        R_DMA_A(0) R_DMA_B(0) R_DMA_A(1) R_DMA_B(1)
        RING_ADVANCE(2)
    }

    const int rsw = ((lane & 31) >> 2) & 3;
    const int a_row_off = (wm * 128 + (lane & 31)) * 64;   // bytes (64-B rows)
    const int b_row_off = (wn * 64 + (lane & 31)) * 64;
    const int hsel = lane >> 5;
    const int coff0 = ((hsel ^ rsw) << 4), coff1 = (((2 + hsel) ^ rsw) << 4);
    // Software pipeline: the barrier of K-step ks certifies stages ks AND ks+1 (one stage = 4 DMA instructions per thread
    // stays in flight), so the first-half fragments of stage ks+1 are read during the MFMAs of stage ks and the matrix
    // pipe restarts right after the next barrier instead of waiting for an LDS read burst of all 8 lock-stepped waves.
    bfrag8 a0[4], b0[2];     // fragments of (current stage, k-half 0)
    for (int ks = 0; ks < nk; ++ks) {
        if (ks + 2 < nk) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // every wave is past the barrier, i.e. has finished reading stage ks-1: that buffer is refilled with stage ks+3
        // (the iterator's stage); its four DMA instructions are spread between the MFMA groups
        const bool refill = is_ks < nk;
        const unsigned char* sa = rsm + (ks & (R_NSTAGE - 1)) * R_STAGE_BYTES;
        const unsigned char* sb = sa + R_TILE_BYTES;
        if (ks == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) a0[i] = *reinterpret_cast<const bfrag8*>(sa + a_row_off + i * 32 * 64 + coff0);
#pragma unroll
            for (int j = 0; j < 2; ++j) b0[j] = *reinterpret_cast<const bfrag8*>(sb + b_row_off + j * 32 * 64 + coff0);
        }
        bfrag8 a1[4], b1[2];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int i = half * 2; i < half * 2 + 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[i], b0[j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);   // keep the MFMA group ahead of the LDS reads / DMA that follow it
            if (half == 0) {
                // second-half fragments of this stage: issued behind the first MFMA group so their latency is covered
#pragma unroll
                for (int i = 0; i < 4; ++i) a1[i] = *reinterpret_cast<const bfrag8*>(sa + a_row_off + i * 32 * 64 + coff1);
#pragma unroll
                for (int j = 0; j < 2; ++j) b1[j] = *reinterpret_cast<const bfrag8*>(sb + b_row_off + j * 32 * 64 + coff1);
            }
            if (refill) {
                if (half == 0) R_DMA_A(0) else R_DMA_B(0)
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int i = half * 2; i < half * 2 + 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[i], b1[j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (half == 0 && ks + 1 < nk) {
                // pre-read the first-half fragments of stage ks+1 (landed and visible since this K-step's barrier); all
                // MFMAs that consume the old a0/b0 have been issued
                const unsigned char* san = rsm + ((ks + 1) & (R_NSTAGE - 1)) * R_STAGE_BYTES;
                const unsigned char* sbn = san + R_TILE_BYTES;
#pragma unroll
                for (int i = 0; i < 4; ++i) a0[i] = *reinterpret_cast<const bfrag8*>(san + a_row_off + i * 32 * 64 + coff0);
#pragma unroll
                for (int j = 0; j < 2; ++j) b0[j] = *reinterpret_cast<const bfrag8*>(sbn + b_row_off + j * 32 * 64 + coff0);
            }
            if (refill) {
                if (half == 0) R_DMA_A(1) else R_DMA_B(1)
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (is_ks < nk) RING_ADVANCE(2)
    }
    __syncthreads();   // all fragment reads done before the LDS is reused by the epilogue

    ring_epilogue<ACT, STATS>(acc, p, stats, rsm, b, t0, n0, out_len, wm, wn, wave, lane);
}

// LDS of the 16x16x32 kernel: the ring, reused as the 256 x 520-byte staging image of r16_stage_pk, and behind it bias | scale |
// shift of the tile's 256 columns (COL_PRM_PARK)
#define R16_PRM_OFF (R_BM * R16_PK_PITCH)
#define R16_LDS_BYTES (R16_PRM_OFF + 3 * R_BN * 4)      // 136,192 B


template <int ACT, bool STATS>
__device__ __forceinline__ void r16_tile(const TdnnParams& p, int mtiles, int ntiles, int gtiles,
                                         double* __restrict__ stats, unsigned char* rsm, const int id) {
    TDNN_TILE_HEADER(R_BM, R_BN, id)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    float* prm = reinterpret_cast<float*>(rsm + R16_PRM_OFF);
    if (!STATS && tid < R_BN) COL_PRM_PARK(prm, R_BN)

    RING_FEED_BASES(2)

    int a_t[2];
    unsigned a_cb[2], w_ob[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int q = i * 512 + tid;
        const int row = q >> 2;
        const unsigned chunk = (unsigned)(((q & 3) ^ ((4 - ((row >> 2) & 3)) & 3)) * 16);
        a_cb[i] = chunk;
        a_t[i] = start + (t0 + row) * p.sub;
        w_ob[i] = (unsigned)(n0 + row) * (unsigned)p.ktot * 2u + chunk;
    }

    f32x4v acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0f;

    RING_FEED_ITER(2)
    for (int s_ = 0; s_ < 3 && s_ < nk; ++s_) {
        R_DMA_A(0) R_DMA_B(0) R_DMA_A(1) R_DMA_B(1)
        RING_ADVANCE(2)
    }
    // fragment addressing: lane (r = lane&15, c = lane>>4) reads row R, chunk c ^ f(R); all tile rows keep (R>>2)&3 of r
    const int fr = (4 - (((lane & 15) >> 2) & 3)) & 3;
    const int coff = (((lane >> 4) ^ fr) << 4);
    const int a_row_off = (wm * 128 + (lane & 15)) * 64 + coff;
    const int b_row_off = (wn * 64 + (lane & 15)) * 64 + coff;
    bfrag8 a[8], bq[4];
    for (int ks = 0; ks < nk; ++ks) {
        if (ks + 2 < nk) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const bool refill = is_ks < nk;
        const unsigned char* sa = rsm + (ks & (R_NSTAGE - 1)) * R_STAGE_BYTES;
        const unsigned char* sb = sa + R_TILE_BYTES;
        if (ks == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bfrag8*>(sa + a_row_off + i * 16 * 64);
#pragma unroll
            for (int j = 0; j < 4; ++j) bq[j] = *reinterpret_cast<const bfrag8*>(sb + b_row_off + j * 16 * 64);
        }
        __builtin_amdgcn_sched_barrier(0);
        // first half: rows 0-63 of the wave's block; the second half's A fragments are fetched behind the first MFMAs
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = STATS ? mfma16x16x32(a[i], bq[j], acc[i][j]) : mfma16x16x32(bq[j], a[i], acc[i][j]);
            __builtin_amdgcn_sched_barrier(0);
            if (i == 0) {
#pragma unroll
                for (int i2 = 4; i2 < 8; ++i2) a[i2] = *reinterpret_cast<const bfrag8*>(sa + a_row_off + i2 * 16 * 64);
            }
            if (refill) {
                if (i == 1) R_DMA_A(0)
                if (i == 3) R_DMA_B(0)
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 4; i < 8; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = STATS ? mfma16x16x32(a[i], bq[j], acc[i][j]) : mfma16x16x32(bq[j], a[i], acc[i][j]);
            __builtin_amdgcn_sched_barrier(0);
            if (i == 4 && ks + 1 < nk) {
                // next stage (certified by this K-step's barrier): first-half A fragments; a[0..3] are no longer needed
                const unsigned char* san = rsm + ((ks + 1) & (R_NSTAGE - 1)) * R_STAGE_BYTES;
#pragma unroll
                for (int i2 = 0; i2 < 4; ++i2) a[i2] = *reinterpret_cast<const bfrag8*>(san + a_row_off + i2 * 16 * 64);
            }
            if (refill) {
                if (i == 5) R_DMA_A(1)
                if (i == 7) R_DMA_B(1)
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (ks + 1 < nk) {
            // B fragments of the next stage: all MFMAs of this stage have been issued
            const unsigned char* sbn = rsm + ((ks + 1) & (R_NSTAGE - 1)) * R_STAGE_BYTES + R_TILE_BYTES;
#pragma unroll
            for (int j = 0; j < 4; ++j) bq[j] = *reinterpret_cast<const bfrag8*>(sbn + b_row_off + j * 16 * 64);
        }
        if (is_ks < nk) RING_ADVANCE(2)
    }
    if (STATS) {
        ring_epilogue16<ACT, STATS>(acc, p, stats, rsm, b, t0, n0, out_len, wm, wn, wave, lane, epi16_load(p, n0, wn, lane));
    } else if (p.y_dtype == KTF_F32) {
        Epi16Cols cols;
        epi16_cols_load(cols, p, n0, wn, lane);
        ring_epilogue16_direct<ACT, true, false>(acc, p, cols, b, t0, n0, out_len, wm * 128, wn, lane);
    } else {
        __syncthreads();          // every wave's fragment reads are done before the ring is reused as staging
        // column constants were parked in LDS when the tile started (no global loads, and no latency, at this point)
        Epi16Cols cols;
        epi16_cols_lds<R_BN, true>(cols, prm, wn, lane);
        r16_stage_pk<ACT, true>(acc, cols, rsm, wm * 128, wn, lane);
        __syncthreads();
        r16_store_staged(p, rsm, reinterpret_cast<unsigned short*>(p.y), b, t0, n0, out_len, wave, lane);
    }
}

template <int ACT, bool STATS>
__global__ __launch_bounds__(512) void tdnn_bf16r16_kernel(TdnnParams p, int mtiles, int ntiles, int gtiles,
                                                           double* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rsm[];
    r16_tile<ACT, STATS>(p, mtiles, ntiles, gtiles, stats, rsm, blockIdx.x);
}

// ------------------------------------------------------------------------------------ BF16, 128x256 tile, 2 workgroups/CU
// The 256x256 kernel keeps one workgroup per CU, so its fixed per-tile phases (address setup, first-stage latency,
// epilogue: ~11 us against 16 us of K-loop at K = 512) leave the MFMA pipe idle. Here a workgroup is FOUR waves on a
// 128 x 256 tile (the same 128 x 64 block of 16x16x32 MFMAs per wave) with a 3-stage ring of 24 KiB stages: 76,800 B of
// LDS and <= 256 VGPRs let TWO workgroups share a CU, out of phase, so one's epilogue / prologue overlaps the other's
// K-loop and the two waves of a SIMD are no longer barrier-locked to each other.
//  * bias is preloaded into the accumulators, BatchNorm scale/shift sit in LDS (no global loads in the epilogue);
//  * non-reducing epilogue: operands swapped (W fragment as A) so a lane owns 4 consecutive columns -> packed bf16
//    ds_write_b64 staging, one barrier, 16-byte global stores (store issue is per instruction, T21);
//  * reducing (fused StatsPooling) epilogue: natural operand order, fp64 column sums, fp64 atomics.
#define H_BM 128
#define H_BN 256
#define H_NSTAGE 3
#define H_A_BYTES (H_BM * R_BK * 2)                  // 8 KiB
#define H_B_BYTES (H_BN * R_BK * 2)                  // 16 KiB
#define H_STAGE_BYTES (H_A_BYTES + H_B_BYTES)        // 24 KiB
#define H_RING_BYTES (H_NSTAGE * H_STAGE_BYTES)      // 72 KiB (bf16 staging of the tile: 128 x 520 B = 66,560 B)
#define H_LDS_BYTES (H_RING_BYTES + 3 * H_BN * 4)    // + bias | scale | shift of the tile's columns = 76,800 B


template <int ACT, bool STATS>
__global__ __launch_bounds__(256, 2) void tdnn_bf16h_kernel(TdnnParams p, int mtiles, int ntiles, int gtiles,
                                                            double* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rsm[];
    TDNN_TILE_HEADER(H_BM, H_BN, blockIdx.x)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave = wn;                              // one row of four waves
    const int c = lane & 15, g4 = lane >> 4;

    float* prm = reinterpret_cast<float*>(rsm + H_RING_BYTES);
    COL_PRM_PARK(prm, H_BN)

    RING_FEED_BASES(2)

    // LDS-DMA chunk q = i*256 + tid -> tile row q/4, LDS position q%4, global chunk (q%4) ^ f(row) (f as in the r16 kernel)
    int a_t[2];
    unsigned a_cb[2], w_ob[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = i * 256 + tid;
        const int row = q >> 2;
        const unsigned chunk = (unsigned)(((q & 3) ^ ((4 - ((row >> 2) & 3)) & 3)) * 16);
        if (i < 2) {
            a_cb[i] = chunk;
            a_t[i] = start + (t0 + row) * p.sub;
        }
        w_ob[i] = (unsigned)(n0 + row) * (unsigned)p.ktot * 2u + chunk;
    }

    RING_FEED_ITER(2)
    // three stages of A | W: a wrap counter names the slot; two pieces of A and four of W per thread
    int is_slot = 0;
#define H_DMA_A(i) RING_DMA_A(i, is_slot, H_STAGE_BYTES, 4096)
#define H_DMA_B(i) RING_DMA_W(i, wb, is_slot, H_STAGE_BYTES, H_A_BYTES, 4096)
#define H_ADVANCE()                                                                                                    \
    {                                                                                                                  \
        is_slot = (is_slot == H_NSTAGE - 1) ? 0 : is_slot + 1;                                                         \
        RING_ADVANCE(2)                                                                                                \
    }
    for (int s_ = 0; s_ < 2 && s_ < nk; ++s_) {
        H_DMA_A(0) H_DMA_A(1) H_DMA_B(0) H_DMA_B(1) H_DMA_B(2) H_DMA_B(3)
        H_ADVANCE()
    }
    __syncthreads();                                  // prm[] visible

    f32x4v acc[8][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f32x4v bj;
        if (STATS) {
            const float bv = prm[wn * 64 + j * 16 + c];
            bj[0] = bv; bj[1] = bv; bj[2] = bv; bj[3] = bv;
        } else {
            bj = *reinterpret_cast<const f32x4v*>(prm + wn * 64 + j * 16 + g4 * 4);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i][j] = bj;
    }

    const int fr = (4 - ((c >> 2) & 3)) & 3;
    const int coff = ((g4 ^ fr) << 4);
    const int a_row_off = c * 64 + coff;
    const int b_row_off = (wn * 64 + c) * 64 + coff;
    bfrag8 a[8], bq[4];
    int cs = 0;
    for (int ks = 0; ks < nk; ++ks) {
        if (ks + 1 < nk) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const bool refill = is_ks < nk;
        const unsigned char* sa = rsm + cs * H_STAGE_BYTES;
        const unsigned char* sb = sa + H_A_BYTES;
        cs = (cs == H_NSTAGE - 1) ? 0 : cs + 1;
        {
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const bfrag8*>(sa + a_row_off + i * 16 * 64);
#pragma unroll
            for (int j = 0; j < 4; ++j) bq[j] = *reinterpret_cast<const bfrag8*>(sb + b_row_off + j * 16 * 64);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = STATS ? mfma16x16x32(a[i], bq[j], acc[i][j]) : mfma16x16x32(bq[j], a[i], acc[i][j]);
            __builtin_amdgcn_sched_barrier(0);
            if (i == 0) {
#pragma unroll
                for (int i2 = 4; i2 < 8; ++i2) a[i2] = *reinterpret_cast<const bfrag8*>(sa + a_row_off + i2 * 16 * 64);
            }
            if (refill) {
                if (i == 1) H_DMA_A(0)
                if (i == 2) H_DMA_A(1)
                if (i == 3) H_DMA_B(0)
                if (i == 4) H_DMA_B(1)
                if (i == 5) H_DMA_B(2)
                if (i == 6) H_DMA_B(3)
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (refill) H_ADVANCE()
    }
    const int rows_valid = out_len - t0;
    if (STATS) {
        // natural layout: acc[i][j][r] = out[row i*16 + g4*4 + r][col wn*64 + j*16 + c]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nl = wn * 64 + j * 16 + c;
            const float scj = prm[H_BN + nl], shj = prm[2 * H_BN + nl];
            const PooledSums t = pooled_sums16<8, true>(lane, rows_valid, [&](int i, int r) { return EPI_VALUE_NB(ACT, acc[i][j][r], scj, shj); });
            const int n = n0 + nl;
            if (lane < 16 && n < p.units) stats_out(stats, p, b, pool_block128().slot_of(t0), n, t.s, t.q);
        }
        return;
    }
    // swapped layout: acc[i][j][e] = out[row i*16 + c][col wn*64 + j*16 + g4*4 + e]
    Epi16Cols cols;
    epi16_cols_lds<H_BN, false>(cols, prm, wn, lane);
    if (p.y_dtype == KTF_F32) {
        ring_epilogue16_direct<ACT, false, true>(acc, p, cols, b, t0, n0, out_len, 0, wn, lane);
        return;
    }
    __syncthreads();                                  // all fragment reads done: the ring becomes the staging buffer
    r16_stage_pk<ACT, false>(acc, cols, rsm, 0, wn, lane);
    __syncthreads();
    r16_store_staged(p, rsm, reinterpret_cast<unsigned short*>(p.y), b, t0, n0, out_len, wn, lane);
}


// ------------------------------------------------------------------------------------ launcher
int tdnn_launch_16(const TdnnParams& p, const KtfTdnnDesc* d, int64_t B, int64_t Tout, int64_t ldy, double* stats_sums, hipStream_t st) {
    KTF_REQUIRE(d->w_dtype == KTF_BF16, "ktf_tdnn: bf16 gemm needs bf16 weights");
    const bool k64 = (d->din_pad % 64) == 0;             // K-step: 64 when the per-context width allows it, else 32
    // the 128x128 kernel; its two names per operand form are the ones ktf_tdnn_last_kernel() reports
    auto plain = [&](auto XF, auto X3, const char* name64, const char* name32) {
        const dim3 grid((unsigned)ktf_cdiv(d->units, 128), (unsigned)ktf_cdiv(Tout, BF_BM), (unsigned)B);
        tdnn_pick<64, 32>(k64 ? 64 : 32, [&](auto BK) {
            constexpr int lds = 2 * 128 * BfCfg<BK>::PITCH * 2 * (X3 ? 2 : 1) * sizeof(unsigned short);
            tdnn_launch_kernel<tdnn_bf16_kernel<BK, XF, X3>>(BK == 64 ? name64 : name32, grid, dim3(256), lds, lds > 64 * 1024 ? lds : 0, st, p);
        });
    };
    if (d->gemm == KTF_GEMM_BF16X3) {
        plain(std::true_type{}, std::true_type{}, "tdnn_bf16_kernel<64, true, true>", "tdnn_bf16_kernel<32, true, true>");
    } else if (d->x_dtype == KTF_F32) {
        plain(std::true_type{}, std::false_type{}, "tdnn_bf16_kernel<64, true, false>", "tdnn_bf16_kernel<32, true, false>");
    } else {
        KTF_REQUIRE(d->x_dtype == KTF_BF16, "ktf_tdnn: bad x_dtype");
        if (d->units > 128 && ldy % 4 == 0) {
            // W must be padded to a multiple of 256 rows for this kernel (documented in ktf_hip.h)
            const int mtiles = ktf_cdiv(Tout, R_BM), ntiles_r = ktf_cdiv(d->units, R_BN);
            const int64_t gtiles = B * (int64_t)mtiles;
            const int64_t nblocks = grouped_blocks(gtiles, ntiles_r);
            KTF_REQUIRE(nblocks < (1ll << 31), "ktf_tdnn: grid too large");
            // 128x256 tiles with two workgroups per CU win while the fixed per-tile phases are comparable to the K-loop
            // (K <= 768); deeper K amortises them and the 256x256 tile moves fewer bytes per flop
            const bool htile = p.ktot <= 768;
            if (htile && (d->act == KTF_ACT_RELU || d->act == KTF_ACT_NONE)) {
                const int mt_h = ktf_cdiv(Tout, H_BM);
                const int64_t gt_h = B * (int64_t)mt_h;
                const int64_t nb_h = grouped_blocks(gt_h, ntiles_r);
                KTF_REQUIRE(nb_h < (1ll << 31), "ktf_tdnn: grid too large");
                tdnn_pick<KTF_ACT_RELU, KTF_ACT_NONE>(d->act, [&](auto A) {
                    tdnn_pick<true, false>(stats_sums != nullptr, [&](auto ST) {
                        tdnn_launch_kernel<tdnn_bf16h_kernel<A, ST>>("tdnn_bf16h_kernel", dim3((unsigned)nb_h), dim3(256), H_LDS_BYTES, H_LDS_BYTES,
                                                                      st, p, mt_h, ntiles_r, (int)gt_h, stats_sums);
                    });
                });
            } else if (d->act == KTF_ACT_RELU || d->act == KTF_ACT_NONE) {      // 16x16x32 MFMAs; sigmoid / tanh stay on the 32x32x16 kernel
                TDNN_REQUIRE_Y_ALIGNED(p, stats_sums != nullptr || p.y_dtype != KTF_F32)      // (bf16 rows: r16_store_staged tests)
                tdnn_pick<KTF_ACT_RELU, KTF_ACT_NONE>(d->act, [&](auto A) {
                    tdnn_pick<true, false>(stats_sums != nullptr, [&](auto ST) {
                        tdnn_launch_kernel<tdnn_bf16r16_kernel<A, ST>>("tdnn_bf16r16_kernel", dim3((unsigned)nblocks), dim3(512), R16_LDS_BYTES,
                                                                        R16_LDS_BYTES, st, p, mtiles, ntiles_r, (int)gtiles, stats_sums);
                    });
                });
            } else {
                TDNN_REQUIRE_Y_ALIGNED(p, stats_sums != nullptr)
                tdnn_pick<KTF_ACT_SIGMOID, KTF_ACT_TANH>(d->act, [&](auto A) {
                    tdnn_pick<true, false>(stats_sums != nullptr, [&](auto ST) {
                        tdnn_launch_kernel<tdnn_bf16r_kernel<A, ST>>("tdnn_bf16r_kernel", dim3((unsigned)nblocks), dim3(512), R_LDS_BYTES, R_LDS_BYTES,
                                                                      st, p, mtiles, ntiles_r, (int)gtiles, stats_sums);
                    });
                });
            }
        } else if (k64 && ldy % 4 == 0) {
            const int mtiles = ktf_cdiv(Tout, G_BM), ntiles_g = ktf_cdiv(d->units, G_BN);
            const int64_t gtiles = B * (int64_t)mtiles;
            const int64_t nblocks = grouped_blocks(gtiles, ntiles_g);
            KTF_REQUIRE(nblocks < (1ll << 31), "ktf_tdnn: grid too large");
            TDNN_REQUIRE_Y_ALIGNED(p, false)
            tdnn_launch_kernel<tdnn_bf16g_kernel>("tdnn_bf16g_kernel", dim3((unsigned)nblocks), dim3(256), G_LDS_BYTES, G_LDS_BYTES, st, p, mtiles,
                                                  ntiles_g, (int)gtiles);
        } else {
            plain(std::false_type{}, std::false_type{}, "tdnn_bf16_kernel<64, false, false>", "tdnn_bf16_kernel<32, false, false>");
        }
    }
    KTF_CHECK_LAUNCH("ktf_tdnn");
    return KTF_OK;
}
