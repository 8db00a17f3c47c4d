// The 64-row small-tile kernels (tdnn_f32s_kernel in tdnn_f32.hip, tdnn_x4s_kernel in tdnn_pair.hip: a bf16-pair row IS an fp32 row to
// the DMA): their constants, the 4-stage LDS-DMA ring of 64 x BK activation rows and BN x BK weight rows (four bytes per element), the
// K-loop with its counted waits, the row-store epilogue and the launcher's choice of the instantiation. A kernel brings its operand
// format as a `Frag` (below): the accumulators, the fragment read and the MFMA step of one position of a K-step.
#pragma once
#include "tdnn_common.h"

typedef __attribute__((ext_vector_type(4))) float f32x4v;

#define FS_BM 64
#define FS_NSTAGE 4
// s_waitcnt with vmcnt = v, expcnt / lgkmcnt left at their maxima (also tdnn_f32_rowvec_kernel's)
#define FS_VM(v_) (((v_) & 15) | (((v_) >> 4) << 14) | 0x0f70)

// <BK, BN, NB>: K-step, tile width, 16-column blocks per wave (they share the A fragment)
template <int BK, int BN, int NB>
struct SmallTile {
    static_assert(BN % (16 * NB) == 0, "a wave owns NB 16-column blocks");
    static constexpr int WN = BN / 16 / NB;                         // waves across the tile's columns, NB blocks each (one A fragment
    static constexpr int NT = 64 * 4 * WN;                          // feeds NB MFMAs); 1024 / 512 threads
    static constexpr int CH = BK / 4;                               // 16-byte chunks per row
    static constexpr int ROWB = BK * 4;                             // bytes per staged row
    static constexpr int A_BYTES = FS_BM * ROWB, W_BYTES = BN * ROWB;
    static constexpr int TILE_BYTES = A_BYTES;                      // offset of the W tile inside a stage
    static constexpr int STAGE_BYTES = A_BYTES + W_BYTES;
    static constexpr int LDS_BYTES = FS_NSTAGE * STAGE_BYTES;
    static constexpr bool HALVES = (FS_BM * CH + BN * CH == NT);    // <32,64>: threads 0-511 stage A, 512-1023 stage W
    static constexpr int NA = HALVES ? 1 : (FS_BM * CH) / NT;       // DMAs per thread and stage into the A tile
    static constexpr int NW = HALVES ? 0 : (BN * CH) / NT;          // ... and into the W tile
    static constexpr int NDMA = HALVES ? 1 : NA + NW;
    static_assert(HALVES || ((FS_BM * CH) % NT == 0 && (BN * CH) % NT == 0), "staging does not divide");
    static_assert(3 * NDMA <= 63, "vmcnt range");
};

// The whole K-loop of a tile: fills the ring, then runs the nk = ktot / BK steps. Frag (a struct of the kernel's translation unit):
//   init(wm, wn, lane) zeroes the accumulators and sets the lane's fragment offsets (called once the ring's first DMAs are issued)
//   POS               positions per K-step (a position = the fragments one MFMA step consumes)
//   read(c, stage)    the lane's fragments of position c from the stage at `stage` into the registers of position c
//   mfma(c)           the MFMA(s) of position c on those registers
// (wave: through readfirstlane.)
template <int BK, int BN, int NB, typename Frag>
__device__ __forceinline__ void small_tile_kloop(const TdnnParams& p, unsigned char* fsm, int b, int len, int start, int t0, int n0, int tid,
                                                 int wave, int wm, int wn, int lane, Frag& f) {
    using S = SmallTile<BK, BN, NB>;
    constexpr int NT = S::NT, CH = S::CH, ROWB = S::ROWB, TILE_BYTES = S::TILE_BYTES, STAGE_BYTES = S::STAGE_BYTES;
    constexpr bool HALVES = S::HALVES;
    constexpr int NA = S::NA, NW = S::NW, NDMA = S::NDMA, POS = Frag::POS;
    // staging: chunk q of a tile -> row q / CH, LDS position q % CH holds global chunk (q % CH) ^ (row & (CH-1)); a DMA
    // instruction of the workgroup covers NT consecutive chunks
    const bool isw = HALVES && tid >= NT / 2;
    constexpr int NAq = NA > 0 ? NA : 1, NWq = NW > 0 ? NW : 1;
    int a_t[NAq];
    unsigned a_cb[NAq], w_ob[NWq];
#pragma unroll
    for (int i = 0; i < NAq; ++i) {
        const int q = HALVES ? (tid & (NT / 2 - 1)) : i * NT + tid;
        const int row = q / CH;
        a_cb[i] = (unsigned)(((q % CH) ^ (row & (CH - 1))) * 16);
        a_t[i] = start + (t0 + row) * p.sub;
    }
#pragma unroll
    for (int i = 0; i < NWq; ++i) {
        const int q = HALVES ? (tid & (NT / 2 - 1)) : i * NT + tid;
        const int row = q / CH;
        w_ob[i] = (unsigned)(n0 + row) * (unsigned)p.ktot * 4u + (unsigned)(((q % CH) ^ (row & (CH - 1))) * 16);
    }
    const char* xb = reinterpret_cast<const char*>(p.x) + ((int64_t)b * p.T * p.ldx) * 4;
    const char* wb = reinterpret_cast<const char*>(p.w);
    const unsigned ldxb = (unsigned)p.ldx * 4u;
    const int nk = p.ktot / BK;
    const int lenm1 = len - 1;
    int is_ks = 0, is_c = 0, is_db = 0, is_off = p.ctx[0];
    const int dpad_b = p.din_pad * 4;
    // A stage is fetched in three pieces so that its DMAs can be spread over a K-step: FS_SRC (source offsets of stage
    // is_ks into soff[], LDS destination st_d), FS_ADV (scalar cursor to the next stage; holds the only scalar load, of a
    // context offset), FS_DMA(i) (the i-th 16-byte-per-lane DMA of the stage).
    // (Macros: they share the cursor and soff[] and FS_DMA's argument selects its branch at compile time.)
    unsigned soff[NDMA];
    unsigned char* st_d;
#define FS_SRC()                                                                                                       \
    {                                                                                                                  \
        st_d = fsm + (is_ks & (FS_NSTAGE - 1)) * STAGE_BYTES + wave * 1024;                                            \
        if (HALVES) {                                        /* waves 8-15 land in the W tile: wave * 1024 >= A_BYTES */ \
            int r_ = a_t[0] + is_off;                                                                                  \
            r_ = r_ < 0 ? 0 : (r_ > lenm1 ? lenm1 : r_);                                                               \
            soff[0] = isw ? w_ob[0] + (unsigned)(is_ks * ROWB) : (unsigned)r_ * ldxb + a_cb[0] + (unsigned)is_db;      \
        } else {                                                                                                       \
            _Pragma("unroll") for (int i = 0; i < NA; ++i) {                                                           \
                int r_ = a_t[i] + is_off;                                                                              \
                r_ = r_ < 0 ? 0 : (r_ > lenm1 ? lenm1 : r_);                                                           \
                soff[i] = (unsigned)r_ * ldxb + a_cb[i] + (unsigned)is_db;                                             \
            }                                                                                                          \
            _Pragma("unroll") for (int i = 0; i < NW; ++i) soff[NA + i] = w_ob[i] + (unsigned)(is_ks * ROWB);          \
        }                                                                                                              \
    }
#define FS_DMA(i_)                                                                                                     \
    {                                                                                                                  \
        if (HALVES)                                                                                                    \
            __builtin_amdgcn_global_load_lds((glb_ptr_t*)((isw ? wb : xb) + soff[0]), (lds_ptr_t*)st_d, 16, 0, 0);     \
        else if ((i_) < NA)                                                                                            \
            __builtin_amdgcn_global_load_lds((glb_ptr_t*)(xb + soff[i_]), (lds_ptr_t*)(st_d + (i_) * (NT * 16)), 16, 0, 0); \
        else                                                                                                           \
            __builtin_amdgcn_global_load_lds((glb_ptr_t*)(wb + soff[i_]),                                              \
                                             (lds_ptr_t*)(st_d + TILE_BYTES + ((i_) - NA) * (NT * 16)), 16, 0, 0);     \
    }
#define FS_ADV()                                                                                                       \
    {                                                                                                                  \
        ++is_ks;                                                                                                       \
        is_db += ROWB;                                                                                                 \
        if (is_db == dpad_b) {                                                                                         \
            is_db = 0;                                                                                                 \
            ++is_c;                                                                                                    \
            is_off = (is_c < p.nctx) ? p.ctx[is_c] : 0;                                                                \
        }                                                                                                              \
    }
    for (int s_ = 0; s_ < FS_NSTAGE && s_ < nk; ++s_) {
        FS_SRC()
#pragma unroll
        for (int i = 0; i < NDMA; ++i) FS_DMA(i)
        FS_ADV()
    }
    f.init(wm, wn, lane);
    // wait until at most `n_` (0..3) of this wave's stages are still in flight (NDMA DMAs each)
#define FS_WAIT(n_)                                                                                                    \
    {                                                                                                                  \
        const int n__ = (n_);                                                                                          \
        if (n__ >= 3) __builtin_amdgcn_s_waitcnt(FS_VM(3 * NDMA));                                                     \
        else if (n__ == 2) __builtin_amdgcn_s_waitcnt(FS_VM(2 * NDMA));                                                \
        else if (n__ == 1) __builtin_amdgcn_s_waitcnt(FS_VM(NDMA));                                                    \
        else __builtin_amdgcn_s_waitcnt(FS_VM(0));                                                                     \
    }
    // The fragments of step ks + 1 are read under the MFMAs of step ks (one workgroup per CU, both waves of a SIMD in the
    // same phase: read latency in front of the MFMAs was 40 % of the step). A stage is refilled four steps ahead, into
    // the slot whose fragments every wave took during the previous step.
    {
        const int issued = nk < FS_NSTAGE ? nk : FS_NSTAGE;
        FS_WAIT(issued - 1)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#pragma unroll
        for (int c = 0; c < POS; ++c) f.read(c, fsm);
        __builtin_amdgcn_s_waitcnt(0xc07f);                  // lgkmcnt(0), as an instruction the compiler's counter model sees
    }                                                        // (an inline-asm wait is not: fragments "pending" at the loop head
                                                             // put a wait for the reads just issued in front of every MFMA)
    for (int ks = 0; ks + 1 < nk; ++ks) {
        const int beyond = nk - 2 - ks;                      // stages issued beyond ks + 1: min(beyond, 2)
        FS_WAIT(beyond < 2 ? beyond : 2)
        __builtin_amdgcn_s_barrier();                         // every wave has taken stage ks (its reads were waited for at the
        asm volatile("" ::: "memory");                       // end of the previous step): the slot can be refilled
        const bool refill = is_ks < nk;
        if (refill) {
            FS_SRC()
            FS_ADV()
        }
        // One position of the K-step at a time: its MFMA(s), then the fragment reads of the same position of the next stage
        // into the registers those MFMAs just consumed, and the DMAs of the refill spread evenly over the positions (DMA i
        // behind position i * POS / NDMA). Bursts keep all
        // waves in LDS issue (at most 15 LDS operations of a wave are in flight) or in the texture addresser's queue while
        // the matrix pipes idle. In-kernel stamps (tdnn_f32s_kernel, K = 1536, 64 x 32 tiles, tools/b1_tile_probe.py with
        // -DKTF_FS_ABL): K-loop 22.7 us; MFMAs + barrier alone 13.8, fragment reads + barrier alone 13.9 (256 ds_read_b32 per
        // step and workgroup at ~4.8 cycles each), DMA stream alone 9.4: the LDS instruction rate and the MFMAs are both near
        // their limits.
        const unsigned char* nst = fsm + ((ks + 1) & (FS_NSTAGE - 1)) * STAGE_BYTES;
#pragma unroll
        for (int c = 0; c < POS; ++c) {
            f.mfma(c);
#pragma unroll
            for (int i = 0; i < NDMA; ++i)
                if ((i * POS) / NDMA == c) {
                    if (refill) FS_DMA(i)
                }
            f.read(c, nst);
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
    }
#pragma unroll
    for (int c = 0; c < POS; ++c) f.mfma(c);
#undef FS_WAIT
#undef FS_SRC
#undef FS_DMA
#undef FS_ADV
}

// The row epilogue: 16x16 accumulator layout, f.value(j, r) = out[row 4 * (lane >> 4) + r of the wave's 16][column lane & 15 of block j].
// BF16_ROWS: the rows may be bf16 (tdnn_f32s_kernel); tdnn_x4s_kernel writes fp32-sized slots only.
template <int BN, int NB, bool BF16_ROWS, typename Frag>
__device__ __forceinline__ void small_tile_store(const TdnnParams& p, const Frag& f, int b, int t0, int n0, int out_len, int wm, int wn, int lane) {
    const int r16 = lane & 15, kq = lane >> 4;
    const int rows_valid = out_len - t0;
    const int64_t out_row0 = (int64_t)b * p.Tout + t0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int n = n0 + (wn * NB + j) * 16 + r16;
        if (n >= p.units) continue;
        const float bias = p.bias ? p.bias[n] : 0.0f;
        const float sc = p.scale ? p.scale[n] : 1.0f;
        const float sh = p.shift ? p.shift[n] : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = wm * 16 + kq * 4 + r;
            if (m < rows_valid) {
                const float v = TDNN_EPI_ROW(f.value(j, r), bias, sc, sh, p.act);
                const int64_t off = (out_row0 + m) * p.ldy + n;
                if (BF16_ROWS) TDNN_STORE_Y(off, v)
                else reinterpret_cast<float*>(p.y)[off] = v;
            }
        }
    }
}

// The launch of a small-tile family: K-step 64 where the per-context width allows it, with the tile width of small_tile_width, else
// <32, 64>. go(BK, BN, NB, i, grid, threads, lds) launches the family's instantiation i (0: <32, 64>; 1 .. 3: <64, 32 / 64 / 96>) with
// BK, BN, NB as integral constants.
template <typename Go>
static void small_tile_launch(const KtfTdnnDesc* d, int64_t B, int64_t Tout, Go&& go) {
    auto small = [&](auto BK, auto BN) {
        constexpr int NB = BN == 96 ? 3 : 1;
        using S = SmallTile<BK, BN, NB>;
        const dim3 grid((unsigned)ktf_cdiv(d->units, BN), (unsigned)ktf_cdiv(Tout, FS_BM), (unsigned)B);
        go(BK, BN, std::integral_constant<int, NB>{}, BK == 32 ? 0 : BN / 32, grid, dim3(S::NT), S::LDS_BYTES);
    };
    if (d->din_pad % 64 == 0)
        tdnn_pick<32, 64, 96>(small_tile_width(d->units, (int64_t)ktf_cdiv(Tout, FS_BM) * B),
                              [&](auto BN) { small(std::integral_constant<int, 64>{}, BN); });
    else
        small(std::integral_constant<int, 32>{}, std::integral_constant<int, 64>{});
}
