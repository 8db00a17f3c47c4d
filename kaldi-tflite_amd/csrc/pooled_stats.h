// The reducing StatsPooling fused into the wide TDNN kernels' epilogues (stats_pooling.py:231-240), every party of its contract once
// ("Fused pooling"): the WRITERS' fp64 partial sums (S, Q) = (sum v, sum v^2) of a column over the rows of a slot
// and their store, the SLOT RULE (which rows belong to which slot, how many slots an utterance gets and uses), and the READER that
// adds an utterance's used slots in order and forms mean | std.
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------ slot rule
// With KTF_TDNN_DET_STATS `sums` is (B, slots(T), 2, units): slot k of utterance b holds the rows of its k-th `slot_rows`-row block and
// has exactly one writer. Per-utterance tiles (tile_slots > 0) always write every slot of a tile, so the slots come in whole tiles
// and an utterance's blocks start at its row 0. Flat row tiles (tile_slots == 0) cut the blocks out of the flat row space (the batch's
// valid rows laid end to end), where an utterance starts at any row: T rows touch up to (T + 2 slot_rows - 2) / slot_rows blocks.
struct PoolSlots {
    int slot_rows, tile_slots;
    // slots per utterance of up to T rows
    __host__ __device__ constexpr int64_t slots(int64_t T) const {
        if (tile_slots == 0) return T <= 0 ? 1 : (T + 2 * slot_rows - 2) / slot_rows;
        const int64_t tile_rows = (int64_t)tile_slots * slot_rows;
        return T <= 0 ? tile_slots : tile_slots * ((T + tile_rows - 1) / tile_rows);
    }
    // the slot a writer fills: the block of its `row` (the tile's first row + the writer's row block) counted from the block of the
    // utterance's first row `first` (both >= 0; flat rows for flat row tiles, else rows of the utterance and first = 0)
    __host__ __device__ constexpr int slot_of(int row, int first = 0) const {
        return (int)((unsigned)row / (unsigned)slot_rows) - (int)((unsigned)first / (unsigned)slot_rows);
    }
    // the slots 0 .. used - 1 a reader adds for an utterance of len rows whose first row is `first`
    __host__ __device__ constexpr int used(int len, int first = 0) const { return len > 0 ? slot_of(first + len - 1, first) + 1 : 0; }
};
// the ring, split, bf16h and f16mx 256-row tiles: two 128-row wave blocks
__host__ __device__ constexpr PoolSlots pool_block128() { return {128, 2}; }
// the f16mx loader-wave kernel's 192-row tiles: two 96-row wave blocks
__host__ __device__ constexpr PoolSlots pool_block96() { return {96, 2}; }
// the pair kernel's 64-row tiles
__host__ __device__ constexpr PoolSlots pool_tile64() { return {64, 1}; }
// flat row tiles (split, f16mx): the 128-row blocks of the flat row space
__host__ __device__ constexpr PoolSlots pool_flat128() { return {128, 0}; }
// ... by what selects the kernel of a per-utterance launch: ktf_tdnn_stats' GEMM mode, ktf_tdnn_mx_stats' KtfTdnnDesc.flags
static inline PoolSlots pool_slots_tdnn(int32_t gemm) { return gemm == KTF_GEMM_BF16X4 ? pool_tile64() : pool_block128(); }
static inline PoolSlots pool_slots_mx(int32_t flags) { return (flags & KTF_TDNN_MX_LOADER) ? pool_block96() : pool_block128(); }

// ------------------------------------------------------------------------------------ writers
// Adds (stat_slots == 0) or stores (stat_slots > 0: `slot` of utterance b is written by exactly one wave) column n's partial sums.
// P: the kernel's parameter block (TdnnParams, MxParams); only its stat_slots and units are read.
template <typename P>
__device__ __forceinline__ void stats_out(double* __restrict__ stats, const P& p, int b, int slot, int n, double s, double q) {
    if (p.stat_slots > 0) {
        double* dst = stats + (((int64_t)b * p.stat_slots + slot) * 2) * p.units + n;
        dst[0] = s;
        dst[p.units] = q;
    } else {
        double* dst = stats + ((int64_t)b * 2) * p.units + n;
        atomicAdd(dst, s);
        atomicAdd(dst + p.units, q);
    }
}

struct PooledSums { double s, q; };

// A lane's fp32 sums relative to the pivot pv over its cnt rows of a column -> the column's fp64 sums over the rows of all four 16-lane
// groups (they hold the same column): sum v = s + n p, sum v^2 = q + 2 p s + n p^2.
__device__ __forceinline__ PooledSums pooled_sums_combine(float pv, float s32, float q32, int cnt) {
    const double pd = (double)pv, sd = (double)s32, nd = (double)cnt;
    double s = sd + nd * pd;
    double q = (double)q32 + 2.0 * pd * sd + nd * pd * pd;
    s += __shfl_xor(s, 16, 64); q += __shfl_xor(q, 16, 64);
    s += __shfl_xor(s, 32, 64); q += __shfl_xor(q, 32, 64);
    return {s, q};
}

// Sum and sum of squares of one column of a wave's block of NI 16 x 16 accumulator tiles (natural layout: the lane holds rows
// 16 i + 4 (lane >> 4) + r of column lane & 15) over the block's first `rv` rows (may be <= 0). `value(i, r)`: the FINISHED value
// (bias, activation, BatchNorm applied) of the lane's row (i, r). The sums are taken in fp32 RELATIVE TO A PIVOT (row 0 of the block, the
// same for the four lanes that share the column: a constant column -- a dead ReLU unit, a zero weight row -- gives exactly 0 and 0, not
// fp32 cancellation noise, hence var == 0 exactly as with fp64 accumulation) and only the per-lane results go to fp64: 3 fp32
// operations per row instead of 3 fp64 ones (the fp64 form was 4.3 us per tile, a fifth of a K = 512 tile's K-loop). The wave-uniform
// "full block" case carries no row predicate: FULL_LOOP gives it a loop of its own, else it is the first term of the predicate.
template <int NI, bool FULL_LOOP, typename ValueFn>
__device__ __forceinline__ PooledSums pooled_sums16(int lane, int rv, ValueFn value) {
    const float pv = __shfl(value(0, 0), lane & 15, 64);      // row 0 of the block lives in the (lane >> 4) == 0 lane of this column
    float s32 = 0.0f, q32 = 0.0f;
    int cnt = 0;
    if (FULL_LOOP && rv >= 16 * NI) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float u = value(i, r) - pv;
                s32 += u;
                q32 = fmaf(u, u, q32);
            }
        }
        cnt = 4 * NI;
    } else {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if ((!FULL_LOOP && rv >= 16 * NI) || i * 16 + (lane >> 4) * 4 + r < rv) {
                    const float u = value(i, r) - pv;
                    s32 += u;
                    q32 = fmaf(u, u, q32);
                    ++cnt;
                }
            }
        }
    }
    return pooled_sums_combine(pv, s32, q32, cnt);
}

// Flat row tiles (tdnn_split.hip, tdnn_mx.hip): a wave's 128-row block of a tile over the batch's valid rows laid end to end holds rows
// of several utterances, each a run of consecutive rows.
// acc[i][j][r]: the FINISHED value (activation, BatchNorm applied) of tile row 128 wm + 16 i + 4 (lane >> 4) + r, column 16 j + (lane & 15) of
// the wave's 64 columns. Per run (wave-uniform loop) the wave sums its columns over the run's rows -- in fp32 relative to the run's first
// row, so that a constant column sums to exactly (n v, n v^2) -- and hands the fp64 result to `out(b, slot, j, s, q)` on lanes 0..15,
// slot = pool_flat128()'s: every (utterance, slot) has one writer.
// `run_of(m)`: (frame t, utterance length, utterance b) of tile row m (wave-uniform m; valid rows only). R0: first flat row of the tile.
template <typename RunFn, typename OutFn>
__device__ __forceinline__ void flat_stats_runs(f32x4 (&acc)[8][4], int R0, int rows_valid, int wm, int lane, RunFn run_of, OutFn out) {
    const int g4 = lane >> 4;
    const int blk0 = wm * 128;
    const int blk_end = min(blk0 + 128, rows_valid);
    int m = blk0;
    while (m < blk_end) {
        int t_m, len_m, b;
        run_of(m, t_m, len_m, b);
        const int seg_end = min(blk_end, m + (len_m - t_m));
        const int lm = m - blk0, le = seg_end - blk0;                 // the run's rows inside the block: [lm, le)
        const int slot = pool_flat128().slot_of(R0 + blk0, R0 + m - t_m);
        const int rb = g4 * 4 - lm;                                    // lane's row (i, r) relative to the run's first: rb + 16 i + r
        const unsigned span = (unsigned)(le - lm);
        // (lm, le are the same on every lane: as scalars they steer wave-uniform branches)
        const int lmu = __builtin_amdgcn_readfirstlane(lm), leu = __builtin_amdgcn_readfirstlane(le);
        // the run's first row lmu = 16 i0 + 4 g + r0 of the block is held by the lanes of quarter g in acc[i0][.][r0]
        float pv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i == (lmu >> 4)) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j) pv[j] = r == (lmu & 3) ? acc[i][j][r] : pv[j];
            }
        const int src = ((lmu >> 2) & 3) * 16 + (lane & 15);          // the lane that holds the run's first row of this column
#pragma unroll
        for (int j = 0; j < 4; ++j) pv[j] = __shfl(pv[j], src, 64);
        float s32[4] = {0.0f, 0.0f, 0.0f, 0.0f}, q32[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int cnt = 0;
        // per 16-row group of the block (wave-uniform tests): outside the run -- nothing (its terms were + 0.0f: the sums are the same bits);
        // inside -- the plain sums, 12 vector instructions per row of four columns; across an end of the run -- per-row tests, 22 per row.
        // A 998-frame utterance: seven blocks in eight are one run over all eight groups.
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (16 * i + 16 <= lmu || 16 * i >= leu) continue;
            if (16 * i >= lmu && 16 * i + 16 <= leu) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float u = acc[i][j][r] - pv[j];
                        s32[j] += u;
                        q32[j] = fmaf(u, u, q32[j]);
                    }
                cnt += 4;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool in = (unsigned)(rb + 16 * i + r) < span;
                    cnt += in ? 1 : 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float u = in ? acc[i][j][r] - pv[j] : 0.0f;
                        s32[j] += u;
                        q32[j] = fmaf(u, u, q32[j]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const PooledSums t = pooled_sums_combine(pv[j], s32[j], q32[j], cnt);
            if (lane < 16) out(b, slot, j, t.s, t.q);
        }
        m = seg_end;
    }
}

// ------------------------------------------------------------------------------------ reader
// tf.nn.relu of the variance (stats_pooling.py:238, 293): a NaN -- the 0 / 0 of an utterance or a window without a frame, NaN
// activations -- stays a NaN (fmax would return 0 and the standard deviation sqrt(epsilon))
__device__ __forceinline__ double relu_keep_nan(double v) { return v < 0.0 ? 0.0 : v; }

struct PooledMoments { float mean, std; };

// mean and (include_std) standard deviation of column c of utterance b (n rows) from sums (B, max(slots, 1), 2, D): the first `used`
// slots added in slot order, or -- slots == 0 -- the one slot the fp64 atomics accumulated
__device__ __forceinline__ PooledMoments pooled_moments(const double* __restrict__ sums, int64_t slots, int used, int64_t b, int D, int c, double n,
                                                        int include_std, float eps) {
    double s = 0.0, q = 0.0;
    if (slots == 0) {
        s = sums[(b * 2) * D + c];
        q = sums[(b * 2 + 1) * D + c];
    } else {
        for (int k = 0; k < used; ++k) {
            s += sums[((b * slots + k) * 2) * D + c];
            q += sums[((b * slots + k) * 2 + 1) * D + c];
        }
    }
    const double mean = s / n;
    return {(float)mean, include_std ? (float)sqrt(relu_keep_nan(q / n - mean * mean) + (double)eps) : 0.0f};
}
