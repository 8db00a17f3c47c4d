// KTF_GEMM_BF16X4: fp32-grade products on the bf16 matrix pipe for FEW tiles (a single utterance, a handful of them): the small-tile
// K-loop of tdnn_f32s_kernel (tdnn_small_tile.h: ring, schedule, row epilogue, launcher) with operands in the PAIR format (KTF_BF16P): every fp32 slot of an activation
// row / weight row holds bf16(v) in its low half and bf16(v - bf16(v)) in its high half -- same shapes, strides and padding as
// fp32, 16 mantissa bits.
//
// A lane's 16-byte fragment read (one chunk of its row: 4 values) IS an operand of v_mfma_f32_16x16x32_bf16: 8 bf16 slots
// (h0 l0 h1 l1 h2 l2 h3 l3). With A and B read the same way, MFMA(A, B) sums h*g + l*m over the chunk and MFMA(A', B), A' = A
// with the halves of every dword swapped (one v_alignbit each), sums l*g + h*m: all four products of (h + l)(g + m), fp32
// accumulate, no de-interleave. Two MFMAs of 16 cycles per 16 values of K against four fp32 16x16x4 MFMAs of 32 cycles, and one
// ds_read_b128 where the fp32 kernel issues four ds_read_b32 -- the two things its K-loop is bound by (tdnn_f32.hip: MFMAs + barrier
// alone 13.8 us, fragment reads + barrier alone 13.9 us, DMA stream alone 9.4 us of 22.7 us at K = 1536). What is left is the DMA stream.
//
// Replaces: layers/tdnn/tdnn.py:251-280 (+ keras ReLU, batchnorm.py:78-88) for batches too small to fill the chip on 256-row tiles,
// in every mode but "f32" (Sequential.batch_gemm): the first layer runs the fp32 kernel and writes pairs, the last one in front of
// the pooling reads pairs and writes fp32.
#include "tdnn_small_tile.h"

typedef __attribute__((ext_vector_type(4))) unsigned u32x4v;
typedef __attribute__((ext_vector_type(8))) __bf16 bpair8;

// The pair operand format of the small tiles (tdnn_small_tile.h): G = CH / 4 positions per K-step, lane quarter kq takes chunk 4 g + kq
// of its row for position g; two accumulators per block -- the (A, B) and the (A', B) products -- so that consecutive MFMAs never
// depend on each other.
template <int BK, int BN, int NB>
struct PairFrag {
    using S = SmallTile<BK, BN, NB>;
    static constexpr int G = S::CH / 4, POS = G;
    f32x4v acc[NB][2];
    u32x4v av[G], bv[NB][G];
    int a_row_off, b_row_off, frag_off[G];
    __device__ __forceinline__ void init(int wm, int wn, int lane) {
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[j][h][r] = 0.0f;
        const int r16 = lane & 15, kq = lane >> 4;
        const int sw = r16 & (S::CH - 1);
        a_row_off = (wm * 16 + r16) * S::ROWB;
        b_row_off = S::TILE_BYTES + (wn * NB * 16 + r16) * S::ROWB;                 // block j: + j * 16 rows
#pragma unroll
        for (int g = 0; g < G; ++g) frag_off[g] = ((4 * g + kq) ^ sw) << 4;        // chunk 4 g + kq of the lane's row
    }
    __device__ __forceinline__ void read(int g, const unsigned char* st) {
        av[g] = *reinterpret_cast<const u32x4v*>(st + a_row_off + frag_off[g]);
#pragma unroll
        for (int j = 0; j < NB; ++j) bv[j][g] = *reinterpret_cast<const u32x4v*>(st + b_row_off + j * 16 * S::ROWB + frag_off[g]);
    }
    __device__ __forceinline__ void mfma(int g) {
        const u32x4v a_ = av[g];
        const u32x4v s_ = u32x4v{__builtin_amdgcn_alignbit(a_.x, a_.x, 16), __builtin_amdgcn_alignbit(a_.y, a_.y, 16),
                                 __builtin_amdgcn_alignbit(a_.z, a_.z, 16), __builtin_amdgcn_alignbit(a_.w, a_.w, 16)};
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const bpair8 b_ = __builtin_bit_cast(bpair8, bv[j][g]);
            acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bpair8, a_), b_, acc[j][0], 0, 0, 0);
            acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bpair8, s_), b_, acc[j][1], 0, 0, 0);
        }
    }
    __device__ __forceinline__ float value(int j, int r) const { return acc[j][0][r] + acc[j][1][r]; }
};

// STATS: fused StatsPooling (stats_pooling.py:231-240): the tile's fp64 column sums / sums of squares over its 64 rows go to `stats`
// (pool_tile64() slots with KTF_TDNN_DET_STATS, else atomics); the layer output is never written.
template <int BK, int BN, int NB, bool STATS>
__global__ __launch_bounds__(64 * 4 * (BN / 16 / NB)) void tdnn_x4s_kernel(TdnnParams p, double* __restrict__ stats) {
    constexpr int WN = SmallTile<BK, BN, NB>::WN, NT = SmallTile<BK, BN, NB>::NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
    TDNN_TILE3D_HEADER(FS_BM, BN)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    // the fragments of step ks + 1 are read under the MFMAs of step ks; a stage is refilled four steps ahead (tdnn_f32s_kernel's schedule)
    PairFrag<BK, BN, NB> f;
    small_tile_kloop<BK, BN, NB>(p, fsm, b, len, start, t0, n0, tid, wave, wm, wn, lane, f);
    // 16x16 accumulator layout: acc[r] = out[row 4*(lane>>4) + r][col lane&15]
    if constexpr (STATS) {
        const int r16 = lane & 15, kq = lane >> 4;
        const int rows_valid = out_len - t0;
        // per column: the lane's four rows in fp64, the four lane quarters by two shuffles, the four row waves through LDS (the ring
        // is free: every wave's last fragment reads were waited for), one store / atomic pair per column
        double* red = reinterpret_cast<double*>(fsm);                    // [wm][2][BN]
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int cl = (wn * NB + j) * 16 + r16;
            const int n = n0 + cl;
            const bool nv = n < p.units;
            const float bias = (nv && p.bias) ? p.bias[n] : 0.0f;
            const float sc = (nv && p.scale) ? p.scale[n] : 1.0f;
            const float sh = (nv && p.shift) ? p.shift[n] : 0.0f;
            double s = 0.0, q = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = wm * 16 + kq * 4 + r;
                const float v = TDNN_EPI_VALUE(f.value(j, r), bias, sc, sh, p.act);
                if (m < rows_valid) {
                    s += (double)v;
                    q += (double)v * (double)v;
                }
            }
            s += __shfl_xor(s, 16, 64);
            q += __shfl_xor(q, 16, 64);
            s += __shfl_xor(s, 32, 64);
            q += __shfl_xor(q, 32, 64);
            if (kq == 0) {
                red[(wm * 2 + 0) * BN + cl] = s;
                red[(wm * 2 + 1) * BN + cl] = q;
            }
        }
        __syncthreads();
        for (int cl = tid; cl < BN; cl += NT) {
            const int n = n0 + cl;
            if (n < p.units) {
                double s = 0.0, q = 0.0;
#pragma unroll
                for (int w_ = 0; w_ < 4; ++w_) {
                    s += red[(w_ * 2 + 0) * BN + cl];
                    q += red[(w_ * 2 + 1) * BN + cl];
                }
                stats_out(stats, p, b, pool_tile64().slot_of(t0), n, s, q);
            }
        }
        return;
    }
    small_tile_store<BN, NB, false>(p, f, b, t0, n0, out_len, wm, wn, lane);
}

int tdnn_launch_x4(const TdnnParams& p, const KtfTdnnDesc* d, int64_t B, int64_t Tout, double* stats, hipStream_t st) {
    // tile width as for the fp32 small tiles (tdnn_launch_f32; the host pads W's rows to 128 here)
    static const char* const names[] = {"tdnn_x4s_kernel<32, 64>", "tdnn_x4s_kernel<64, 32>", "tdnn_x4s_kernel<64, 64>", "tdnn_x4s_kernel<64, 96>"};
    small_tile_launch(d, B, Tout, [&](auto BK, auto BN, auto NB, int i, dim3 grid, dim3 block, int lds) {
        tdnn_pick<true, false>(stats != nullptr, [&](auto STATS) {
            tdnn_launch_kernel<tdnn_x4s_kernel<BK, BN, NB, STATS>>(names[i], grid, block, lds, lds, st, p, stats);
        });
    });
    KTF_CHECK_LAUNCH("ktf_tdnn");
    return KTF_OK;
}
