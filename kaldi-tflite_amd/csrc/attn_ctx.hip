// Global-context attention logits for attentive statistics pooling (include/ktf_gctx.h states the contract as numbered rules,
// INTEGRATION.md section 2v the use, DESIGN.md section 7 the design and the measurements). Three launches:
//
//   ktf_gctx_stats    gctx_stats_kernel     one workgroup = one utterance x 64 channels: mu and sigma in fp64, the canonical order (rules 2, 3)
//   ktf_gctx_bias     gctx_bias_kernel      one wave = 16 utterances x 16 units: g = b1 + [mu ; sigma] W1c on fp64 MFMA (rule 5)
//   ktf_gctx_logits   gctx_logits_kernel    one workgroup = 64 rows of one utterance: e = W2^T act(W1x^T x + g) + b2 (rules 6 - 9)
//
// The logits kernel. A workgroup of four waves owns GC_R = 64 rows [t0, t0 + 64) of one utterance, t0 a multiple of 64, and ALL A <= 256
// hidden units of them: the bias g_b is then one vector per workgroup, and nothing an utterance computes depends on its neighbours in
// the batch. A wave owns a quadrant of 32 rows x 128 columns, sixteen 16 x 16 accumulators (2 row blocks x 8 column blocks) held in
// registers; NCB, the column blocks a wave really has in phase 1, is 2, 4 or 8 for A <= 64, 128, 256. A tile at or beyond len_b exits at once.
//
// One flat loop of nk1 + nb2 nk2 steps, nk1 = ceil(D / 32), nk2 = ceil(A / 32), nb2 = ceil(H / 256), fed one step ahead through a ring of
// two stages, one barrier per step (it says both "step s has landed" and "everyone has finished reading the stage step s + 1 goes into"):
//   phase 1, step k < nk1: the stage holds x[64 rows][32 k] and W1x[32 k][256 units]; 2 x NCB blocks take chunk k. The epilogue of the
//     last step adds g_b, applies act and writes h (units >= A as +0) into the LDS tile -- h never reaches global memory.
//   phase 2, step (block j, chunk k): the stage holds W2[32 k][256 heads of block j]; the left operand is read from the h tile. The
//     epilogue of a block's last chunk adds b2 and stores the 64 x 256 block of e, rows below len_b and heads below H only.
// x is read from global memory once, by the one workgroup that owns its rows; W1x and W2 come from L2.
//
// LDS, 149504 of the 163840 bytes of a gfx950 workgroup (one workgroup per compute unit: the kernel lives on matrix instructions, not on
// occupancy):
//   stage = x image 64 rows x 128 bytes = 8192, W image 32 rows x 1040 bytes = 33280            2 x 41472 =  82944
//   h tile 64 rows x 260 floats                                                                            66560
// x image: as in agg_conv.hip, LDS piece p (16 bytes) of row r holds global piece p ^ ((r >> 1) & 7), so the sixteen rows of a fragment
// read fall on disjoint banks although the DMA image cannot be padded. W image: one k-row of 256 floats is exactly one wave-wide DMA (64
// lanes x 16 bytes), so every row has a destination of its own and IS padded, to 260 floats: a fragment read takes W[8 i + s][col + n] for
// the lane groups i = 0 .. 3, whose rows lie 8 x 260 floats = 32 banks apart. The h tile has the same stride of 260 floats: a 16-byte
// fragment read of sixteen consecutive rows covers all 64 banks once.
//
// Feed. 16 bytes per lane by global_load_lds DMA, no VGPR round trip: two DMAs for x and eight for W per lane and step. The DMA needs
// a 16-byte aligned base, a leading dimension that is a multiple of 4 and (W) a width that is one, and is used for full chunks only; any
// other operand, and the last chunk when D or A is no multiple of 32, goes by guarded scalar loads (columns and k beyond the operand
// read as +0) and one LDS store into the same image. The choice is wave-uniform; the bits are the same (rule 9). Rows are clamped to
// len_b - 1 where they are READ, DMA pieces beyond the width to the last whole piece; what such rows and columns compute is never stored.
//
// Matrix instructions. The rows are the first operand (M), the weights the second (N): lane (n = lane & 15, i = lane >> 4) of block
// (rb, cb) holds rows 16 rb + 4 i + 0 .. 3 of column 16 cb + n, so a store instruction writes four runs of 64 contiguous bytes. Lane
// group i supplies the reduction elements 8 i .. 8 i + 7 of a chunk of either operand in both modes: F32 feeds them to eight
// v_mfma_f32_16x16x4_f32, BF16X3 splits them in registers (r2_split8) into three v_mfma_f32_16x16x32_bf16.
#include "res2_common.h"
#include "canon_sum.h"
#include "f64_mfma.h"
#include "../../include/ktf_gctx.h"

// every operation is rounded on its own: no contraction into fma, in any kernel of this file
#pragma clang fp contract(off)

#define GC_THREADS 256
#define GC_R 64
#define GC_NT 256                                 // columns of a W image: hidden units (phase 1), heads of a block (phase 2)
#define GC_XBYTES 8192                            // 64 rows of 128 bytes
#define GC_WS 260                                 // floats per row of the W image and of the h tile
#define GC_WROW (GC_WS * 4)
#define GC_STAGE_BYTES (GC_XBYTES + 32 * GC_WROW)
#define GC_H_BYTES (GC_R * GC_WS * 4)
#define GC_LDS_BYTES (2 * GC_STAGE_BYTES + GC_H_BYTES)
#define GC_ST_THREADS 1024
#define GC_B_THREADS 256
#define GC_B_KC 128                               // elements of [mu ; sigma] staged in LDS at a time

static_assert(GC_LDS_BYTES <= R2_LDS_BYTES, "the ring and the h tile must fit one workgroup's LDS");

typedef __attribute__((address_space(3))) void gc_lds_ptr_t;
typedef __attribute__((address_space(1))) const void gc_glb_ptr_t;

// ------------------------------------------------------------------------------------ mu, sigma (rules 2 - 4)
// 16 row groups of 64 lanes, a channel per lane; thread (rg, lc) keeps the canonical groups rg, rg + 16, rg + 32, rg + 48 of its channel
// apart and combines them as canon_sum.h says: the mapping of se_squeeze_kernel<.., 256> with scalar loads (any D, any ldx).
__global__ __launch_bounds__(GC_ST_THREADS) void gctx_stats_kernel(const float* __restrict__ x, int64_t T, int D, int64_t ldx,
                                                                   const int32_t* __restrict__ lens, double eps, double* __restrict__ ctx) {
    __shared__ double red[2][16][64];
    const int b = blockIdx.y;
    const int len = ap_len(lens, b, T);
    const int lc = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lc;
    double s[4] = {0., 0., 0., 0.}, q[4] = {0., 0., 0., 0.};
    if (c < D) {
        const float* xb = x + (int64_t)b * T * ldx + c;
        for (int t0 = rg; t0 < len; t0 += 64) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = t0 + 16 * u;
                if (t < len) {
                    const double v = (double)xb[(int64_t)t * ldx];
                    s[u] += v;
                    q[u] += v * v;
                }
            }
        }
    }
    red[0][rg][lc] = ((s[0] + s[1]) + s[2]) + s[3];
    red[1][rg][lc] = ((q[0] + q[1]) + q[2]) + q[3];
    __syncthreads();
    if (threadIdx.x < 64 && c < D) {
        const double n = (double)len;
        const double mu = ap_total<16>(&red[0][0][lc], 64) / n;
        const double var = ap_total<16>(&red[1][0][lc], 64) / n - mu * mu;
        ctx[((int64_t)b * 2 + 0) * D + c] = mu;
        ctx[((int64_t)b * 2 + 1) * D + c] = sqrt((var < 0. ? 0. : var) + eps);       // (a NaN variance stays NaN)
    }
}

// ------------------------------------------------------------------------------------ g (rule 5)
// Lane l of a wave holds left[row l & 15][k = l >> 4] and right[k = l >> 4][col l & 15]; result register r is [row (l >> 4) + 4 r]
// [col l & 15] (f64_mfma.hip). The left operand, 16 rows of ctx read as (B, 2 D), goes through LDS in chunks of GC_B_KC; the weights
// come as fp32 from global / L2 and are widened in registers, as in se_excite_kernel.
__global__ __launch_bounds__(GC_B_THREADS) void gctx_bias_kernel(const double* __restrict__ ctx, int B, int K, const float* __restrict__ w,
                                                                 int64_t ldw, const float* __restrict__ b1, int A, float* __restrict__ g,
                                                                 int64_t ldg) {
    __shared__ double ps[16][GC_B_KC + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const int b0 = blockIdx.x * 16;
    const int col = (blockIdx.y * 4 + wave) * 16 + lc;
    const double v0 = (b1 && col < A) ? (double)b1[col] : 0.;
    f64x4 acc = f64x4{v0, v0, v0, v0};
    for (int cb = 0; cb < K; cb += GC_B_KC) {
        const int kc = K - cb < GC_B_KC ? K - cb : GC_B_KC;
        __syncthreads();                                          // the last chunk has been read
        for (int i = threadIdx.x; i < 16 * GC_B_KC; i += GC_B_THREADS) {
            const int row = i / GC_B_KC, k = i % GC_B_KC;
            const int b = b0 + row;
            ps[row][k] = (b < B && k < kc) ? ctx[(int64_t)b * K + cb + k] : 0.;
        }
        __syncthreads();
        for (int k0 = 0; k0 < kc; k0 += 4) {
            const int k = k0 + lk;                                // (< GC_B_KC; at or beyond kc the left operand is +0)
            const double bv = (col < A && k < kc) ? (double)w[(int64_t)(cb + k) * ldw + col] : 0.;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ps[lc][k], bv, acc, 0, 0, 0);
        }
    }
    if (col < A) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + lk + 4 * r;
            if (b < B) g[(int64_t)b * ldg + col] = (float)acc[r];
        }
    }
}

// ------------------------------------------------------------------------------------ the logits (rules 6 - 9)
struct GctxParams {
    const float* x;
    const int32_t* lens;
    const float* w1;
    const float* g;
    const float* w2;
    const float* b2;
    float* e;
    int64_t T, ldx, ldw1, ldg, ldw2, lde;
    int32_t D, A, H, act, x_vec, w1_vec, w2_vec;
};

// the lane's 16-byte piece into the wave's 1 KiB of an image at `dst` (wave-uniform): DMA, or the values loaded by the scalar path
__device__ __forceinline__ void gc_dma(const float* src, unsigned char* dst) {
    __builtin_amdgcn_global_load_lds((gc_glb_ptr_t*)src, (gc_lds_ptr_t*)dst, 16, 0, 0);
}

// the lane's eight reduction elements 8 i .. 8 i + 7 of row `row` (byte offset) of the x image under the row's swizzle `sw`
__device__ __forceinline__ void gc_xfrag(const unsigned char* row, int i, int sw, float (&v)[8]) {
    const r2_fv4 v0 = *reinterpret_cast<const r2_fv4*>(row + (((2 * i) ^ sw) << 4));
    const r2_fv4 v1 = *reinterpret_cast<const r2_fv4*>(row + (((2 * i + 1) ^ sw) << 4));
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v0[j], v[4 + j] = v1[j];
}

// ... of a row of the h tile (a pointer to the lane's first element)
__device__ __forceinline__ void gc_hfrag(const float* at, float (&v)[8]) {
    const r2_fv4 v0 = *reinterpret_cast<const r2_fv4*>(at);
    const r2_fv4 v1 = *reinterpret_cast<const r2_fv4*>(at + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v0[j], v[4 + j] = v1[j];
}

// acc[rb] += a[rb] (16 rows x 32) . W image columns at `wcol` (a pointer to W[8 i][col + n]): one chunk of one column block
template <int MODE>
__device__ __forceinline__ void gc_block(const float (&a)[2][8], const r2_bfrag8 (&ah)[2], const r2_bfrag8 (&al)[2], const float* wcol,
                                         f32x4 (&acc)[2]) {
    float w[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) w[s] = wcol[s * GC_WS];
    if constexpr (MODE == KTF_GEMM_F32) {
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb][s], w[s], acc[rb], 0, 0, 0);
    } else {
        r2_bfrag8 wh, wl;
        r2_split8<true>(w, wh, wl);
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[rb], wh, acc[rb], 0, 0, 0);
            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[rb], wh, acc[rb], 0, 0, 0);
            acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[rb], wl, acc[rb], 0, 0, 0);
        }
    }
}

template <int MODE, int NCB>
__global__ __launch_bounds__(GC_THREADS) void gctx_logits_kernel(GctxParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gc_lds[];
    const int b = blockIdx.y;
    const int len = ap_len(p.lens, b, p.T);
    const int t0 = (int)blockIdx.x * GC_R;
    if (t0 >= len) return;                                       // (rule 4: an empty utterance has no tile that runs)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int n = lane & 15, hi = lane >> 4;
    float* hs = reinterpret_cast<float*>(gc_lds + 2 * GC_STAGE_BYTES);
    const int D = p.D, A = p.A, H = p.H;

    // ---- the feed of x: DMA j of wave `wave` fills LDS rows 8 (4 j + wave) .. + 7; the lane's piece is row (lane >> 3), position lane & 7
    const float* px[2];                          // the lane's piece of chunk 0: its frame, clamped to the utterance, its swizzled column
    int xcol[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = 8 * (4 * j + wave) + (lane >> 3);
        xcol[j] = ((lane & 7) ^ ((r >> 1) & 7)) * 4;
        const int t = t0 + r < len ? t0 + r : len - 1;
        px[j] = p.x + ((int64_t)b * p.T + t) * p.ldx + xcol[j];
    }
    auto feed_x = [&](int stage, int k0) {
        const bool vec = p.x_vec && k0 + 32 <= D;               // (wave-uniform)
        unsigned char* st = gc_lds + stage * GC_STAGE_BYTES + wave * 1024;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float* src = px[j] + k0;
            if (vec) {
                gc_dma(src, st + j * 4096);
            } else {
                r2_fv4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = k0 + xcol[j] + i < D ? src[i] : 0.0f;
                *reinterpret_cast<r2_fv4*>(st + j * 4096 + lane * 16) = v;
            }
        }
    };
    // ---- the feed of a weight chunk W[k0 .. k0 + 31][c0 .. c0 + 255] of W (K, N): wave `wave` fills the rows wave, wave + 4, ...
    auto feed_w = [&](int stage, const float* W, int64_t ldw, int k0, int K, int c0, int N, bool wvec) {
        const bool vec = wvec && k0 + 32 <= K;                   // (wave-uniform; wvec says N % 4 == 0, so N - 4 >= c0)
        unsigned char* st = gc_lds + stage * GC_STAGE_BYTES + GC_XBYTES;
        const int c = c0 + 4 * lane;
        const int cv = c + 4 <= N ? c : N - 4;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = wave + 4 * j, k = k0 + kk;
            if (vec) {
                gc_dma(W + (int64_t)k * ldw + cv, st + kk * GC_WROW);
            } else {
                r2_fv4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = (k < K && c + i < N) ? W[(int64_t)k * ldw + c + i] : 0.0f;
                *reinterpret_cast<r2_fv4*>(st + kk * GC_WROW + lane * 16) = v;
            }
        }
    };
    const int nk1 = (D + 31) >> 5, nk2 = (A + 31) >> 5, nb2 = (H + GC_NT - 1) / GC_NT;
    const int total = nk1 + nb2 * nk2;
    auto feed = [&](int s) {
        if (s < nk1) {
            feed_x(s & 1, 32 * s);
            feed_w(s & 1, p.w1, p.ldw1, 32 * s, D, 0, A, p.w1_vec);
        } else {
            const int q = s - nk1, blk = q / nk2, kc = q - blk * nk2;
            feed_w(s & 1, p.w2, p.ldw2, 32 * kc, A, GC_NT * blk, H, p.w2_vec);
        }
    };

    f32x4 acc[8][2];                             // [cb][rb]
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) acc[cb][0] = acc[cb][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int sw = (n >> 1) & 7;                 // (every fragment row of the x image is 16 k + n: the swizzle of row n)
    const int row0 = wm * 32 + n;                // the lane's fragment row of row block 0
    const float* gb = p.g + (int64_t)b * p.ldg;
    float* eb = p.e + (int64_t)b * p.T * p.lde;

    feed(0);
    for (int s = 0; s < total; ++s) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // step s has landed (nothing else is in flight)
        __syncthreads();
        if (s + 1 < total) feed(s + 1);                        // step s + 1 -> the stage every wave has finished reading
        const unsigned char* st = gc_lds + (s & 1) * GC_STAGE_BYTES;
        const float* wimg = reinterpret_cast<const float*>(st + GC_XBYTES) + 8 * hi * GC_WS + n;
        float a[2][8];
        r2_bfrag8 ah[2], al[2];
        if (s < nk1) {
            // ------------------------------------------------ phase 1: chunk s of h = x W1x
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                gc_xfrag(st + (row0 + 16 * rb) * 128, hi, sw, a[rb]);
                if constexpr (MODE != KTF_GEMM_F32) r2_split8<true>(a[rb], ah[rb], al[rb]);
            }
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) gc_block<MODE>(a, ah, al, wimg + 16 * (NCB * wn + cb), acc[cb]);
            if (s == nk1 - 1) {                                // + g_b, act -> the h tile; units at and beyond A as +0
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) {
                    const int col = 16 * (NCB * wn + cb) + n;
                    const float gv = col < A ? gb[col] : 0.0f;
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            float v = acc[cb][rb][i] + gv;
                            if (p.act == KTF_ACT_RELU) v = v < 0.0f ? 0.0f : v;
                            else v = tanhf(v);
                            hs[(wm * 32 + 16 * rb + 4 * hi + i) * GC_WS + col] = col < A ? v : 0.0f;
                        }
                    }
                }
            }
        } else {
            // ------------------------------------------------ phase 2: chunk kc of block blk of e = h W2
            const int q = s - nk1, blk = q / nk2, kc = q - blk * nk2;
            const int j0 = GC_NT * blk + 128 * wn;             // the wave's first head of this block
            if (kc == 0) {
#pragma unroll
                for (int cb = 0; cb < 8; ++cb) acc[cb][0] = acc[cb][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                gc_hfrag(hs + (row0 + 16 * rb) * GC_WS + 32 * kc + 8 * hi, a[rb]);
                if constexpr (MODE != KTF_GEMM_F32) r2_split8<true>(a[rb], ah[rb], al[rb]);
            }
#pragma unroll
            for (int cb = 0; cb < 8; ++cb)
                if (j0 + 16 * cb < H) gc_block<MODE>(a, ah, al, wimg + 128 * wn + 16 * cb, acc[cb]);      // (wave-uniform)
            if (kc == nk2 - 1) {                               // + b2 -> e: rows below len_b, heads below H (rule 8)
#pragma unroll
                for (int cb = 0; cb < 8; ++cb) {
                    const int j = j0 + 16 * cb + n;
                    if (j >= H) continue;
                    const float bv = p.b2 ? p.b2[j] : 0.0f;
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int t = t0 + wm * 32 + 16 * rb + 4 * hi + i;
                            if (t < len) eb[(int64_t)t * p.lde + j] = acc[cb][rb][i] + bv;
                        }
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------ host
static int gc_check_rows(const char* who, int64_t B, int64_t T, int32_t D) {
    KTF_REQUIRE(B >= 0 && T >= 0, "%s: negative size (B %lld, T %lld)", who, (long long)B, (long long)T);
    KTF_REQUIRE(B <= KTF_GCTX_MAX_BATCH && T <= KTF_GCTX_MAX_ROWS, "%s: B %lld above %d or T %lld above %d", who, (long long)B, KTF_GCTX_MAX_BATCH,
                (long long)T, KTF_GCTX_MAX_ROWS);
    KTF_REQUIRE(D >= 1 && D <= KTF_GCTX_MAX_DIM, "%s: D %d outside [1, %d]", who, (int)D, KTF_GCTX_MAX_DIM);
    return KTF_OK;
}

static int gc_check_ld(const char* who, const char* name, int64_t ld, int32_t width) {
    KTF_REQUIRE(ld >= width && ld < (1ll << 31), "%s: %s %lld below its %d columns or at 2^31", who, name, (long long)ld, (int)width);
    return KTF_OK;
}

static int gc_check_shape(const char* who, int32_t A, int32_t H, int32_t gemm) {
    KTF_REQUIRE(A >= 1 && A <= KTF_GCTX_MAX_UNITS, "%s: A %d outside [1, %d]", who, (int)A, KTF_GCTX_MAX_UNITS);
    KTF_REQUIRE(H >= 1 && H <= KTF_GCTX_MAX_DIM, "%s: H %d outside [1, %d]", who, (int)H, KTF_GCTX_MAX_DIM);
    KTF_REQUIRE(gemm == KTF_GEMM_F32 || gemm == KTF_GEMM_BF16X3, "%s: gemm %d is not KTF_GEMM_F32 or KTF_GEMM_BF16X3", who, (int)gemm);
    return KTF_OK;
}

static bool gc_vec(const void* p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

extern "C" int ktf_gctx_stats(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const int32_t* lens, float eps, double* ctx,
                              void* stream) {
    const char* who = "ktf_gctx_stats";
    int rc = gc_check_rows(who, B, T, D);
    if (rc != KTF_OK || (rc = gc_check_ld(who, "ldx", ldx, D)) != KTF_OK) return rc;
    KTF_REQUIRE(eps >= 0.0f && eps <= 3.402823466e+38f, "%s: eps must be finite and >= 0", who);
    KTF_REQUIRE(ctx != nullptr, "%s: null ctx", who);
    KTF_REQUIRE(x != nullptr || B * T == 0, "%s: null x", who);
    if (B == 0) return KTF_OK;
    hipLaunchKernelGGL(gctx_stats_kernel, dim3((unsigned)ktf_cdiv(D, 64), (unsigned)B), dim3(GC_ST_THREADS), 0, (hipStream_t)stream, x, T, (int)D, ldx,
                       lens, (double)eps, ctx);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_gctx_bias(const double* ctx, int64_t B, int32_t D, const float* w1c, int64_t ldw, const float* b1, int32_t A, float* g,
                             int64_t ldg, void* stream) {
    const char* who = "ktf_gctx_bias";
    int rc = gc_check_rows(who, B, 0, D);
    if (rc != KTF_OK || (rc = gc_check_shape(who, A, 1, KTF_GEMM_F32)) != KTF_OK) return rc;
    if ((rc = gc_check_ld(who, "ldw", ldw, A)) != KTF_OK || (rc = gc_check_ld(who, "ldg", ldg, A)) != KTF_OK) return rc;
    KTF_REQUIRE(B == 0 || (ctx && w1c && g), "%s: null ctx, w1c or g", who);
    if (B == 0) return KTF_OK;
    hipLaunchKernelGGL(gctx_bias_kernel, dim3((unsigned)ktf_cdiv(B, 16), (unsigned)ktf_cdiv(A, 64)), dim3(GC_B_THREADS), 0, (hipStream_t)stream, ctx, (int)B,
                       2 * (int)D, w1c, ldw, b1, (int)A, g, ldg);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int32_t ktf_gctx_row_tile(int32_t A, int32_t H, int32_t gemm) {
    if (int rc = gc_check_shape("ktf_gctx_row_tile", A, H, gemm)) return rc;
    return GC_R;                                               // (one tile shape: the h tile holds every unit of its rows)
}

template <int MODE, int NCB>
static void gc_launch(const GctxParams& p, dim3 grid, hipStream_t st) {
    KTF_LDS_ONCE(GC_LDS_BYTES, gctx_logits_kernel<MODE, NCB>);
    hipLaunchKernelGGL((gctx_logits_kernel<MODE, NCB>), grid, dim3(GC_THREADS), GC_LDS_BYTES, st, p);
}

template <int MODE>
static void gc_launch_units(const GctxParams& p, dim3 grid, hipStream_t st) {
    if (p.A <= 64) gc_launch<MODE, 2>(p, grid, st);
    else if (p.A <= 128) gc_launch<MODE, 4>(p, grid, st);
    else gc_launch<MODE, 8>(p, grid, st);
}

extern "C" int ktf_gctx_logits(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const int32_t* lens, const float* w1x, int64_t ldw1,
                               const float* g, int64_t ldg, int32_t A, int32_t act, const float* w2, int64_t ldw2, const float* b2, int32_t H,
                               int32_t gemm, float* e, int64_t lde, void* stream) {
    const char* who = "ktf_gctx_logits";
    int rc = gc_check_rows(who, B, T, D);
    if (rc != KTF_OK || (rc = gc_check_shape(who, A, H, gemm)) != KTF_OK) return rc;
    KTF_REQUIRE(act == KTF_ACT_TANH || act == KTF_ACT_RELU, "%s: act %d is not KTF_ACT_TANH or KTF_ACT_RELU", who, (int)act);
    if ((rc = gc_check_ld(who, "ldx", ldx, D)) != KTF_OK || (rc = gc_check_ld(who, "ldw1", ldw1, A)) != KTF_OK ||
        (rc = gc_check_ld(who, "ldg", ldg, A)) != KTF_OK || (rc = gc_check_ld(who, "ldw2", ldw2, H)) != KTF_OK ||
        (rc = gc_check_ld(who, "lde", lde, H)) != KTF_OK)
        return rc;
    KTF_REQUIRE(B * T == 0 || (x && w1x && g && w2 && e), "%s: null x, w1x, g, w2 or e", who);
    if (B * T == 0) return KTF_OK;

    GctxParams p = {};
    p.x = x, p.lens = lens, p.w1 = w1x, p.g = g, p.w2 = w2, p.b2 = b2, p.e = e;
    p.T = T, p.ldx = ldx, p.ldw1 = ldw1, p.ldg = ldg, p.ldw2 = ldw2, p.lde = lde;
    p.D = D, p.A = A, p.H = H, p.act = act;
    p.x_vec = gc_vec(x, ldx), p.w1_vec = gc_vec(w1x, ldw1) && A % 4 == 0, p.w2_vec = gc_vec(w2, ldw2) && H % 4 == 0;
    const dim3 grid((unsigned)ktf_cdiv(T, GC_R), (unsigned)B);                // <= 2^24 x 65535
    hipStream_t st = (hipStream_t)stream;
    if (gemm == KTF_GEMM_F32) gc_launch_units<KTF_GEMM_F32>(p, grid, st);
    else gc_launch_units<KTF_GEMM_BF16X3>(p, grid, st);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
