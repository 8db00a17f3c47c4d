// The gradient of the global-context attention logits (include/ktf_gcgrad.h states the contract as numbered rules, INTEGRATION.md
// section 2w the use, DESIGN.md section 7 the design and the measurements). Five kernels behind three entry points:
//
//   ktf_gcgrad_hidden    gcgrad_hidden_kernel   one workgroup = 64 rows of one utterance: z, h recomputed, dz = (de W2^T) act'(z)   (rules 2 - 4)
//   ktf_gcgrad_context   gcgrad_dg_kernel       one workgroup = one utterance x 64 units: dg = sum_t dz in fp64, the canonical order
//                        gcgrad_dctx_kernel     one wave = 16 utterances x 16 context channels: dctx = dg W1c^T on fp64 MFMA -> coef
//                        gcgrad_w1c_kernel      one wave = 16 context channels x 16 units: dW1c = ctx^T dg, db1 on fp64 MFMA      (rules 5, 6)
//   ktf_gcgrad_data      gcgrad_data_kernel     one workgroup = 64 rows of one utterance: dx (+)= dz W1x^T + the two context terms (rule 7)
//
// The two big kernels keep the tile of csrc/attn_ctx.hip: four waves, a wave owns 32 rows x 128 columns as sixteen 16 x 16 accumulators,
// lane (n = lane & 15, i = lane >> 4) of block (rb, cb) holding rows 16 rb + 4 i + 0 .. 3 of column 16 cb + n; lane group i supplies the
// reduction elements 8 i .. 8 i + 7 of a chunk of 32 of either operand (F32: eight v_mfma_f32_16x16x4_f32; BF16X3: the fragments split in
// registers into three v_mfma_f32_16x16x32_bf16). A ring of two LDS stages is fed one step ahead, one barrier per step.
//
// What is new is the TRANSPOSED weight operand. Both gradient products reduce over the weight's column index -- dh = de W2^T reduces over
// the heads j of W2 (A, H), dz W1x^T over the units a of W1x (D, A) -- so the 32 reduction elements of an output column are CONTIGUOUS in
// the weight's row. The weight chunk therefore goes into LDS as a "row image" like x: 256 rows (output columns) x 128 bytes (the 32
// reduction elements), 16-byte piece p of row r at position p ^ ((r >> 1) & 7). A lane's eight reduction elements of its column are
// two 16-byte LDS reads (against eight scalar reads from the k-major image of the forward), the sixteen columns of a fragment fall on
// disjoint banks, and a row image is fed by eight 16-byte LDS-DMAs per lane and step with no transposition anywhere. Rows beyond the
// operand (units >= A, channels >= D) are fed from the last row by the DMA and as +0 by the scalar feed; what they compute is never stored.
//
// gcgrad_hidden_kernel, one flat loop of nk1 + nkh steps (nk1 = ceil(D / 32), nkh = ceil(H / 32)):
//   phase 1, step k < nk1: the step of gctx_logits_kernel -- x image 64 x 32, W1x image 32 x 256 k-major -- so z and h have the
//     forward's bits; its epilogue writes h = act(z + g_b) into the LDS tile (64 rows x 260 floats).
//   phase 2, step k: the stage holds the de image 64 rows x 32 heads and the W2 row image 256 units x 32 heads; the accumulators are
//     dh (rows x units), at the SAME lane positions as phase 1, so the epilogue multiplies by act' from the lane's own h in LDS and
//     stores dz and h (rows at and beyond len_b as +0).
//   LDS: 2 x 41472 (stage) + 66560 (h tile) = 149504 bytes, one workgroup per compute unit.
// gcgrad_data_kernel: the dz tile (64 x A) is loaded into the 260-float tile once; one flat loop of ceil(D / 256) ceil(A / 32) steps,
//   the stage holding the W1x row image 256 channels x 32 units; the epilogue of a block's last chunk reads x and (accumulate) dx, adds
//   the context terms in fp64 and writes dx once. LDS: 2 x 32768 + 66560 = 132096 bytes.
#include "res2_common.h"
#include "canon_sum.h"
#include "f64_mfma.h"
#include "../../include/ktf_gcgrad.h"

// every operation is rounded on its own: no contraction into fma, in any kernel of this file
#pragma clang fp contract(off)

#define GG_THREADS 256
#define GG_R 64
#define GG_NT 256                                 // columns of a weight image
#define GG_XBYTES 8192                            // a row image of 64 rows of 128 bytes
#define GG_TBYTES 32768                           // a row image of 256 rows of 128 bytes
#define GG_WS 260                                 // floats per row of the k-major W image and of the h / dz tile
#define GG_WROW (GG_WS * 4)
#define GG_STAGE_BYTES (GG_XBYTES + 32 * GG_WROW)
#define GG_H_BYTES (GG_R * GG_WS * 4)
#define GG_LDS_HIDDEN (2 * GG_STAGE_BYTES + GG_H_BYTES)
#define GG_LDS_DATA (2 * GG_TBYTES + GG_H_BYTES)
#define GG_ST_THREADS 1024
#define GG_B_THREADS 256
#define GG_B_KC 128

static_assert(GG_XBYTES + GG_TBYTES <= GG_STAGE_BYTES, "phase 2 of the hidden kernel reuses the stage of phase 1");
static_assert(GG_LDS_HIDDEN <= R2_LDS_BYTES && GG_LDS_DATA <= R2_LDS_BYTES, "the ring and the tile must fit one workgroup's LDS");

typedef __attribute__((address_space(3))) void gg_lds_ptr_t;
typedef __attribute__((address_space(1))) const void gg_glb_ptr_t;

__device__ __forceinline__ void gg_dma(const float* src, unsigned char* dst) {
    __builtin_amdgcn_global_load_lds((gg_glb_ptr_t*)src, (gg_lds_ptr_t*)dst, 16, 0, 0);
}

// the lane's eight reduction elements 8 i .. 8 i + 7 of row `row` (a pointer) of a row image under the row's swizzle `sw`
__device__ __forceinline__ void gg_rowfrag(const unsigned char* row, int i, int sw, float (&v)[8]) {
    const r2_fv4 v0 = *reinterpret_cast<const r2_fv4*>(row + (((2 * i) ^ sw) << 4));
    const r2_fv4 v1 = *reinterpret_cast<const r2_fv4*>(row + (((2 * i + 1) ^ sw) << 4));
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v0[j], v[4 + j] = v1[j];
}

// ... of a row of the h / dz tile (a pointer to the lane's first element)
__device__ __forceinline__ void gg_tilefrag(const float* at, float (&v)[8]) {
    const r2_fv4 v0 = *reinterpret_cast<const r2_fv4*>(at);
    const r2_fv4 v1 = *reinterpret_cast<const r2_fv4*>(at + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v0[j], v[4 + j] = v1[j];
}

// acc[rb] += a[rb] (16 rows x 32) . w (the lane's eight reduction elements of its column): one chunk of one column block
template <int MODE>
__device__ __forceinline__ void gg_mma(const float (&a)[2][8], const r2_bfrag8 (&ah)[2], const r2_bfrag8 (&al)[2], const float (&w)[8],
                                       f32x4 (&acc)[2]) {
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

// The feed of a row image of 256 rows: rows r0 .. r0 + 255 of W (N rows of K reduction elements, leading dimension ldw), the reduction
// elements k0 .. k0 + 31. DMA j of wave `wave` fills LDS rows 8 (4 j + wave) .. + 7; the lane's piece is row (lane >> 3), position lane & 7.
__device__ __forceinline__ void gg_feed_rows256(unsigned char* img, const float* W, int64_t ldw, int r0, int N, int k0, int K, bool wvec, int wave,
                                                int lane) {
    const bool vec = wvec && k0 + 32 <= K;                       // (wave-uniform)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int r = 8 * (4 * j + wave) + (lane >> 3);
        const int col = ((lane & 7) ^ ((r >> 1) & 7)) * 4;
        const int row = r0 + r;
        unsigned char* dst = img + (4 * j + wave) * 1024;
        if (vec) {
            gg_dma(W + (int64_t)(row < N ? row : N - 1) * ldw + k0 + col, dst);
        } else {
            r2_fv4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = (row < N && k0 + col + i < K) ? W[(int64_t)row * ldw + k0 + col + i] : 0.0f;
            *reinterpret_cast<r2_fv4*>(dst + lane * 16) = v;
        }
    }
}

// ------------------------------------------------------------------------------------ dz and h (rules 2 - 4)
struct GcgradHiddenParams {
    const float* x;
    const int32_t* lens;
    const float* w1;
    const float* g;
    const float* w2;
    const float* de;
    float* dz;
    float* h;
    int64_t T, ldx, ldw1, ldg, ldw2, lde, ldz;
    int32_t D, A, H, act, x_vec, w1_vec, w2_vec, de_vec;
};

template <int MODE, int NCB>
__global__ __launch_bounds__(GG_THREADS) void gcgrad_hidden_kernel(GcgradHiddenParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gg_lds[];
    const int b = blockIdx.y;
    const int len = ap_len(p.lens, b, p.T);
    const int t0 = (int)blockIdx.x * GG_R;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = p.D, A = p.A, H = p.H;
    float* dzb = p.dz + (int64_t)b * p.T * p.ldz;
    float* hb = p.h + (int64_t)b * p.T * p.ldz;
    if (t0 >= len) {                                             // (rule 4: a tile past the utterance writes its rows as +0)
        const int rows = p.T - t0 < GG_R ? (int)(p.T - t0) : GG_R;
        for (int i = tid; i < rows * A; i += GG_THREADS) {
            const int64_t at = (int64_t)(t0 + i / A) * p.ldz + i % A;
            dzb[at] = 0.0f, hb[at] = 0.0f;
        }
        return;
    }
    const int wm = wave >> 1, wn = wave & 1;
    const int n = lane & 15, hi = lane >> 4;
    float* hs = reinterpret_cast<float*>(gg_lds + 2 * GG_STAGE_BYTES);

    // ---- the feed of a 64-row image (x, de): DMA j of wave `wave` fills LDS rows 8 (4 j + wave) .. + 7
    const float* px[2];
    const float* pd[2];
    int xcol[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = 8 * (4 * j + wave) + (lane >> 3);
        xcol[j] = ((lane & 7) ^ ((r >> 1) & 7)) * 4;
        const int t = t0 + r < len ? t0 + r : len - 1;         // (rows are clamped to the utterance where they are read)
        px[j] = p.x + ((int64_t)b * p.T + t) * p.ldx + xcol[j];
        pd[j] = p.de + ((int64_t)b * p.T + t) * p.lde + xcol[j];
    }
    auto feed_rows64 = [&](int stage, const float* const (&ptr)[2], int k0, int K, bool rvec) {
        const bool vec = rvec && k0 + 32 <= K;                   // (wave-uniform)
        unsigned char* st = gg_lds + stage * GG_STAGE_BYTES + wave * 1024;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float* src = ptr[j] + k0;
            if (vec) {
                gg_dma(src, st + j * 4096);
            } else {
                r2_fv4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = k0 + xcol[j] + i < K ? src[i] : 0.0f;
                *reinterpret_cast<r2_fv4*>(st + j * 4096 + lane * 16) = v;
            }
        }
    };
    // ---- the k-major feed of W1x[k0 .. k0 + 31][0 .. 255] (the forward's): wave `wave` fills the rows wave, wave + 4, ...
    auto feed_w1 = [&](int stage, int k0) {
        const bool vec = p.w1_vec && k0 + 32 <= D;               // (wave-uniform; w1_vec says A % 4 == 0, so A - 4 >= 0)
        unsigned char* st = gg_lds + stage * GG_STAGE_BYTES + GG_XBYTES;
        const int c = 4 * lane;
        const int cv = c + 4 <= A ? c : A - 4;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = wave + 4 * j, k = k0 + kk;
            if (vec) {
                gg_dma(p.w1 + (int64_t)k * p.ldw1 + cv, st + kk * GG_WROW);
            } else {
                r2_fv4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = (k < D && c + i < A) ? p.w1[(int64_t)k * p.ldw1 + c + i] : 0.0f;
                *reinterpret_cast<r2_fv4*>(st + kk * GG_WROW + lane * 16) = v;
            }
        }
    };
    const int nk1 = (D + 31) >> 5, nkh = (H + 31) >> 5;
    const int total = nk1 + nkh;
    auto feed = [&](int s) {
        if (s < nk1) {
            feed_rows64(s & 1, px, 32 * s, D, p.x_vec);
            feed_w1(s & 1, 32 * s);
        } else {
            const int k0 = 32 * (s - nk1);
            feed_rows64(s & 1, pd, k0, H, p.de_vec);
            gg_feed_rows256(gg_lds + (s & 1) * GG_STAGE_BYTES + GG_XBYTES, p.w2, p.ldw2, 0, A, k0, H, p.w2_vec, wave, lane);
        }
    };

    f32x4 acc[NCB][2];                           // [cb][rb]
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) acc[cb][0] = acc[cb][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int sw = (n >> 1) & 7;                 // (every fragment row of a row image is 16 k + n: the swizzle of row n)
    const int row0 = wm * 32 + n;                // the lane's fragment row of row block 0
    const float* gb = p.g + (int64_t)b * p.ldg;

    feed(0);
    for (int s = 0; s < total; ++s) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // step s has landed (nothing else is in flight)
        __syncthreads();
        if (s + 1 < total) feed(s + 1);                        // step s + 1 -> the stage every wave has finished reading
        const unsigned char* st = gg_lds + (s & 1) * GG_STAGE_BYTES;
        float a[2][8];
        r2_bfrag8 ah[2], al[2];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {                       // the left operand of either phase: the lane's rows of the 64-row image
            gg_rowfrag(st + (row0 + 16 * rb) * 128, hi, sw, a[rb]);
            if constexpr (MODE != KTF_GEMM_F32) r2_split8<true>(a[rb], ah[rb], al[rb]);
        }
        if (s < nk1) {
            // ------------------------------------------------ phase 1: chunk s of z = x W1x (the forward's arithmetic)
            const float* wimg = reinterpret_cast<const float*>(st + GG_XBYTES) + 8 * hi * GG_WS + n;
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                float w[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) w[q] = wimg[16 * (NCB * wn + cb) + q * GG_WS];
                gg_mma<MODE>(a, ah, al, w, acc[cb]);
            }
            if (s == nk1 - 1) {                                // + g_b, act -> the h tile; then the accumulators start over for dh
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
                            hs[(wm * 32 + 16 * rb + 4 * hi + i) * GG_WS + col] = col < A ? v : 0.0f;
                        }
                        acc[cb][rb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    }
                }
            }
        } else {
            // ------------------------------------------------ phase 2: chunk s - nk1 of dh = de W2^T
            const unsigned char* timg = st + GG_XBYTES;
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                float w[8];
                gg_rowfrag(timg + (16 * (NCB * wn + cb) + n) * 128, hi, sw, w);
                gg_mma<MODE>(a, ah, al, w, acc[cb]);
            }
        }
    }
    // ---- dz = dh act'(z) from the lane's own h; rows at and beyond len_b as +0 (rule 4)
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        const int col = 16 * (NCB * wn + cb) + n;
        if (col >= A) continue;
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = wm * 32 + 16 * rb + 4 * hi + i;
                const int t = t0 + r;
                if (t >= p.T) continue;
                const float hv = hs[r * GG_WS + col];
                const float d = p.act == KTF_ACT_RELU ? (hv > 0.0f ? 1.0f : 0.0f) : 1.0f - hv * hv;
                const bool live = t < len;
                dzb[(int64_t)t * p.ldz + col] = live ? acc[cb][rb][i] * d : 0.0f;
                hb[(int64_t)t * p.ldz + col] = live ? hv : 0.0f;
            }
        }
    }
}

// ------------------------------------------------------------------------------------ dx (rule 7)
struct GcgradDataParams {
    const float* dz;
    const int32_t* lens;
    const float* w1;
    const float* x;
    const double* ctx;
    const double* coef;
    float* dx;
    int64_t T, ldz, ldw1, ldx, lddx;
    int32_t D, A, w1_vec, accumulate;
};

template <int MODE>
__global__ __launch_bounds__(GG_THREADS) void gcgrad_data_kernel(GcgradDataParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gg_lds[];
    const int b = blockIdx.y;
    const int len = ap_len(p.lens, b, p.T);
    const int t0 = (int)blockIdx.x * GG_R;
    if (t0 >= len) return;                                       // (rows at and beyond len_b are left untouched)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int n = lane & 15, hi = lane >> 4;
    const int D = p.D, A = p.A;
    float* zs = reinterpret_cast<float*>(gg_lds + 2 * GG_TBYTES);
    const int nk = (A + 31) >> 5, nb = (D + GG_NT - 1) / GG_NT;
    const int total = nb * nk;
    auto feed = [&](int s) {
        const int blk = s / nk, kc = s - blk * nk;
        gg_feed_rows256(gg_lds + (s & 1) * GG_TBYTES, p.w1, p.ldw1, GG_NT * blk, D, 32 * kc, A, p.w1_vec, wave, lane);
    };
    feed(0);
    // ---- the dz tile: units at and beyond A as +0, rows clamped to the utterance (what they compute is never stored)
    for (int i = tid; i < GG_R * GG_NT; i += GG_THREADS) {
        const int r = i >> 8, col = i & 255;
        const int t = t0 + r < len ? t0 + r : len - 1;
        zs[r * GG_WS + col] = col < A ? p.dz[((int64_t)b * p.T + t) * p.ldz + col] : 0.0f;
    }
    f32x4 acc[8][2];
    const int sw = (n >> 1) & 7;
    const int row0 = wm * 32 + n;
    const int64_t brow = (int64_t)b * p.T;
    const double* cb0 = p.coef + (int64_t)b * 2 * D;
    const double* mub = p.ctx + (int64_t)b * 2 * D;
    for (int s = 0; s < total; ++s) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                       // (the first one also publishes the dz tile)
        if (s + 1 < total) feed(s + 1);
        const unsigned char* timg = gg_lds + (s & 1) * GG_TBYTES;
        const int blk = s / nk, kc = s - blk * nk;
        const int c0 = GG_NT * blk + 128 * wn;                 // the wave's first channel of this block
        if (kc == 0) {
#pragma unroll
            for (int cb = 0; cb < 8; ++cb) acc[cb][0] = acc[cb][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        float a[2][8];
        r2_bfrag8 ah[2], al[2];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) {
            gg_tilefrag(zs + (row0 + 16 * rb) * GG_WS + 32 * kc + 8 * hi, a[rb]);
            if constexpr (MODE != KTF_GEMM_F32) r2_split8<true>(a[rb], ah[rb], al[rb]);
        }
#pragma unroll
        for (int cb = 0; cb < 8; ++cb) {
            if (c0 + 16 * cb >= D) continue;                   // (wave-uniform)
            float w[8];
            gg_rowfrag(timg + (128 * wn + 16 * cb + n) * 128, hi, sw, w);
            gg_mma<MODE>(a, ah, al, w, acc[cb]);
        }
        if (kc == nk - 1) {                                    // + the context terms in fp64 -> dx, once (rule 7)
#pragma unroll
            for (int cb = 0; cb < 8; ++cb) {
                const int c = c0 + 16 * cb + n;
                if (c >= D) continue;
                const double k0 = cb0[c], k1 = cb0[D + c], mu = mub[c];
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int t = t0 + wm * 32 + 16 * rb + 4 * hi + i;
                        if (t >= len) continue;
                        float* at = p.dx + (brow + t) * p.lddx + c;
                        const double in = p.accumulate ? (double)*at : 0.;
                        const double xv = (double)p.x[(brow + t) * p.ldx + c];
                        *at = (float)((((double)acc[cb][rb][i] + in) + k0) + k1 * (xv - mu));
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------ dg (rule 5): the mapping of gctx_stats_kernel
__global__ __launch_bounds__(GG_ST_THREADS) void gcgrad_dg_kernel(const float* __restrict__ dz, int64_t T, int A, int64_t ldz,
                                                                  const int32_t* __restrict__ lens, double* __restrict__ dg) {
    __shared__ double red[16][64];
    const int b = blockIdx.y;
    const int len = ap_len(lens, b, T);
    const int lc = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int a = blockIdx.x * 64 + lc;
    double s[4] = {0., 0., 0., 0.};
    if (a < A) {
        const float* zb = dz + (int64_t)b * T * ldz + a;
        for (int t0 = rg; t0 < len; t0 += 64) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = t0 + 16 * u;
                if (t < len) s[u] += (double)zb[(int64_t)t * ldz];
            }
        }
    }
    red[rg][lc] = ((s[0] + s[1]) + s[2]) + s[3];
    __syncthreads();
    if (threadIdx.x < 64 && a < A) dg[(int64_t)b * A + a] = ap_total<16>(&red[0][lc], 64);
}

// ------------------------------------------------------------------------------------ dctx -> coef (rules 5, 6)
// Lane l of a wave holds left[row l & 15][k = l >> 4] and right[k = l >> 4][col l & 15]; result register r is [row (l >> 4) + 4 r]
// [col l & 15] (f64_mfma.hip). Rows are utterances, columns the 2 D context channels, the reduction runs over the units.
__global__ __launch_bounds__(GG_B_THREADS) void gcgrad_dctx_kernel(const double* __restrict__ dg, int B, int64_t T, int A, int D,
                                                                   const int32_t* __restrict__ lens, const double* __restrict__ ctx,
                                                                   const float* __restrict__ w, int64_t ldw, double eps, double* __restrict__ coef) {
    __shared__ double ps[16][GG_B_KC + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const int b0 = blockIdx.x * 16;
    const int col = (blockIdx.y * 4 + wave) * 16 + lc;
    f64x4 acc = f64x4{0., 0., 0., 0.};
    for (int cb = 0; cb < A; cb += GG_B_KC) {
        const int kc = A - cb < GG_B_KC ? A - cb : GG_B_KC;
        __syncthreads();                                          // the last chunk has been read
        for (int i = threadIdx.x; i < 16 * GG_B_KC; i += GG_B_THREADS) {
            const int row = i / GG_B_KC, k = i % GG_B_KC;
            const int b = b0 + row;
            ps[row][k] = (b < B && k < kc) ? dg[(int64_t)b * A + cb + k] : 0.;
        }
        __syncthreads();
        for (int k0 = 0; k0 < kc; k0 += 4) {
            const int k = k0 + lk;
            const double bv = (col < 2 * D && k < kc) ? (double)w[(int64_t)col * ldw + cb + k] : 0.;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ps[lc][k], bv, acc, 0, 0, 0);
        }
    }
    if (col < 2 * D) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + lk + 4 * r;
            if (b >= B) continue;
            const int len = ap_len(lens, b, T);
            const double nn = (double)len;
            double v = 0.;
            if (len > 0) {
                if (col < D) {
                    v = acc[r] / nn;
                } else {
                    const double sig = ctx[(int64_t)b * 2 * D + col];
                    v = sig * sig > eps ? acc[r] / (nn * sig) : 0.;
                }
            }
            coef[(int64_t)b * 2 * D + col] = v;
        }
    }
}

// ------------------------------------------------------------------------------------ dW1c, db1 (rule 5)
// Rows are the context channels k < 2 D plus one row of ones (k = 2 D: db1), columns the units, the reduction runs over the utterances
// in ascending order, four per instruction; an empty utterance enters as zero.
__global__ __launch_bounds__(GG_B_THREADS) void gcgrad_w1c_kernel(const double* __restrict__ dg, int B, int64_t T, int A, int D,
                                                                  const int32_t* __restrict__ lens, const double* __restrict__ ctx,
                                                                  float* __restrict__ dw, int64_t lddw, float* __restrict__ db1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const int krow = blockIdx.x * 16 + lc;                        // the lane's row of the left operand
    const int col = (blockIdx.y * 4 + wave) * 16 + lc;
    const int K2 = 2 * D;
    f64x4 acc = f64x4{0., 0., 0., 0.};
    for (int bb = 0; bb < B; bb += 4) {
        const int b = bb + lk;
        const bool live = b < B && ap_len(lens, b, T) > 0;
        double av = 0., bv = 0.;
        if (live) {
            av = krow < K2 ? ctx[(int64_t)b * K2 + krow] : (krow == K2 ? 1. : 0.);
            bv = col < A ? dg[(int64_t)b * A + col] : 0.;
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    if (col < A) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = blockIdx.x * 16 + lk + 4 * r;
            if (k < K2) {
                if (dw) dw[(int64_t)k * lddw + col] = (float)acc[r];
            } else if (k == K2 && db1) {
                db1[col] = (float)acc[r];
            }
        }
    }
}

// ------------------------------------------------------------------------------------ host
static int gg_check_rows(const char* who, int64_t B, int64_t T, int32_t D) {
    KTF_REQUIRE(B >= 0 && T >= 0, "%s: negative size (B %lld, T %lld)", who, (long long)B, (long long)T);
    KTF_REQUIRE(B <= KTF_GCTX_MAX_BATCH && T <= KTF_GCTX_MAX_ROWS, "%s: B %lld above %d or T %lld above %d", who, (long long)B, KTF_GCTX_MAX_BATCH,
                (long long)T, KTF_GCTX_MAX_ROWS);
    KTF_REQUIRE(D >= 1 && D <= KTF_GCTX_MAX_DIM, "%s: D %d outside [1, %d]", who, (int)D, KTF_GCTX_MAX_DIM);
    return KTF_OK;
}

static int gg_check_ld(const char* who, const char* name, int64_t ld, int32_t width) {
    KTF_REQUIRE(ld >= width && ld < (1ll << 31), "%s: %s %lld below its %d columns or at 2^31", who, name, (long long)ld, (int)width);
    return KTF_OK;
}

static int gg_check_shape(const char* who, int32_t A, int32_t H, int32_t gemm) {
    KTF_REQUIRE(A >= 1 && A <= KTF_GCTX_MAX_UNITS, "%s: A %d outside [1, %d]", who, (int)A, KTF_GCTX_MAX_UNITS);
    KTF_REQUIRE(H >= 1 && H <= KTF_GCTX_MAX_DIM, "%s: H %d outside [1, %d]", who, (int)H, KTF_GCTX_MAX_DIM);
    KTF_REQUIRE(gemm == KTF_GEMM_F32 || gemm == KTF_GEMM_BF16X3, "%s: gemm %d is not KTF_GEMM_F32 or KTF_GEMM_BF16X3", who, (int)gemm);
    return KTF_OK;
}

static bool gg_vec(const void* p, int64_t ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

extern "C" int32_t ktf_gcgrad_row_tile(int32_t A, int32_t H, int32_t gemm) {
    if (int rc = gg_check_shape("ktf_gcgrad_row_tile", A, H, gemm)) return rc;
    return GG_R;                                               // (one tile shape: the h / dz tile holds every unit of its rows)
}

extern "C" int64_t ktf_gcgrad_workspace_bytes(int64_t B, int32_t A) {
    const char* who = "ktf_gcgrad_workspace_bytes";
    if (int rc = gg_check_rows(who, B, 0, 1)) return rc;
    if (int rc = gg_check_shape(who, A, 1, KTF_GEMM_F32)) return rc;
    return al256(B * A * (int64_t)sizeof(double));
}

template <int MODE, int NCB>
static void gg_launch_hidden(const GcgradHiddenParams& p, dim3 grid, hipStream_t st) {
    KTF_LDS_ONCE(GG_LDS_HIDDEN, gcgrad_hidden_kernel<MODE, NCB>);
    hipLaunchKernelGGL((gcgrad_hidden_kernel<MODE, NCB>), grid, dim3(GG_THREADS), GG_LDS_HIDDEN, st, p);
}

template <int MODE>
static void gg_launch_hidden_units(const GcgradHiddenParams& p, dim3 grid, hipStream_t st) {
    if (p.A <= 64) gg_launch_hidden<MODE, 2>(p, grid, st);
    else if (p.A <= 128) gg_launch_hidden<MODE, 4>(p, grid, st);
    else gg_launch_hidden<MODE, 8>(p, grid, st);
}

extern "C" int ktf_gcgrad_hidden(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const int32_t* lens, const float* w1x, int64_t ldw1,
                                 const float* g, int64_t ldg, int32_t A, int32_t act, const float* w2, int64_t ldw2, int32_t H, int32_t gemm,
                                 const float* de, int64_t lde, float* dz, float* h, int64_t ldz, void* stream) {
    const char* who = "ktf_gcgrad_hidden";
    int rc = gg_check_rows(who, B, T, D);
    if (rc != KTF_OK || (rc = gg_check_shape(who, A, H, gemm)) != KTF_OK) return rc;
    KTF_REQUIRE(act == KTF_ACT_TANH || act == KTF_ACT_RELU, "%s: act %d is not KTF_ACT_TANH or KTF_ACT_RELU", who, (int)act);
    if ((rc = gg_check_ld(who, "ldx", ldx, D)) != KTF_OK || (rc = gg_check_ld(who, "ldw1", ldw1, A)) != KTF_OK ||
        (rc = gg_check_ld(who, "ldg", ldg, A)) != KTF_OK || (rc = gg_check_ld(who, "ldw2", ldw2, H)) != KTF_OK ||
        (rc = gg_check_ld(who, "lde", lde, H)) != KTF_OK || (rc = gg_check_ld(who, "ldz", ldz, A)) != KTF_OK)
        return rc;
    KTF_REQUIRE(B * T == 0 || (x && w1x && g && w2 && de && dz && h), "%s: null x, w1x, g, w2, de, dz or h", who);
    if (B * T == 0) return KTF_OK;

    GcgradHiddenParams p = {};
    p.x = x, p.lens = lens, p.w1 = w1x, p.g = g, p.w2 = w2, p.de = de, p.dz = dz, p.h = h;
    p.T = T, p.ldx = ldx, p.ldw1 = ldw1, p.ldg = ldg, p.ldw2 = ldw2, p.lde = lde, p.ldz = ldz;
    p.D = D, p.A = A, p.H = H, p.act = act;
    p.x_vec = gg_vec(x, ldx), p.w1_vec = gg_vec(w1x, ldw1) && A % 4 == 0, p.w2_vec = gg_vec(w2, ldw2), p.de_vec = gg_vec(de, lde);
    const dim3 grid((unsigned)ktf_cdiv(T, GG_R), (unsigned)B);                // <= 2^24 x 65535
    hipStream_t st = (hipStream_t)stream;
    if (gemm == KTF_GEMM_F32) gg_launch_hidden_units<KTF_GEMM_F32>(p, grid, st);
    else gg_launch_hidden_units<KTF_GEMM_BF16X3>(p, grid, st);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_gcgrad_context(const float* dz, int64_t B, int64_t T, int32_t A, int64_t ldz, const int32_t* lens, const double* ctx, int32_t D,
                                  const float* w1c, int64_t ldw, float eps, float* dw1c, int64_t lddw, float* db1, double* coef, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    const char* who = "ktf_gcgrad_context";
    int rc = gg_check_rows(who, B, T, D);
    if (rc != KTF_OK || (rc = gg_check_shape(who, A, 1, KTF_GEMM_F32)) != KTF_OK) return rc;
    if ((rc = gg_check_ld(who, "ldz", ldz, A)) != KTF_OK || (rc = gg_check_ld(who, "ldw", ldw, A)) != KTF_OK ||
        (dw1c && (rc = gg_check_ld(who, "lddw", lddw, A)) != KTF_OK))
        return rc;
    KTF_REQUIRE(eps >= 0.0f && eps <= 3.402823466e+38f, "%s: eps must be finite and >= 0", who);
    KTF_REQUIRE(B == 0 || (ctx && w1c && coef && workspace), "%s: null ctx, w1c, coef or workspace", who);
    KTF_REQUIRE(B * T == 0 || dz, "%s: null dz", who);
    if (B == 0) return KTF_OK;
    if ((rc = ktf_check_workspace(who, workspace, workspace_bytes, ktf_gcgrad_workspace_bytes(B, A))) != KTF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    double* dg = (double*)workspace;
    hipLaunchKernelGGL(gcgrad_dg_kernel, dim3((unsigned)ktf_cdiv(A, 64), (unsigned)B), dim3(GG_ST_THREADS), 0, st, dz, T, (int)A, ldz, lens, dg);
    hipLaunchKernelGGL(gcgrad_dctx_kernel, dim3((unsigned)ktf_cdiv(B, 16), (unsigned)ktf_cdiv(2 * (int64_t)D, 64)), dim3(GG_B_THREADS), 0, st, dg, (int)B, T,
                       (int)A, (int)D, lens, ctx, w1c, ldw, (double)eps, coef);
    if (dw1c || db1)
        hipLaunchKernelGGL(gcgrad_w1c_kernel, dim3((unsigned)ktf_cdiv(2 * (int64_t)D + 1, 16), (unsigned)ktf_cdiv(A, 64)), dim3(GG_B_THREADS), 0, st, dg,
                           (int)B, T, (int)A, (int)D, lens, ctx, dw1c, lddw, db1);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

template <int MODE>
static void gg_launch_data(const GcgradDataParams& p, dim3 grid, hipStream_t st) {
    KTF_LDS_ONCE(GG_LDS_DATA, gcgrad_data_kernel<MODE>);
    hipLaunchKernelGGL((gcgrad_data_kernel<MODE>), grid, dim3(GG_THREADS), GG_LDS_DATA, st, p);
}

extern "C" int ktf_gcgrad_data(const float* dz, int64_t B, int64_t T, int32_t A, int64_t ldz, const int32_t* lens, const float* w1x, int64_t ldw1,
                               int32_t D, const float* x, int64_t ldx, const double* ctx, const double* coef, int32_t gemm, int32_t accumulate,
                               float* dx, int64_t lddx, void* stream) {
    const char* who = "ktf_gcgrad_data";
    int rc = gg_check_rows(who, B, T, D);
    if (rc != KTF_OK || (rc = gg_check_shape(who, A, 1, gemm)) != KTF_OK) return rc;
    if ((rc = gg_check_ld(who, "ldz", ldz, A)) != KTF_OK || (rc = gg_check_ld(who, "ldw1", ldw1, A)) != KTF_OK ||
        (rc = gg_check_ld(who, "ldx", ldx, D)) != KTF_OK || (rc = gg_check_ld(who, "lddx", lddx, D)) != KTF_OK)
        return rc;
    KTF_REQUIRE(B * T == 0 || (dz && w1x && x && ctx && coef && dx), "%s: null dz, w1x, x, ctx, coef or dx", who);
    if (B * T == 0) return KTF_OK;

    GcgradDataParams p = {};
    p.dz = dz, p.lens = lens, p.w1 = w1x, p.x = x, p.ctx = ctx, p.coef = coef, p.dx = dx;
    p.T = T, p.ldz = ldz, p.ldw1 = ldw1, p.ldx = ldx, p.lddx = lddx;
    p.D = D, p.A = A, p.w1_vec = gg_vec(w1x, ldw1), p.accumulate = accumulate != 0;
    const dim3 grid((unsigned)ktf_cdiv(T, GG_R), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (gemm == KTF_GEMM_F32) gg_launch_data<KTF_GEMM_F32>(p, grid, st);
    else gg_launch_data<KTF_GEMM_BF16X3>(p, grid, st);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
