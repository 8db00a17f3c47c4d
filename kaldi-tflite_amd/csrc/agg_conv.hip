// Multi-layer feature aggregation in one launch (include/ktf_agg.h states the contract as numbered rules, INTEGRATION.md section 2u the
// use, DESIGN.md section 7 the design and the measurements): a GEMM whose K axis walks the channels of S tensors, each with a base
// pointer and a leading dimension of its own, against one (units, K) weight matrix read as it stands. The concatenation is never formed.
//
// Work split. A workgroup of four waves owns AG_R = 128 rows [t0, t0 + 128) of one utterance and AG_NT = 128 units; a wave owns a
// 64 x 64 quadrant, sixteen 16 x 16 accumulators held in registers for the whole of K. The grid's x index is (row tile, N-tile) with the
// N-tile fastest: the workgroups that share a row tile are neighbours in launch order, so the source rows they all read stay in L2.
// A tile at or beyond len_b exits at once (rule 3: an empty utterance has no tile that runs).
//
// K-loop. One flat loop over the K / 32 chunks of the concatenation; only the FEED knows about sources. The feed runs one chunk ahead of
// the matrix instructions through a ring of two 32 KiB stages (A: 128 rows x 32 fp32 | W: 128 units x 32 fp32), 16 bytes per lane by
// global_load_lds DMAs: four for A and four for W per lane and chunk, no VGPR round trip. A lane keeps one 64-bit pointer per DMA;
// within a source it advances by 32 floats, and when the feed crosses into the next source the four A pointers are rebuilt from that
// source's wave-uniform base and stride (at most three times per tile) -- the W pointers never notice, as w is laid out in
// concatenation order. Rows are clamped to len_b - 1 where they are READ (never to T), units to units - 1; what such rows and units
// compute is never stored. A source or a weight matrix whose base is not 16-byte aligned is fed by scalar loads and one LDS store into
// the same image (wave-uniform choice per source); the bits are the same. One barrier per chunk: it says both "chunk k has landed" and
// "everyone has finished reading the stage chunk k + 1 goes into".
//
// LDS image. Rows of 128 bytes, eight 16-byte pieces; LDS piece p of row r holds global piece p ^ ((r >> 1) & 7), so the sixteen rows a
// fragment read touches fall on sixteen disjoint sets of four banks although the DMA image cannot be padded (a wave's DMA writes 1 KiB
// lane-linear). The W image is also PERMUTED by rows: LDS row 64 wn + 16 cb + m holds unit n0 + 64 wn + 4 m + cb, which makes a lane's
// sixteen outputs of a row sixteen CONSECUTIVE units (below) while its fragment reads stay on consecutive LDS rows.
//
// Matrix instructions. As in res2_conv.hip the blocks are transposed: W is the first operand (M = unit), the rows are the second
// (N = row), so lane (n = lane & 15, h = lane >> 4) of block (rb, cb) holds row 16 rb + n and the units 4 (4 h + i) + cb, i = 0 .. 3: over
// cb = 0 .. 3 that is the run of sixteen units from 16 h -- four 16-byte stores per row and lane, 256 contiguous bytes per row and wave.
// Lane group h supplies the reduction elements 32 chunk + 8 h .. + 7 of either operand in every mode (two 16-byte LDS reads): F32 feeds
// them to eight v_mfma_f32_16x16x4_f32, the 16-bit modes round or split them in registers (r2_split8) into one / three
// v_mfma_f32_16x16x32_bf16.
#include "res2_common.h"
#include "../../include/ktf_agg.h"

#define AG_THREADS 256
#define AG_R 128
#define AG_NT 128
#define AG_HALF_BYTES 16384                      // one operand's chunk: 128 rows of 128 bytes
#define AG_STAGE_BYTES (2 * AG_HALF_BYTES)
#define AG_LDS_BYTES (2 * AG_STAGE_BYTES)

typedef __attribute__((address_space(3))) void ag_lds_ptr_t;
typedef __attribute__((address_space(1))) const void ag_glb_ptr_t;

struct AggParams {
    const float* x[KTF_AGG_MAX_SOURCES];
    int64_t ldx[KTF_AGG_MAX_SOURCES];
    int32_t nch[KTF_AGG_MAX_SOURCES];            // chunks of 32 channels per source
    int32_t x_vec[KTF_AGG_MAX_SOURCES];          // the base pointer is 16-byte aligned: DMA feed (the bits are the same without)
    const int32_t* lens;
    const float* w;
    const float* bias;
    const float* nscale;
    const float* nshift;
    float* y;
    int64_t T, ldw, ldy;
    int32_t S, nk, units, act, ntiles, w_vec, y_vec;
};

// one 16-byte piece per lane into the wave's 1 KiB of the image at `dst` (wave-uniform): DMA, or scalar loads and one LDS store
__device__ __forceinline__ void ag_feed(const float* g, unsigned char* dst, int lane, bool vec) {
    if (vec) {
        __builtin_amdgcn_global_load_lds((ag_glb_ptr_t*)g, (ag_lds_ptr_t*)dst, 16, 0, 0);
    } else {
        *reinterpret_cast<r2_fv4*>(dst + lane * 16) = r2_fv4{g[0], g[1], g[2], g[3]};
    }
}

// the lane's eight reduction elements of LDS row `row` (byte offset), pieces 2 h and 2 h + 1 under the row's swizzle `sw`
__device__ __forceinline__ void ag_frag(const unsigned char* row, int h, int sw, float (&v)[8]) {
    const r2_fv4 v0 = *reinterpret_cast<const r2_fv4*>(row + (((2 * h) ^ sw) << 4));
    const r2_fv4 v1 = *reinterpret_cast<const r2_fv4*>(row + (((2 * h + 1) ^ sw) << 4));
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = v0[i], v[4 + i] = v1[i];
}

template <int MODE>
__global__ __launch_bounds__(AG_THREADS, 2) void agg_conv_kernel(AggParams p) {
    constexpr bool X3 = MODE == KTF_GEMM_BF16X3;
    extern __shared__ __attribute__((aligned(16))) unsigned char ag_lds[];
    const int b = blockIdx.y;
    int len = p.lens ? p.lens[b] : (int)p.T;
    len = len < 0 ? 0 : (len > (int)p.T ? (int)p.T : len);
    const int tile = (int)(blockIdx.x / (unsigned)p.ntiles), nt = (int)(blockIdx.x - (unsigned)tile * (unsigned)p.ntiles);
    const int t0 = tile * AG_R, n0 = nt * AG_NT;
    if (t0 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int n = lane & 15, h = lane >> 4;

    // ---- the feed: DMA j of wave `wave` fills LDS rows 8 (4 j + wave) .. + 7; the lane's piece is row (lane >> 3), position lane & 7
    int a_row[4];                                // the frame the lane's piece of DMA j comes from, clamped to the utterance
    unsigned f_col[4];                           // ... and its first float within the chunk, swizzled
    const float* pw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = 8 * (4 * j + wave) + (lane >> 3);
        f_col[j] = (unsigned)(((lane & 7) ^ ((r >> 1) & 7)) * 4);
        const int t = t0 + r;
        a_row[j] = t < len ? t : len - 1;
        int u = n0 + (r & 64) + 4 * (r & 15) + ((r >> 4) & 3);              // the unit LDS row r of the W image holds
        u = u < p.units ? u : p.units - 1;
        pw[j] = p.w + (int64_t)u * p.ldw + f_col[j];
    }
    const float* pa[4];
    int fs = 0, fleft = 0;                       // the source the feed is in and the chunks it has left there (wave-uniform)
    bool fvec = false;
    const bool wvec = p.w_vec;
    auto feed = [&](int stage) {
        if (fleft == 0) {                        // into the next source: a wave-uniform base and stride, four pointers rebuilt
            const float* xb = p.x[fs] + (int64_t)b * p.T * p.ldx[fs];
#pragma unroll
            for (int j = 0; j < 4; ++j) pa[j] = xb + (int64_t)a_row[j] * p.ldx[fs] + f_col[j];
            fleft = p.nch[fs];
            fvec = p.x_vec[fs];
            ++fs;
        }
        unsigned char* st = ag_lds + stage * AG_STAGE_BYTES + wave * 1024;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ag_feed(pa[j], st + j * 4096, lane, fvec);
            ag_feed(pw[j], st + AG_HALF_BYTES + j * 4096, lane, wvec);
            pa[j] += 32;
            pw[j] += 32;
        }
        --fleft;
    };

    f32x4 acc[4][4];                             // [rb][cb]
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[rb][cb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int sw = (n >> 1) & 7;                 // (every fragment row is 16 k + n: the swizzle of row n)
    const int a_off = (wm * 64 + n) * 128, w_off = AG_HALF_BYTES + (wn * 64 + n) * 128;
    const int nk = p.nk;
    feed(0);
    for (int k = 0; k < nk; ++k) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // chunk k has landed (nothing else is in flight)
        __syncthreads();
        if (k + 1 < nk) feed((k + 1) & 1);                     // chunk k + 1 -> the stage every wave has finished reading
        const unsigned char* st = ag_lds + (k & 1) * AG_STAGE_BYTES;
        float a[4][8], bw[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ag_frag(st + a_off + i * 2048, h, sw, a[i]);
            ag_frag(st + w_off + i * 2048, h, sw, bw[i]);
        }
        if constexpr (MODE == KTF_GEMM_F32) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb) acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(bw[cb][e], a[rb][e], acc[rb][cb], 0, 0, 0);
        } else {
            r2_bfrag8 ah[4], al[4];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) r2_split8<X3>(a[rb], ah[rb], al[rb]);
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                r2_bfrag8 bh, bl;
                r2_split8<X3>(bw[cb], bh, bl);
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) {
                    acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, ah[rb], acc[rb][cb], 0, 0, 0);
                    if (X3) {
                        acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, al[rb], acc[rb][cb], 0, 0, 0);
                        acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl, ah[rb], acc[rb][cb], 0, 0, 0);
                    }
                }
            }
        }
    }

    // ---- epilogue: bias -> act -> scale / shift; the lane's sixteen consecutive units from u0 of row t, element 4 i + cb = acc[rb][cb][i]
    const int u0 = n0 + wn * 64 + 16 * h;
    float* yb = p.y + (int64_t)b * p.T * p.ldy;
    const bool yv = p.y_vec;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        const int t = t0 + wm * 64 + rb * 16 + n;
        if (t >= len) continue;                                // (rule 2; such a lane computed a copy of row len_b - 1)
        float* yr = yb + (int64_t)t * p.ldy;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = u0 + 4 * i;
            if (u >= p.units) continue;                        // (rule 2; such a lane computed a copy of unit units - 1)
            r2_fv4 v;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const int uc = u + cb < p.units ? u + cb : p.units - 1;
                float z = acc[rb][cb][i];
                if (p.bias) z += p.bias[uc];
                if (p.act == KTF_ACT_RELU) z = z < 0.0f ? 0.0f : z;
                if (p.nscale) z = __fadd_rn(__fmul_rn(z, p.nscale[uc]), p.nshift[uc]);
                v[cb] = z;
            }
            if (u + 4 <= p.units) {
                r2_store4(yr + u, v, yv);
            } else {
#pragma unroll
                for (int cb = 0; cb < 3; ++cb)
                    if (u + cb < p.units) yr[u + cb] = v[cb];
            }
        }
    }
}

// ------------------------------------------------------------------------------------ host
static int ag_check_shape(const char* who, int32_t units, int32_t K, int32_t gemm) {
    KTF_REQUIRE(units >= 1 && units <= KTF_AGG_MAX_UNITS, "%s: units %d outside [1, %d]", who, (int)units, KTF_AGG_MAX_UNITS);
    KTF_REQUIRE(K >= 64 && K <= KTF_AGG_MAX_SOURCES * KTF_AGG_MAX_WIDTH && K % 32 == 0, "%s: K %d is not a multiple of 32 in [64, %d]", who, (int)K,
                KTF_AGG_MAX_SOURCES * KTF_AGG_MAX_WIDTH);
    KTF_REQUIRE(gemm == KTF_GEMM_F32 || gemm == KTF_GEMM_BF16 || gemm == KTF_GEMM_BF16X3, "%s: gemm %d is not KTF_GEMM_F32, _BF16 or _BF16X3", who,
                (int)gemm);
    return KTF_OK;
}

extern "C" int32_t ktf_agg_row_tile(int32_t units, int32_t K, int32_t gemm) {
    if (int rc = ag_check_shape("ktf_agg_row_tile", units, K, gemm)) return rc;
    return AG_R;                                               // (one tile shape serves every width: the ring holds chunks, not rows of K)
}

template <int MODE>
static void ag_launch(const AggParams& p, dim3 grid, hipStream_t st) {
    KTF_LDS_ONCE(AG_LDS_BYTES, agg_conv_kernel<MODE>);
    hipLaunchKernelGGL(agg_conv_kernel<MODE>, grid, dim3(AG_THREADS), AG_LDS_BYTES, st, p);
}

extern "C" int ktf_agg_conv(const float* const* xs, const int32_t* widths, const int64_t* ldxs, int32_t S, int64_t B, int64_t T, const int32_t* lens,
                            const float* w, int64_t ldw, const float* bias, const float* nscale, const float* nshift, int32_t units, int32_t act,
                            int32_t gemm, float* y, int64_t ldy, void* stream) {
    const char* who = "ktf_agg_conv";
    KTF_REQUIRE(S >= 2 && S <= KTF_AGG_MAX_SOURCES, "%s: %d sources, outside [2, %d]", who, (int)S, KTF_AGG_MAX_SOURCES);
    KTF_REQUIRE(B >= 0 && T >= 0, "%s: negative size (B %lld, T %lld)", who, (long long)B, (long long)T);
    KTF_REQUIRE(B <= KTF_AGG_MAX_BATCH && T <= KTF_AGG_MAX_ROWS, "%s: B %lld above %d or T %lld above %d", who, (long long)B, KTF_AGG_MAX_BATCH,
                (long long)T, KTF_AGG_MAX_ROWS);
    KTF_REQUIRE(widths && ldxs, "%s: null source table", who);
    int32_t K = 0;
    for (int s = 0; s < S; ++s) {
        KTF_REQUIRE(widths[s] >= 32 && widths[s] <= KTF_AGG_MAX_WIDTH && widths[s] % 32 == 0, "%s: source %d has %d channels, not a multiple of 32 in [32, %d]",
                    who, s, (int)widths[s], KTF_AGG_MAX_WIDTH);
        KTF_REQUIRE(ldxs[s] >= widths[s] && ldxs[s] % 4 == 0 && ldxs[s] < (1ll << 31), "%s: ldx of source %d (%lld) below its %d channels, not a multiple of 4 or at 2^31",
                    who, s, (long long)ldxs[s], (int)widths[s]);
        K += widths[s];
    }
    if (int rc = ag_check_shape(who, units, K, gemm)) return rc;
    KTF_REQUIRE(ldw >= K && ldw % 4 == 0 && ldw < (1ll << 31), "%s: ldw %lld below K %d, not a multiple of 4 or at 2^31", who, (long long)ldw, (int)K);
    KTF_REQUIRE(ldy >= units && ldy % 4 == 0 && ldy < (1ll << 31), "%s: ldy %lld below units %d, not a multiple of 4 or at 2^31", who, (long long)ldy,
                (int)units);
    KTF_REQUIRE((nscale == nullptr) == (nshift == nullptr), "%s: nscale and nshift go together", who);
    KTF_REQUIRE(act == KTF_ACT_NONE || act == KTF_ACT_RELU, "%s: act %d is not KTF_ACT_NONE or KTF_ACT_RELU", who, (int)act);
    const int64_t rows = B * T;                                // < 2^46
    KTF_REQUIRE(rows == 0 || (xs && w && y), "%s: null xs, w or y", who);
    int64_t ny = 0;
    KTF_REQUIRE(!__builtin_mul_overflow(rows, ldy, &ny) && ny < (1ll << 60), "%s: B * T * ldy reaches 2^60", who);
    for (int s = 0; s < S; ++s) {
        int64_t nx = 0;
        KTF_REQUIRE(!__builtin_mul_overflow(rows, ldxs[s], &nx) && nx < (1ll << 60), "%s: B * T * ldx of source %d reaches 2^60", who, s);
        if (rows == 0) continue;
        KTF_REQUIRE(xs[s] != nullptr, "%s: null source %d", who, s);
        const uintptr_t x0 = (uintptr_t)xs[s], y0 = (uintptr_t)y;
        const uintptr_t xn = (uintptr_t)(nx - ldxs[s] + widths[s]) * 4, yn = (uintptr_t)ny * 4;
        KTF_REQUIRE(!(x0 < y0 + yn && y0 < x0 + xn), "%s: y overlaps source %d", who, s);
    }
    if (rows == 0) return KTF_OK;

    AggParams p = {};
    for (int s = 0; s < S; ++s) {
        p.x[s] = xs[s];
        p.ldx[s] = ldxs[s];
        p.nch[s] = widths[s] / 32;
        p.x_vec[s] = ((uintptr_t)xs[s] & 15) == 0;
    }
    p.lens = lens, p.w = w, p.bias = bias, p.nscale = nscale, p.nshift = nshift, p.y = y;
    p.T = T, p.ldw = ldw, p.ldy = ldy;
    p.S = S, p.nk = K / 32, p.units = units, p.act = act, p.ntiles = ktf_cdiv(units, AG_NT);
    p.w_vec = ((uintptr_t)w & 15) == 0, p.y_vec = ((uintptr_t)y & 15) == 0;
    const dim3 grid((unsigned)(ktf_cdiv(T, AG_R) * (int64_t)p.ntiles), (unsigned)B);      // <= 2^23 * 64
    hipStream_t st = (hipStream_t)stream;
    if (gemm == KTF_GEMM_F32) ag_launch<KTF_GEMM_F32>(p, grid, st);
    else if (gemm == KTF_GEMM_BF16) ag_launch<KTF_GEMM_BF16>(p, grid, st);
    else ag_launch<KTF_GEMM_BF16X3>(p, grid, st);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
