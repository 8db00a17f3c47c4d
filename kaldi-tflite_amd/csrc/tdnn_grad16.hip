// The TDNN gradients on the 16-bit matrix pipe (include/ktf_grad.h rules 6-8): the counterparts of grad_dx_kernel / grad_dw_kernel of
// tdnn_grad.hip on v_mfma_f32_32x32x16_bf16, in a one-pass bf16 mode and a three-pass split-bf16 mode (X3: hi.hi + lo.hi + hi.lo). Same
// decomposition, same workspace, same fold and reduce kernels (tdnn_grad_common.h); no atomics.
//
//   ktf_grad_tdnn16_data     grad_fold_kernel  -> grad16_dx_kernel       dx = gather(g) * W
//   ktf_grad_tdnn16_weights  grad16_dw_kernel  -> grad_dw_reduce_kernel  dW = g^T * gather(x), dbias = column sums of the fp32 g
//
// The operands arrive as fp32 and are rounded in registers on the way to LDS (v_cvt_pk_bf16_f32: nearest even). Both GEMMs are
// register-staged, double-buffered LDS tiles of four waves (2 x 2), K-step 32 = two MFMAs deep. An LDS image is [tile row][K] bf16 with
// rows of 40 elements (80 bytes: the 16 lanes of a ds_read_b128 group fall on 16 disjoint sets of four banks); lane l reads the 8
// consecutive K of row l & 31 at K = 8 (l >> 5) as one 16-byte fragment. X3 keeps a second image of the lo parts. Operands whose K
// index is the row axis in memory (W for dx, g and x for dW) are transposed in registers: a thread owns ONE tile row (lanes = consecutive
// columns in memory: every 4-byte load of a wave is one contiguous 256 bytes) and loads 8 or 16 consecutive K of it, which the
// conversion packs pairwise into 16-byte stores -- so the conversion's pairing IS the transpose. (A thread that loaded 16 bytes of
// four rows instead would store to rows 4 apart: 320 bytes, two banks for a whole wave. ds_read_b64_tr_b16 on a K-major image would
// save nothing here: an image is written once and read by two waves, and the 16-byte fragment read of the row-major image is the
// cheaper read.)
#include "tdnn_grad_common.h"

#define G16_BK 32
#define G16_PITCH 40

__device__ __forceinline__ unsigned g16_pack(float a, float b) { return (unsigned)f2bf(a) | ((unsigned)f2bf(b) << 16); }

// 8 consecutive K of one LDS row (16 bytes): hi = bf16(v) to `hi`; X3: lo = bf16(v - hi) to `lo`
template <bool X3>
__device__ __forceinline__ void g16_put8(unsigned short* hi, unsigned short* lo, const float* v) {
    unsigned h[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h[i] = g16_pack(v[2 * i], v[2 * i + 1]);
        l[i] = X3 ? g16_pack(v[2 * i] - bf2f((unsigned short)(h[i] & 0xffffu)), v[2 * i + 1] - bf2f((unsigned short)(h[i] >> 16))) : 0u;
    }
    *reinterpret_cast<u32x4*>(hi) = u32x4{h[0], h[1], h[2], h[3]};
    if (X3) *reinterpret_cast<u32x4*>(lo) = u32x4{l[0], l[1], l[2], l[3]};
}

// Four consecutive units u .. u + 3 of a g row (`row` = its first element); units at or beyond `units` are 0 and not read. `vec`: g
// and ldg allow 16-byte loads.
__device__ __forceinline__ fv4 g16_load_g(const float* row, int u, int units, bool vec) {
    if (vec && u + 4 <= units) return *reinterpret_cast<const fv4*>(row + u);
    fv4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = u + e < units ? row[u + e] : 0.0f;
    return v;
}

// A transposed operand tile of G16_BK K-rows x C tile rows: thread -> tile row col() and the KPT consecutive K from k0()
template <int C>
struct G16Tr {
    static constexpr int KPT = G16_BK * C / GR_THREADS;
    static_assert(C == 64 || C == 128, "256 threads cover 32 x C, 8 or 16 K each");
    static __device__ __forceinline__ int col(int tid) { return tid % C; }
    static __device__ __forceinline__ int k0(int tid) { return (tid / C) * KPT; }
    template <bool X3>
    static __device__ __forceinline__ void store(unsigned short* hi, unsigned short* lo, const float (&r)[KPT], int tid) {
        const int at = col(tid) * G16_PITCH + k0(tid);
#pragma unroll
        for (int q = 0; q < KPT; q += 8) g16_put8<X3>(hi + at + q, lo + at + q, r + q);
    }
};

// The main loop: wave (wm, wn) owns MTM x MTN blocks of 32 x 32. As / Bs: [stage][plane][(64 MTM) / (64 MTN) rows of G16_PITCH].
// load_global(ks) fetches step ks into the caller's registers, store_lds(buf) converts and writes them to stage buf. nk >= 1.
// NST = 2: two stages, one barrier per step. NST = 1: one stage and a second barrier per step (the loads of the next step still fly
// under the MFMAs): X3's two images per operand then take the LDS of the one-pass mode's two stages, and as many workgroups fit a CU.
template <int MTM, int MTN, bool X3, int NST, typename LoadGlobal, typename StoreLds>
__device__ __forceinline__ void g16_mainloop(f32x16 (&acc)[MTM][MTN], const unsigned short* As, const unsigned short* Bs, int nk, int wm, int wn,
                                             int lane, LoadGlobal&& load_global, StoreLds&& store_lds) {
    constexpr int NPL = X3 ? 2 : 1, APL = 64 * MTM * G16_PITCH, BPL = 64 * MTN * G16_PITCH;
#pragma unroll
    for (int i = 0; i < MTM; ++i)
#pragma unroll
        for (int j = 0; j < MTN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    load_global(0);
    if (NST == 2) {
        store_lds(0);
        __syncthreads();
    }
    for (int ks = 0; ks < nk; ++ks) {
        const int buf = NST == 2 ? ks & 1 : 0;
        if (NST == 1) {
            store_lds(0);
            __syncthreads();
        }
        if (ks + 1 < nk) load_global(ks + 1);
        const unsigned short* a_base = As + buf * NPL * APL + (wm * 32 * MTM + (lane & 31)) * G16_PITCH + 8 * (lane >> 5);
        const unsigned short* b_base = Bs + buf * NPL * BPL + (wn * 32 * MTN + (lane & 31)) * G16_PITCH + 8 * (lane >> 5);
#pragma unroll
        for (int kk = 0; kk < G16_BK; kk += 16) {
            bfrag8 ah[MTM], bh[MTN], al[MTM], bl[MTN];
#pragma unroll
            for (int i = 0; i < MTM; ++i) {
                ah[i] = *reinterpret_cast<const bfrag8*>(a_base + i * 32 * G16_PITCH + kk);
                if (X3) al[i] = *reinterpret_cast<const bfrag8*>(a_base + APL + i * 32 * G16_PITCH + kk);
            }
#pragma unroll
            for (int j = 0; j < MTN; ++j) {
                bh[j] = *reinterpret_cast<const bfrag8*>(b_base + j * 32 * G16_PITCH + kk);
                if (X3) bl[j] = *reinterpret_cast<const bfrag8*>(b_base + BPL + j * 32 * G16_PITCH + kk);
            }
#pragma unroll
            for (int i = 0; i < MTM; ++i)
#pragma unroll
                for (int j = 0; j < MTN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                    if (X3) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                    }
                }
        }
        if (NST == 2 && ks + 1 < nk) store_lds(buf ^ 1);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------ data gradient
// dx tile: 64 input rows x 128 features of one utterance; reduction over (context k, unit u) in steps of 32 units: a = g row of the
// input row (as grad_dx_kernel finds it), b = W as stored, transposed on the way. X3: rows 0 and len - 1 add the folded rows (fp32 sums
// of the fp32 g) before the split, as the fp32 kernel does before its product. One-pass mode: the fold (fp32 sums of the ROUNDED g) is
// not a bf16 number; the tiles that hold row 0 or len - 1 run it as a hi / lo pair in K-steps of their own behind the main ones, over
// the contexts that can clamp at their edge (negative offsets at row 0, positive ones at len - 1; none with VALID padding).
template <bool X3>
__global__ __launch_bounds__(GR_THREADS) void grad16_dx_kernel(GradParams p) {
    constexpr int BM = KTF_GRAD_ROW_TILE, BN = 128, NPL = X3 ? 2 : 1, NST = X3 ? 1 : 2;
    using TB = G16Tr<BN>;
    __shared__ __attribute__((aligned(16))) unsigned short As[NST * NPL * BM * G16_PITCH];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[NST * NPL * BN * G16_PITCH];
    const int b = blockIdx.z;
    const int T = (int)p.f.T;
    const int len = grad_len(p, b);
    int start;
    const int out_len = tdnn_out_len(len, p.f, start);
    const int r0 = blockIdx.y * BM, d0 = blockIdx.x * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    float* dxb = p.dx + (int64_t)b * T * p.f.ldx;
    if (r0 >= len || d0 >= p.f.din_pad) {            // nothing but zeros: rows past the utterance, or the columns [din_pad, ldx)
        for (int q = tid; q < BM * BN; q += GR_THREADS) {
            const int r = r0 + q / BN, d = d0 + q % BN;
            if (r < T && d < p.f.ldx) dxb[(int64_t)r * p.f.ldx + d] = 0.0f;
        }
        return;
    }
    const float* gb = p.g + (int64_t)b * p.f.Tout * p.ldg;
    const float* fold_lo = p.fold + ((int64_t)b * 2 + 0) * p.f.nctx * p.f.units;
    const float* fold_hi = p.fold + ((int64_t)b * 2 + 1) * p.f.nctx * p.f.units;
    const bool gvec = ((reinterpret_cast<uintptr_t>(p.g) & 15) | (p.ldg & 3)) == 0;

    const int a_row = tid >> 2, a_col = (tid & 3) * 8;           // A: 64 rows x 32 units, 8 consecutive units per thread
    const int r = r0 + a_row;
    const bool first = r == 0, last = r == len - 1;

    const int nu = (p.f.units + G16_BK - 1) / G16_BK;            // W has round_up(units, 256) rows: a step past `units` reads its zero rows
    const int nk_main = p.f.nctx * nu;
    int klo = 0, khi = 0;                                        // contexts of the fold steps (one-pass mode)
    if (!X3 && !p.f.valid) {
        int nneg = 0, npos = 0;
        for (int k = 0; k < p.f.nctx; ++k) nneg += p.f.ctx[k] < 0, npos += p.f.ctx[k] > 0;
        const bool has_first = r0 == 0, has_last = len - 1 < r0 + BM;       // (r0 < len)
        klo = has_first && nneg > 0 ? 0 : p.f.nctx - npos;     // the offsets ascend: [0, nneg) clamp at row 0, [nctx - npos, nctx) at len - 1
        khi = has_last && npos > 0 ? p.f.nctx : nneg;          // (an empty range where the tile holds neither row)
    }
    const int nfs = khi > klo ? (khi - klo) * nu : 0;
    const int nk = nk_main + 2 * nfs;

    f32x16 acc[1][2];
    fv4 ra[2];
    float rb[TB::KPT];

    auto load_global = [&](int ks) {
        int pass = -1, kk = ks;                                  // pass: -1 a main step, 0 / 1 the hi / lo half of the folded rows
        if (ks >= nk_main) {
            pass = (ks - nk_main) / nfs;
            kk = klo * nu + (ks - nk_main - pass * nfs);
        }
        const int k = kk / nu;
        const int u0 = (kk - k * nu) * G16_BK;
        const int off = p.f.ctx[k];
        const int s = r - start - off;
        const int t = s / p.f.sub;
        const bool hit = r < len && s >= 0 && t * p.f.sub == s && t < out_len;
        const float* gr = gb + (int64_t)(hit ? t : 0) * p.ldg;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int u = u0 + a_col + 4 * h;
            fv4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if ((X3 || pass < 0) && hit) v = g16_load_g(gr, u, p.f.units, gvec);
            if (X3 || pass >= 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (u + e < p.f.units) {
                        if (first) v[e] += fold_lo[k * p.f.units + u + e];
                        if (last) v[e] += fold_hi[k * p.f.units + u + e];
                    }
            }
            if (pass == 1) {                                     // the lo half: f - bf16(f), rounded to bf16 by the store
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] -= bf2f(f2bf(v[e]));
            }
            ra[h] = v;
        }
        const int d = d0 + TB::col(tid);
        const float* wc = reinterpret_cast<const float*>(p.f.w) + (int64_t)(u0 + TB::k0(tid)) * p.f.ktot + (int64_t)k * p.f.din_pad + d;
#pragma unroll
        for (int i = 0; i < TB::KPT; ++i) rb[i] = d < p.f.din_pad ? wc[(int64_t)i * p.f.ktot] : 0.0f;
    };
    auto store_lds = [&](int buf) {
        const float v[8] = {ra[0][0], ra[0][1], ra[0][2], ra[0][3], ra[1][0], ra[1][1], ra[1][2], ra[1][3]};
        unsigned short* a = As + buf * NPL * BM * G16_PITCH + a_row * G16_PITCH + a_col;
        g16_put8<X3>(a, a + BM * G16_PITCH, v);
        unsigned short* bb = Bs + buf * NPL * BN * G16_PITCH;
        TB::template store<X3>(bb, bb + BN * G16_PITCH, rb, tid);
    };

    g16_mainloop<1, 2, X3, NST>(acc, As, Bs, nk, wm, wn, lane, load_global, store_lds);

    // accumulator layout: column = lane & 31, row = acc32_row(0, reg, lane)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int d = d0 + wn * 64 + j * 32 + (lane & 31);
        if (d >= p.f.ldx) continue;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int rr = acc32_row(r0 + wm * 32, reg, lane);
            if (rr < T) dxb[(int64_t)rr * p.f.ldx + d] = (rr < len && d < p.din) ? acc[0][j][reg] : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------ weight and bias gradient
// One workgroup = 128 units x 128 features of ONE context x one slot of KTF_GRAD_SLOT_ROWS flat rows m = b * Tout + t, reduced in
// steps of 32 rows: a = g[m, unit], b = x[b, row(t, k), feature], both transposed on the way. The x row of every flat row of the slot
// (-1: the row stands for nothing) is worked out once, into LDS. The tile goes to the slot's own copy of dW. The workgroups of the
// first feature tile (blockIdx.x == 0) also add up the fp32 g they stage, before it is rounded: a thread sums its unit over its 16
// rows of every step in row order, and the two row groups are added at the end.
template <bool X3>
__global__ __launch_bounds__(GR_THREADS) void grad16_dw_kernel(GradParams p) {
    constexpr int MTN = 2, BM = 128, BN = 64 * MTN, NPL = X3 ? 2 : 1, NST = X3 ? 1 : 2;
    using TA = G16Tr<BM>;
    using TB = G16Tr<BN>;
    __shared__ __attribute__((aligned(16))) unsigned short As[NST * NPL * BM * G16_PITCH];
    __shared__ __attribute__((aligned(16))) unsigned short Bs[NST * NPL * BN * G16_PITCH];
    __shared__ int64_t xrow[KTF_GRAD_SLOT_ROWS];
    static_assert(sizeof(As) >= (GR_THREADS / BM) * BM * sizeof(float), "the bias partials reuse As");
    static_assert(KTF_GRAD_SLOT_ROWS % G16_BK == 0, "a step past the slot's rows stays inside xrow");
    const int dtiles = (p.f.din_pad + BN - 1) / BN;
    const int k = blockIdx.x / dtiles;
    const int d0 = (blockIdx.x - k * dtiles) * BN;
    const int u0 = blockIdx.y * BM;
    const int slot = blockIdx.z;
    const int m0 = slot * KTF_GRAD_SLOT_ROWS;
    const int m1 = m0 + KTF_GRAD_SLOT_ROWS < p.rows ? m0 + KTF_GRAD_SLOT_ROWS : p.rows;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int Tout = (int)p.f.Tout;
    const int off = p.f.ctx[k];
    const bool with_bias = blockIdx.x == 0;

    for (int i = tid; i < KTF_GRAD_SLOT_ROWS; i += GR_THREADS) {
        const int m = m0 + i;
        int64_t xr = -1;
        if (m < m1) {
            const int b = m / Tout, t = m - b * Tout;
            const int len = grad_len(p, b);
            int start;
            if (t < tdnn_out_len(len, p.f, start)) {
                int r = start + t * p.f.sub + off;
                r = r < 0 ? 0 : (r > len - 1 ? len - 1 : r);
                xr = (int64_t)b * p.f.T + r;
            }
        }
        xrow[i] = xr;
    }
    __syncthreads();

    f32x16 acc[2][MTN];
    float bsum = 0.0f;
    const int nk = (m1 - m0 + G16_BK - 1) / G16_BK;
    float ra[TA::KPT], rb[TB::KPT];
    const int ua = u0 + TA::col(tid), db = d0 + TB::col(tid);

    auto load_global = [&](int ks) {
#pragma unroll
        for (int i = 0; i < TA::KPT; ++i) {
            const int mi = ks * G16_BK + TA::k0(tid) + i;
            ra[i] = (xrow[mi] >= 0 && ua < p.f.units) ? p.g[(int64_t)(m0 + mi) * p.ldg + ua] : 0.0f;
            bsum += ra[i];
        }
#pragma unroll
        for (int i = 0; i < TB::KPT; ++i) {
            const int64_t xr = xrow[ks * G16_BK + TB::k0(tid) + i];
            rb[i] = (xr >= 0 && db < p.f.din_pad) ? reinterpret_cast<const float*>(p.f.x)[xr * p.f.ldx + db] : 0.0f;
        }
    };
    auto store_lds = [&](int buf) {
        unsigned short* a = As + buf * NPL * BM * G16_PITCH;
        TA::template store<X3>(a, a + BM * G16_PITCH, ra, tid);
        unsigned short* bb = Bs + buf * NPL * BN * G16_PITCH;
        TB::template store<X3>(bb, bb + BN * G16_PITCH, rb, tid);
    };

    // (nk >= 1: the grid has one z per slot that holds a row, so m0 < p.rows)
    g16_mainloop<2, MTN, X3, NST>(acc, As, Bs, nk, wm, wn, lane, load_global, store_lds);

    float* ws = p.slots + (int64_t)slot * p.slot_stride;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < MTN; ++j) {
            const int d = d0 + wn * 32 * MTN + j * 32 + (lane & 31);
            if (d >= p.f.din_pad) continue;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int u = acc32_row(u0 + wm * 64 + i * 32, reg, lane);
                if (u < p.units_pad) ws[(int64_t)u * p.f.ktot + (int64_t)k * p.f.din_pad + d] = acc[i][j][reg];
            }
        }
    if (with_bias) {                                             // (the main loop's last barrier is behind every read of As)
        float* red = reinterpret_cast<float*>(As);               // [row group][unit of the tile]
        red[tid] = bsum;                                         // tid = row group * BM + unit
        __syncthreads();
        if (tid < BM && u0 + tid < p.units_pad) {
            float v = 0.0f;
#pragma unroll
            for (int q = 0; q < GR_THREADS / BM; ++q) v += red[q * BM + tid];
            ws[(int64_t)p.units_pad * p.f.ktot + u0 + tid] = v;
        }
    }
}

// ------------------------------------------------------------------------------------ entry points
static int grad16_check(const KtfTdnnDesc* d, int32_t gemm, const char* who) {
    if (int rc = grad_check_desc(d, who)) return rc;
    KTF_REQUIRE(gemm == KTF_GEMM_BF16 || gemm == KTF_GEMM_BF16X3, "%s: gemm %d: the 16-bit gradients run as KTF_GEMM_BF16 or KTF_GEMM_BF16X3", who,
                gemm);
    return KTF_OK;
}

extern "C" int64_t ktf_grad_tdnn16_workspace_bytes(int64_t B, int64_t T, const KtfTdnnDesc* d, int32_t gemm) {
    const char* who = "ktf_grad_tdnn16_workspace_bytes";
    if (int rc = grad16_check(d, gemm, who)) return rc;
    GradSizes s;
    if (int rc = grad_sizes(B, T, d, who, &s)) return rc;
    return s.bytes;
}

extern "C" int ktf_grad_tdnn16_data(const float* g, int64_t ldg, int64_t B, int64_t T, const int32_t* lens, const KtfTdnnDesc* d, const float* w,
                                    float* dx, int64_t ldx, void* workspace, size_t workspace_bytes, int32_t gemm, void* stream) {
    const char* who = "ktf_grad_tdnn16_data";
    if (int rc = grad16_check(d, gemm, who)) return rc;
    GradSizes s;
    if (int rc = grad_check_args(who, g, w, dx, workspace, workspace_bytes, B, T, d, ldx, ldg, w, dx, "w and dx", &s)) return rc;
    if (B == 0 || T == 0) return KTF_OK;
    GradParams p;
    grad_fill(p, s, B, T, lens, d, nullptr, ldx, w, g, ldg, workspace);
    p.dx = dx;
    hipStream_t st = (hipStream_t)stream;
    const bool x3 = gemm == KTF_GEMM_BF16X3;
    const dim3 fold_grid((unsigned)ktf_cdiv(B * 2 * d->nctx * d->units, GR_THREADS));
    if (x3) hipLaunchKernelGGL(grad_fold_kernel<false>, fold_grid, dim3(GR_THREADS), 0, st, p);
    else hipLaunchKernelGGL(grad_fold_kernel<true>, fold_grid, dim3(GR_THREADS), 0, st, p);
    KTF_CHECK_LAUNCH(who);
    const dim3 grid((unsigned)ktf_cdiv(ldx, 128), (unsigned)ktf_cdiv(T, KTF_GRAD_ROW_TILE), (unsigned)B);
    if (x3) hipLaunchKernelGGL(grad16_dx_kernel<true>, grid, dim3(GR_THREADS), 0, st, p);
    else hipLaunchKernelGGL(grad16_dx_kernel<false>, grid, dim3(GR_THREADS), 0, st, p);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_grad_tdnn16_weights(const float* x, int64_t B, int64_t T, int64_t ldx, const int32_t* lens, const KtfTdnnDesc* d, const float* g,
                                       int64_t ldg, float* dw, float* dbias, void* workspace, size_t workspace_bytes, int32_t gemm, void* stream) {
    const char* who = "ktf_grad_tdnn16_weights";
    if (int rc = grad16_check(d, gemm, who)) return rc;
    GradSizes s;
    if (int rc = grad_check_args(who, x, g, dw, workspace, workspace_bytes, B, T, d, ldx, ldg, x, dw, "x and dw", &s)) return rc;
    GradParams p;
    grad_fill(p, s, B, T, lens, d, x, ldx, nullptr, g, ldg, workspace);
    hipStream_t st = (hipStream_t)stream;
    if (s.nslots > 0) {
        const dim3 grid((unsigned)(d->nctx * ktf_cdiv(d->din_pad, 128)), (unsigned)ktf_cdiv(d->units, 128), (unsigned)s.nslots);
        if (gemm == KTF_GEMM_BF16X3) hipLaunchKernelGGL(grad16_dw_kernel<true>, grid, dim3(GR_THREADS), 0, st, p);
        else hipLaunchKernelGGL(grad16_dw_kernel<false>, grid, dim3(GR_THREADS), 0, st, p);
        KTF_CHECK_LAUNCH(who);
    }
    grad_launch_reduce(p, s, d, dw, dbias, st);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
