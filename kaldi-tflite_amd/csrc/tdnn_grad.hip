// Gradients of the trainable path (include/ktf_grad.h): the data and the weight / bias gradient of ktf_tdnn with KTF_GEMM_F32 and no
// activation, and the gradient of the reducing statistics pooling. Products and their accumulation run on v_mfma_f32_32x32x2_f32 as in
// tdnn_f32.hip (an fmaf chain in reduction order); nothing here uses an atomic, so every call is reproducible bit for bit.
//
//   ktf_grad_tdnn_data     grad_fold_kernel  -> grad_dx_kernel         dx = gather(g) * W
//   ktf_grad_tdnn_weights  grad_dw_kernel    -> grad_dw_reduce_kernel  dW = g^T * gather(x), dbias = column sums of g
//   ktf_grad_stats_pool    grad_pool_kernel
//
// Both GEMMs are register-staged, double-buffered LDS tiles of four waves (2 x 2), K-step 16, rows of 17 floats (the layout of
// tdnn_f32_kernel, and its main loop: tile32_mainloop in tdnn_common.h): a wave owns MTM x MTN blocks of 32 x 32, `a` operand = the output's row index, `b` operand = its column index, so
// lanes 0-31 of a store cover 32 consecutive floats of an output row. Operand elements that stand for nothing -- rows of g at or
// beyond an utterance's output length, rows past a slot's end, columns past `units` -- are staged as 0.0f and never loaded.
// (The parameter block, the fold and reduce kernels and the entry points' checks are tdnn_grad_common.h's, shared with tdnn_grad16.hip.)
#include "tdnn_grad_common.h"

#define GR_BK 16
#define GR_PITCH (GR_BK + 1)

// ------------------------------------------------------------------------------------ data gradient
// dx tile: (64 MTM) input rows x (64 MTN) features of one utterance; reduction over (context k, unit u) in steps of 16 units. Row r
// takes from context k the g row t = (r - start - ctx[k]) / sub when that is an integer in [0, out_len); rows 0 and len - 1 add the
// folded rows of that context. W is read as stored: (unit, k * din_pad + d).
template <int MTM, int MTN>
__global__ __launch_bounds__(GR_THREADS) void grad_dx_kernel(GradParams p) {
    constexpr int BM = 64 * MTM, BN = 64 * MTN;
    constexpr int NLA = BM / 64;                     // groups of 4 units per thread: BM rows x 4 groups
    constexpr int NLB = BN / 64;                     // float4 per thread: 16 units x BN / 4
    __shared__ float As[2][BM * GR_PITCH];
    __shared__ float Bs[2][BN * GR_PITCH];
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

    int a_row[NLA], a_col[NLA], b_row[NLB], b_col[NLB];
#pragma unroll
    for (int i = 0; i < NLA; ++i) {
        const int q = i * GR_THREADS + tid;
        a_row[i] = q >> 2;
        a_col[i] = (q & 3) * 4;
    }
#pragma unroll
    for (int i = 0; i < NLB; ++i) {
        const int q = i * GR_THREADS + tid;
        b_row[i] = q / (BN / 4);
        b_col[i] = (q % (BN / 4)) * 4;
    }

    f32x16 acc[MTM][MTN];
    const int nu = (p.f.units + GR_BK - 1) / GR_BK;  // W has round_up(units, 256) rows: a step past `units` reads its zero rows
    const int nk = p.f.nctx * nu;
    float ra[NLA][4];
    float4 rb[NLB];

    auto load_global = [&](int ks) {
        const int k = ks / nu;
        const int u0 = (ks - k * nu) * GR_BK;
        const int off = p.f.ctx[k];
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            const int r = r0 + a_row[i];
            const int s = r - start - off;
            const int t = s / p.f.sub;
            const bool hit = r < len && s >= 0 && t * p.f.sub == s && t < out_len;
            const bool first = r == 0, last = r == len - 1;
            const float* gr = gb + (int64_t)(hit ? t : 0) * p.ldg;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int u = u0 + a_col[i] + e;
                float v = 0.0f;
                if (u < p.f.units) {
                    if (hit) v = gr[u];
                    if (first) v += fold_lo[k * p.f.units + u];
                    if (last) v += fold_hi[k * p.f.units + u];
                }
                ra[i][e] = v;
            }
        }
#pragma unroll
        for (int i = 0; i < NLB; ++i) {
            const int d = d0 + b_col[i];
            rb[i] = d < p.f.din_pad ? *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.f.w) + (int64_t)(u0 + b_row[i]) * p.f.ktot +
                                                                       (int64_t)k * p.f.din_pad + d)
                                    : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            float* a = &As[buf][a_row[i] * GR_PITCH + a_col[i]];
            a[0] = ra[i][0]; a[1] = ra[i][1]; a[2] = ra[i][2]; a[3] = ra[i][3];
        }
#pragma unroll
        for (int i = 0; i < NLB; ++i) {                  // transposed: Bs[feature][unit of the step]
            float* bb = &Bs[buf][b_col[i] * GR_PITCH + b_row[i]];
            bb[0] = rb[i].x; bb[GR_PITCH] = rb[i].y; bb[2 * GR_PITCH] = rb[i].z; bb[3 * GR_PITCH] = rb[i].w;
        }
    };

    tile32_mainloop<MTM, MTN, GR_BK, false>(acc, &As[0][0], &Bs[0][0], nk, wm, wn, lane, load_global, store_lds, [](int) {});

    // accumulator layout: column = lane & 31, row = acc32_row(0, reg, lane)
#pragma unroll
    for (int i = 0; i < MTM; ++i)
#pragma unroll
        for (int j = 0; j < MTN; ++j) {
            const int d = d0 + wn * 32 * MTN + j * 32 + (lane & 31);
            if (d >= p.f.ldx) continue;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int r = acc32_row(r0 + wm * 32 * MTM + i * 32, reg, lane);
                if (r < T) dxb[(int64_t)r * p.f.ldx + d] = (r < len && d < p.din) ? acc[i][j][reg] : 0.0f;
            }
        }
}

// ------------------------------------------------------------------------------------ weight and bias gradient
// One workgroup = (64 MTM) units x (64 MTN) features of ONE context x one slot of KTF_GRAD_SLOT_ROWS flat rows m = b * Tout + t,
// reduced in steps of 16 rows: a = g[m, unit], b = x[b, row(t, k), feature]. The tile goes to the slot's own copy of dW; the
// workgroups of the first feature tile (blockIdx.x == 0) also add up the staged g rows, in row order, into the slot's dbias.
template <int MTM, int MTN>
__global__ __launch_bounds__(GR_THREADS) void grad_dw_kernel(GradParams p) {
    constexpr int BM = 64 * MTM, BN = 64 * MTN;
    constexpr int NLA = BM / 64;                     // groups of 4 units per thread: 16 rows x BM / 4
    constexpr int NLB = BN / 64;                     // float4 per thread: 16 rows x BN / 4
    __shared__ float As[2][BM * GR_PITCH];
    __shared__ float Bs[2][BN * GR_PITCH];
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

    int a_row[NLA], a_col[NLA], b_row[NLB], b_col[NLB];
#pragma unroll
    for (int i = 0; i < NLA; ++i) {
        const int q = i * GR_THREADS + tid;
        a_row[i] = q / (BM / 4);
        a_col[i] = (q % (BM / 4)) * 4;
    }
#pragma unroll
    for (int i = 0; i < NLB; ++i) {
        const int q = i * GR_THREADS + tid;
        b_row[i] = q / (BN / 4);
        b_col[i] = (q % (BN / 4)) * 4;
    }

    f32x16 acc[MTM][MTN];
    float bsum = 0.0f;

    const int nk = (m1 - m0 + GR_BK - 1) / GR_BK;
    float ra[NLA][4];
    float4 rb[NLB];

    auto load_global = [&](int ks) {
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            const int m = m0 + ks * GR_BK + a_row[i];
            const int b = m / Tout, t = m - b * Tout;
            bool valid = m < m1;
            if (valid) {
                int start;
                valid = t < tdnn_out_len(grad_len(p, b), p.f, start);
            }
            const float* gr = p.g + (int64_t)m * p.ldg;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int u = u0 + a_col[i] + e;
                ra[i][e] = (valid && u < p.f.units) ? gr[u] : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < NLB; ++i) {
            const int m = m0 + ks * GR_BK + b_row[i];
            const int b = m / Tout, t = m - b * Tout;
            const int d = d0 + b_col[i];
            rb[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (m < m1 && d < p.f.din_pad) {
                const int len = grad_len(p, b);
                int start;
                if (t < tdnn_out_len(len, p.f, start)) {
                    int r = start + t * p.f.sub + off;
                    r = r < 0 ? 0 : (r > len - 1 ? len - 1 : r);
                    rb[i] = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p.f.x) + ((int64_t)b * p.f.T + r) * p.f.ldx + d);
                }
            }
        }
    };
    auto store_lds = [&](int buf) {                      // both transposed: As[unit][row of the step], Bs[feature][row of the step]
#pragma unroll
        for (int i = 0; i < NLA; ++i) {
            float* a = &As[buf][a_col[i] * GR_PITCH + a_row[i]];
            a[0] = ra[i][0]; a[GR_PITCH] = ra[i][1]; a[2 * GR_PITCH] = ra[i][2]; a[3 * GR_PITCH] = ra[i][3];
        }
#pragma unroll
        for (int i = 0; i < NLB; ++i) {
            float* bb = &Bs[buf][b_col[i] * GR_PITCH + b_row[i]];
            bb[0] = rb[i].x; bb[GR_PITCH] = rb[i].y; bb[2 * GR_PITCH] = rb[i].z; bb[3 * GR_PITCH] = rb[i].w;
        }
    };

    // (nk >= 1: the grid has one z per slot that holds a row, so m0 < p.rows)
    tile32_mainloop<MTM, MTN, GR_BK, false>(acc, &As[0][0], &Bs[0][0], nk, wm, wn, lane, load_global, store_lds, [&](int buf) {
        if (with_bias && tid < BM) {
#pragma unroll
            for (int r = 0; r < GR_BK; ++r) bsum += As[buf][tid * GR_PITCH + r];
        }
    });

    float* ws = p.slots + (int64_t)slot * p.slot_stride;
#pragma unroll
    for (int i = 0; i < MTM; ++i)
#pragma unroll
        for (int j = 0; j < MTN; ++j) {
            const int d = d0 + wn * 32 * MTN + j * 32 + (lane & 31);
            if (d >= p.f.din_pad) continue;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int u = acc32_row(u0 + wm * 32 * MTM + i * 32, reg, lane);
                if (u < p.units_pad) ws[(int64_t)u * p.f.ktot + (int64_t)k * p.f.din_pad + d] = acc[i][j][reg];
            }
        }
    if (with_bias && tid < BM && u0 + tid < p.units_pad) ws[(int64_t)p.units_pad * p.f.ktot + u0 + tid] = bsum;
}

// ------------------------------------------------------------------------------------ gradient of the reducing statistics pooling
// One workgroup = one utterance x 64 columns, four row groups. The column sums are taken again, in fp64 (rows j -> group j mod 4,
// groups added as ((0 + 1) + 2) + 3), then every row of the utterance's T is written: the sampled rows below its length with the
// gradient, evaluated in fp64 and rounded once, the others with zero.
__global__ __launch_bounds__(GR_THREADS) void grad_pool_kernel(const float* __restrict__ x, int64_t T, int D, int64_t ldx,
                                                               const int32_t* __restrict__ lens, int period, int include_std, float eps,
                                                               const float* __restrict__ gout, int64_t ldg, float* __restrict__ dx,
                                                               int64_t ld_dx) {
    __shared__ double red[4][2][64];
    const int b = blockIdx.y;
    const int lc = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lc;
    int len = lens ? lens[b] : (int)T;
    len = len < 0 ? 0 : (len > (int)T ? (int)T : len);
    const int nrows = (len + period - 1) / period;
    const float* xb = x + (int64_t)b * T * ldx;
    double s = 0.0, q = 0.0;
    if (c < D)
        for (int j = rg; j < nrows; j += 4) {
            const double v = (double)xb[(int64_t)j * period * ldx + c];
            s += v;
            q += v * v;
        }
    red[rg][0][lc] = s;
    red[rg][1][lc] = q;
    __syncthreads();
    if (c >= ld_dx) return;
    float* dxb = dx + (int64_t)b * T * ld_dx + c;
    double mean = 0.0, ca = 0.0, cb = 0.0;
    if (c < D && nrows > 0) {
        const double n = (double)nrows;
        const double S = ((red[0][0][lc] + red[1][0][lc]) + red[2][0][lc]) + red[3][0][lc];
        const double Q = ((red[0][1][lc] + red[1][1][lc]) + red[2][1][lc]) + red[3][1][lc];
        mean = S / n;
        const double var = Q / n - mean * mean;
        ca = (double)gout[(int64_t)b * ldg + c] / n;
        if (include_std && var > 0.0) cb = (double)gout[(int64_t)b * ldg + D + c] / (n * sqrt(var + (double)eps));
    }
    for (int t = rg; t < (int)T; t += 4) {
        float v = 0.0f;
        if (c < D && t < len && t % period == 0) {
            v = (float)(cb != 0.0 ? ca + cb * ((double)xb[(int64_t)t * ldx + c] - mean) : ca);
        }
        dxb[(int64_t)t * ld_dx] = v;
    }
}

// ------------------------------------------------------------------------------------ entry points
extern "C" int32_t ktf_grad_tdnn_row_tile(void) { return KTF_GRAD_ROW_TILE; }
extern "C" int32_t ktf_grad_tdnn_slot_rows(void) { return KTF_GRAD_SLOT_ROWS; }

extern "C" int64_t ktf_grad_tdnn_workspace_bytes(int64_t B, int64_t T, const KtfTdnnDesc* d) {
    const char* who = "ktf_grad_tdnn_workspace_bytes";
    if (int rc = grad_check_desc(d, who)) return rc;
    GradSizes s;
    if (int rc = grad_sizes(B, T, d, who, &s)) return rc;
    return s.bytes;
}

extern "C" int ktf_grad_tdnn_data(const float* g, int64_t ldg, int64_t B, int64_t T, const int32_t* lens, const KtfTdnnDesc* d, const float* w,
                                  float* dx, int64_t ldx, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_grad_tdnn_data";
    if (int rc = grad_check_desc(d, who)) return rc;
    GradSizes s;
    if (int rc = grad_check_args(who, g, w, dx, workspace, workspace_bytes, B, T, d, ldx, ldg, w, dx, "w and dx", &s)) return rc;
    if (B == 0 || T == 0) return KTF_OK;
    GradParams p;
    grad_fill(p, s, B, T, lens, d, nullptr, ldx, w, g, ldg, workspace);
    p.dx = dx;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nfold = B * 2 * d->nctx * d->units;
    hipLaunchKernelGGL(grad_fold_kernel<false>, dim3((unsigned)ktf_cdiv(nfold, GR_THREADS)), dim3(GR_THREADS), 0, st, p);
    KTF_CHECK_LAUNCH(who);
    const dim3 grid((unsigned)ktf_cdiv(ldx, 128), (unsigned)ktf_cdiv(T, KTF_GRAD_ROW_TILE), (unsigned)B);
    hipLaunchKernelGGL((grad_dx_kernel<1, 2>), grid, dim3(GR_THREADS), 0, st, p);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_grad_tdnn_weights(const float* x, int64_t B, int64_t T, int64_t ldx, const int32_t* lens, const KtfTdnnDesc* d, const float* g,
                                     int64_t ldg, float* dw, float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_grad_tdnn_weights";
    if (int rc = grad_check_desc(d, who)) return rc;
    GradSizes s;
    if (int rc = grad_check_args(who, x, g, dw, workspace, workspace_bytes, B, T, d, ldx, ldg, x, dw, "x and dw", &s)) return rc;
    GradParams p;
    grad_fill(p, s, B, T, lens, d, x, ldx, nullptr, g, ldg, workspace);
    hipStream_t st = (hipStream_t)stream;
    if (s.nslots > 0) {
        const dim3 grid((unsigned)(d->nctx * ktf_cdiv(d->din_pad, 128)), (unsigned)ktf_cdiv(d->units, 128), (unsigned)s.nslots);
        hipLaunchKernelGGL((grad_dw_kernel<2, 2>), grid, dim3(GR_THREADS), 0, st, p);
        KTF_CHECK_LAUNCH(who);
    }
    grad_launch_reduce(p, s, d, dw, dbias, st);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_grad_stats_pool(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const int32_t* lens, int32_t input_period,
                                   int32_t include_std, float eps, const float* gout, int64_t ld_gout, float* dx, int64_t ld_dx, void* stream) {
    const char* who = "ktf_grad_stats_pool";
    KTF_REQUIRE(x && gout && dx, "%s: null argument", who);
    KTF_REQUIRE(B >= 0 && T >= 0 && T < (1ll << 31) && D > 0 && ldx >= D && ld_dx >= D, "%s: bad sizes", who);
    KTF_REQUIRE(input_period > 0, "%s: input_period must be > 0", who);
    KTF_REQUIRE(B <= 65535, "%s: B %lld above 65535", who, (long long)B);
    KTF_REQUIRE(ld_gout >= (include_std ? 2 : 1) * (int64_t)D, "%s: ld_gout too small", who);
    if (B == 0 || T == 0) return KTF_OK;
    hipLaunchKernelGGL(grad_pool_kernel, dim3((unsigned)ktf_cdiv(ld_dx, 64), (unsigned)B), dim3(GR_THREADS), 0, (hipStream_t)stream, x, T, D, ldx,
                       lens, input_period, include_std, eps, gout, ld_gout, dx, ld_dx);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
