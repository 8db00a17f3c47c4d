// Shared by the TDNN gradient kernels (tdnn_grad.hip: the fp32 MFMA; tdnn_grad16.hip: the bf16 MFMA, include/ktf_grad.h rules 6-8): the
// kernel parameter block, the folded rows of the data gradient, the slot reduction of the weight gradient, and the host side of the
// entry points -- descriptor and argument checks, workspace sizes, the parameter fill. The kernels here are `static`: every
// translation unit that launches one holds its own copy.
#pragma once
#include "tdnn_common.h"
#include "../../include/ktf_grad.h"

#define GR_THREADS 256

struct GradParams {
    TdnnParams f;           // the forward's view: x, lens, w, T, ldx, Tout, units, din_pad, nctx, sub, valid, ktot, ctx
    const float* g;         // (B, Tout, ldg)
    float* dx;              // (B, T, ldx)
    float* fold;            // workspace: (B, 2, nctx, units) sums of the g rows whose x row was clamped to 0 / len - 1
    float* slots;           // workspace: `nslots` x slot_stride floats: dW partial (units_pad, ktot), then dbias partial (units_pad)
    int64_t ldg, slot_stride;
    int32_t B, din, units_pad, rows, nslots;     // rows = B * Tout: the flat row space of the weight gradient
};

__device__ __forceinline__ int grad_len(const GradParams& p, int b) {
    const int len = p.f.lens ? p.f.lens[b] : (int)p.f.T;
    return len < 0 ? 0 : (len > (int)p.f.T ? (int)p.f.T : len);
}

// ------------------------------------------------------------------------------------ clamped rows of the data gradient
// fold[b, e, k, u] = sum, in ascending t, of g[b, t, u] over the t < out_len whose row start + t * sub + ctx[k] lies below 0 (e = 0:
// a prefix of the t axis) or beyond len - 1 (e = 1: a suffix). At most |ctx[0]| + |ctx[nctx - 1]| rows per (b, k).
// ROUND_BF16: every g is rounded to bf16 (nearest even) first, the sum stays fp32 (KTF_GEMM_BF16, rule 6).
template <bool ROUND_BF16>
static __global__ __launch_bounds__(GR_THREADS) void grad_fold_kernel(GradParams p) {
    const int64_t idx = (int64_t)blockIdx.x * GR_THREADS + threadIdx.x;
    const int64_t total = (int64_t)p.B * 2 * p.f.nctx * p.f.units;
    if (idx >= total) return;
    const int u = (int)(idx % p.f.units);
    const int k = (int)((idx / p.f.units) % p.f.nctx);
    const int e = (int)((idx / ((int64_t)p.f.units * p.f.nctx)) & 1);
    const int b = (int)(idx / ((int64_t)p.f.units * p.f.nctx * 2));
    const int len = grad_len(p, b);
    int start;
    const int out_len = tdnn_out_len(len, p.f, start);
    float s = 0.0f;
    if (out_len > 0) {
        const int num = (e == 0 ? 0 : len) - start - p.f.ctx[k];
        int cut = num <= 0 ? 0 : (num + p.f.sub - 1) / p.f.sub;      // first t that is not clamped low (e = 0) / that is clamped high (e = 1)
        cut = cut > out_len ? out_len : cut;
        const int t0 = e == 0 ? 0 : cut, t1 = e == 0 ? cut : out_len;
        const float* gb = p.g + (int64_t)b * p.f.Tout * p.ldg + u;
        for (int t = t0; t < t1; ++t) s += ROUND_BF16 ? bf2f(f2bf(gb[(int64_t)t * p.ldg])) : gb[(int64_t)t * p.ldg];
    }
    p.fold[idx] = s;
}

// ------------------------------------------------------------------------------------ slots of the weight gradient
// dW[u, c] = the slots' values added in slot order (zero in the pad region, which no slot is read for); then dbias likewise.
static __global__ __launch_bounds__(GR_THREADS) void grad_dw_reduce_kernel(GradParams p, float* __restrict__ dw, float* __restrict__ dbias) {
    const int64_t idx = (int64_t)blockIdx.x * GR_THREADS + threadIdx.x;
    const int64_t nw = (int64_t)p.units_pad * p.f.ktot;
    if (idx < nw) {
        const int u = (int)(idx / p.f.ktot);
        const int d = (int)(idx % p.f.ktot) % p.f.din_pad;
        float v = 0.0f;
        if (u < p.f.units && d < p.din)
            for (int s = 0; s < p.nslots; ++s) v += p.slots[(int64_t)s * p.slot_stride + idx];
        dw[idx] = v;
    } else if (dbias && idx - nw < p.f.units) {
        float v = 0.0f;
        for (int s = 0; s < p.nslots; ++s) v += p.slots[(int64_t)s * p.slot_stride + idx];
        dbias[idx - nw] = v;
    }
}

// ------------------------------------------------------------------------------------ host side of the entry points
static int grad_check_desc(const KtfTdnnDesc* d, const char* who) {
    KTF_REQUIRE(d != nullptr, "%s: null argument", who);
    KTF_REQUIRE(d->gemm == KTF_GEMM_F32, "%s: gemm %d: the gradients exist for KTF_GEMM_F32 only", who, d->gemm);
    KTF_REQUIRE(d->act == KTF_ACT_NONE, "%s: act %d: the trainable forward has no fused activation (KTF_ACT_NONE)", who, d->act);
    KTF_REQUIRE(d->x_dtype == KTF_F32 && d->w_dtype == KTF_F32 && d->y_dtype == KTF_F32, "%s: x, w and y must be KTF_F32", who);
    return tdnn_check_desc(d, nullptr, nullptr, who);
}

// sizes shared by the TDNN entry points; KTF_OK or a refusal
struct GradSizes {
    int64_t Tout, rows, nslots, slot_stride, fold_bytes, bytes;
    int32_t units_pad, ktot;
};
static int grad_sizes(int64_t B, int64_t T, const KtfTdnnDesc* d, const char* who, GradSizes* s) {
    KTF_REQUIRE(B >= 0 && T >= 0, "%s: negative size", who);
    KTF_REQUIRE(B <= 65535, "%s: B %lld above 65535", who, (long long)B);
    s->Tout = ktf_tdnn_out_len(T, d);
    s->rows = B * s->Tout;
    KTF_REQUIRE(T <= 65535ll * KTF_GRAD_ROW_TILE, "%s: T %lld above %lld", who, (long long)T, 65535ll * KTF_GRAD_ROW_TILE);
    KTF_REQUIRE(s->rows < (1ll << 31), "%s: B * T_out must stay below 2^31", who);
    s->units_pad = (d->units + 255) / 256 * 256;
    s->ktot = d->nctx * d->din_pad;
    s->nslots = (s->rows + KTF_GRAD_SLOT_ROWS - 1) / KTF_GRAD_SLOT_ROWS;
    KTF_REQUIRE(s->nslots <= 65535, "%s: B * T_out %lld above 65535 slots of %d rows", who, (long long)s->rows, KTF_GRAD_SLOT_ROWS);
    s->slot_stride = (int64_t)s->units_pad * s->ktot + s->units_pad;
    s->fold_bytes = al256(B * 2 * d->nctx * d->units * (int64_t)sizeof(float));
    s->bytes = s->fold_bytes + al256((s->nslots > 0 ? s->nslots : 1) * s->slot_stride * (int64_t)sizeof(float));
    return KTF_OK;
}

// The argument checks of a data / weight gradient call behind its descriptor check (rule 5): a = g and b = w (data), or a = x and
// b = g (weights); `aligned` = the two operands read or written 16 bytes at a time, named by `aligned_names`.
static int grad_check_args(const char* who, const void* a, const void* b, const void* out, const void* workspace, size_t workspace_bytes,
                           int64_t B, int64_t T, const KtfTdnnDesc* d, int64_t ldx, int64_t ldg, const void* aligned0, const void* aligned1,
                           const char* aligned_names, GradSizes* s) {
    KTF_REQUIRE(a && b && out && workspace, "%s: null argument", who);
    if (int rc = grad_sizes(B, T, d, who, s)) return rc;
    KTF_REQUIRE(ldx >= d->din_pad && ldx % 4 == 0, "%s: ldx %lld must be a multiple of 4 and >= din_pad %d", who, (long long)ldx, d->din_pad);
    KTF_REQUIRE(ldg >= d->units, "%s: ldg %lld < units %d", who, (long long)ldg, d->units);
    KTF_REQUIRE(((reinterpret_cast<uintptr_t>(aligned0) | reinterpret_cast<uintptr_t>(aligned1)) & 15) == 0, "%s: %s must be 16-byte aligned", who,
                aligned_names);
    return ktf_check_workspace(who, workspace, workspace_bytes, s->bytes);
}

static void grad_fill(GradParams& p, const GradSizes& s, int64_t B, int64_t T, const int32_t* lens, const KtfTdnnDesc* d, const float* x,
                      int64_t ldx, const float* w, const float* g, int64_t ldg, void* workspace) {
    memset(&p, 0, sizeof(p));
    p.f.x = x;
    p.f.lens = lens;
    p.f.w = w;
    p.f.T = T;
    p.f.ldx = ldx;
    p.f.Tout = s.Tout;
    p.f.units = d->units;
    p.f.din_pad = d->din_pad;
    p.f.nctx = d->nctx;
    p.f.sub = d->subsampling;
    p.f.valid = d->valid;
    p.f.ktot = s.ktot;
    for (int i = 0; i < d->nctx; ++i) p.f.ctx[i] = d->ctx[i];
    p.g = g;
    p.ldg = ldg;
    p.fold = reinterpret_cast<float*>(workspace);
    p.slots = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + s.fold_bytes);
    p.slot_stride = s.slot_stride;
    p.B = (int32_t)B;
    p.din = d->din;
    p.units_pad = s.units_pad;
    p.rows = (int32_t)s.rows;
    p.nslots = (int32_t)s.nslots;
}

// The reduce launch that ends both weight gradient calls.
static inline void grad_launch_reduce(const GradParams& p, const GradSizes& s, const KtfTdnnDesc* d, float* dw, float* dbias, hipStream_t st) {
    const int64_t n = (int64_t)s.units_pad * s.ktot + d->units;
    hipLaunchKernelGGL(grad_dw_reduce_kernel, dim3((unsigned)ktf_cdiv(n, GR_THREADS)), dim3(GR_THREADS), 0, st, p, dw, dbias);
}
