// The optimiser step over one flat arena (include/ktf_optim.h, whose rule numbers the comments use).
//   ktf_optim_step   [optim_kernel<.., PASS_G> -> optim_clip_finalize_kernel]         clipping on
//                    [optim_kernel<.., PASS_D> -> optim_change_finalize_kernel]       max-change on
//                    optim_kernel<.., PASS_APPLY>
// One workgroup per slot of KTF_OPTIM_SLOT_ELEMS elements, a thread on four quads of four neighbouring elements. Streaming kernels:
// the apply pass of SGD with momentum moves 20 bytes per element (p, g, m in; p, m out), the reduce over g 4, the max-change reduce
// 12; every value is fp64 arithmetic rounded once.
#include "common.h"
#include "../../include/ktf_optim.h"

// every fp64 operation is rounded on its own: no contraction into fma
#pragma clang fp contract(off)

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_FIN_THREADS = 1024;                                    // the finalize workgroup: 16 waves, a segment each
constexpr int OPT_QUADS = KTF_OPTIM_SLOT_ELEMS / (4 * OPT_THREADS);   // quads per thread and slot
constexpr int PASS_G = 0, PASS_D = 1, PASS_APPLY = 2;
// the norms and scales in the workspace, in the order of the statistics (rule 12)
constexpr int SC_G = 0, SC_C = 1, SC_N = 2, SC_SIGMA = 3, SC_SKIPPED = 4, SC_SEG = 5;

static_assert(KTF_OPTIM_SLOT_ELEMS % (4 * OPT_THREADS) == 0, "a slot is a whole number of quads per thread");

struct OptParams {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t total;
    const KtfOptimSeg* segs;     // the device table
    int n_seg, n_groups, nslots;
    double lr[KTF_OPTIM_MAX_GROUPS], wd[KTF_OPTIM_MAX_GROUPS];
    double mu, beta1, beta2, om_beta1, om_beta2, eps, bc1, bc2_sqrt;
    int has_m, nesterov, decoupled, has_clip, has_change;
    double clip_norm, change_global;
    double* partial;             // (nslots)
    double* scal;                // (5 + n_seg)
    double* segsum;              // (n_seg)
    double* stats;               // the caller's, or NULL
};

__device__ __forceinline__ int64_t opt_clamp(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ bool opt_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN and Inf

// rules 2 - 5 on one element: d, and the new state before scaling
template <int KIND>
__device__ __forceinline__ void opt_element(const OptParams& q, double c, double wd, float pf, float gf, float mf, float vf, double& d,
                                            double& m1, double& v1) {
    const double p = (double)pf;
    double gh = c * (double)gf;
    if (!q.decoupled) gh = gh + wd * p;
    if (KIND == KTF_OPTIM_SGD) {
        v1 = 0.0;
        if (q.has_m) {
            m1 = q.mu * (double)mf + gh;
            d = q.nesterov ? gh + q.mu * m1 : m1;
        } else {
            m1 = 0.0;
            d = gh;
        }
    } else {
        m1 = q.beta1 * (double)mf + q.om_beta1 * gh;
        v1 = q.beta2 * (double)vf + q.om_beta2 * (gh * gh);
        d = (m1 / q.bc1) / (sqrt(v1) / q.bc2_sqrt + q.eps);
    }
    if (q.decoupled) d = d + wd * p;
}

// the quad at x of `a`: elements in [b, e) only; the 16-byte access where the whole quad is inside
template <bool VEC>
__device__ __forceinline__ void opt_load4(const float* __restrict__ a, int64_t x, int64_t b, int64_t e, float v[4]) {
    if (VEC && x >= b && x + 4 <= e) {
        const float4 t = *reinterpret_cast<const float4*>(a + x);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (x + j >= b && x + j < e) ? a[x + j] : 0.0f;
    }
}

template <bool VEC>
__device__ __forceinline__ void opt_store4(float* __restrict__ a, int64_t x, int64_t b, int64_t e, const float v[4]) {
    if (VEC && x >= b && x + 4 <= e) {
        *reinterpret_cast<float4*>(a + x) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x + j >= b && x + j < e) a[x + j] = v[j];
    }
}

// The three passes over a slot. PASS_G: the slot's sum of g^2. PASS_D: its sum of d^2. PASS_APPLY: rule 7.
template <int KIND, bool VEC, int PASS>
__global__ __launch_bounds__(OPT_THREADS) void optim_kernel(OptParams q) {
    __shared__ double red[OPT_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * KTF_OPTIM_SLOT_ELEMS;
    // the slot's segment: the last one that begins at or before the slot (segments begin on slot boundaries)
    int lo = 0, hi = q.n_seg;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (q.segs[mid].begin <= e0) lo = mid + 1;
        else hi = mid;
    }
    const int seg = lo - 1;
    int64_t b = 0, e = 0;
    int grp = 0;
    if (seg >= 0) {                                       // rule 13
        b = opt_clamp(q.segs[seg].begin, e0, q.total);
        e = opt_clamp(q.segs[seg].end, 0, q.total);
        e = e < e0 + KTF_OPTIM_SLOT_ELEMS ? e : e0 + KTF_OPTIM_SLOT_ELEMS;
        grp = (int)opt_clamp(q.segs[seg].group, 0, q.n_groups - 1);
    }
    const double c = (PASS != PASS_G && q.has_clip) ? q.scal[SC_C] : 1.0;
    double scale = 1.0;
    if (PASS == PASS_APPLY) {
        const double sigma = q.has_change ? q.scal[SC_SIGMA] : 1.0;
        const double skipped = (q.has_clip || q.has_change) ? q.scal[SC_SKIPPED] : 0.0;
        if (blockIdx.x == 0 && q.stats) {                 // rule 12
            for (int i = tid; i < SC_SEG + q.n_seg; i += OPT_THREADS) {
                double s;
                if (i == SC_G) s = q.has_clip ? q.scal[SC_G] : 0.0;
                else if (i == SC_C) s = c;
                else if (i == SC_N) s = q.has_change ? q.scal[SC_N] : 0.0;
                else if (i == SC_SIGMA) s = sigma;
                else if (i == SC_SKIPPED) s = skipped;
                else s = q.has_change ? q.scal[i] : 1.0;
                q.stats[i] = s;
            }
        }
        if (skipped != 0.0) return;                       // rule 10
        if (seg >= 0 && q.has_change) scale = sigma * q.scal[SC_SEG + seg];
    }
    if (b >= e) {                                         // a slot of padding
        if (PASS != PASS_APPLY && tid == 0) q.partial[blockIdx.x] = 0.0;
        return;
    }
    const double lr = q.lr[grp], wd = q.wd[grp];
    const bool use_m = KIND == KTF_OPTIM_ADAM || q.has_m;

    float pv[OPT_QUADS][4], gv[OPT_QUADS][4], mv[OPT_QUADS][4], vv[OPT_QUADS][4];
#pragma unroll
    for (int k = 0; k < OPT_QUADS; ++k) {
        const int64_t x = e0 + 4 * (tid + OPT_THREADS * k);
        opt_load4<VEC>(q.g, x, b, e, gv[k]);
        if (PASS != PASS_G) {
            opt_load4<VEC>(q.p, x, b, e, pv[k]);
            if (use_m) opt_load4<VEC>(q.m, x, b, e, mv[k]);
            if (KIND == KTF_OPTIM_ADAM) opt_load4<VEC>(q.v, x, b, e, vv[k]);
        }
    }
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < OPT_QUADS; ++k) {
        const int64_t x = e0 + 4 * (tid + OPT_THREADS * k);
        float po[4], mo[4], vo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = x + j >= b && x + j < e;
            if (PASS == PASS_G) {
                const double g = (double)gv[k][j];
                if (in) sum += g * g;
            } else {
                double d, m1, v1;
                opt_element<KIND>(q, c, wd, pv[k][j], gv[k][j], use_m ? mv[k][j] : 0.0f, KIND == KTF_OPTIM_ADAM ? vv[k][j] : 0.0f, d, m1, v1);
                if (PASS == PASS_D) {
                    if (in) sum += d * d;
                } else {
                    const double a = scale * lr;
                    po[j] = (float)((double)pv[k][j] - a * d);
                    mo[j] = KIND == KTF_OPTIM_SGD ? (float)(scale * m1) : (float)m1;
                    vo[j] = (float)v1;
                }
            }
        }
        if (PASS == PASS_APPLY) {
            opt_store4<VEC>(q.p, x, b, e, po);
            if (use_m) opt_store4<VEC>(q.m, x, b, e, mo);
            if (KIND == KTF_OPTIM_ADAM) opt_store4<VEC>(q.v, x, b, e, vo);
        }
    }
    if (PASS != PASS_APPLY) {                             // rule 8
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if ((tid & 63) == 0) red[tid >> 6] = sum;
        __syncthreads();
        if (tid == 0) q.partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}

// The slots of segment s of the device table, added by one wave (rule 8): lane l adds the segment's slots l, l + 64, ... in ascending
// order and the lanes are added by the butterfly; every lane returns the sum. (One thread walking a segment's slots one after the
// other took 30 us on the 900 slots of a 7 323-class head: a chain of dependent fp64 additions behind loads.)
__device__ __forceinline__ double opt_segment_sum(const OptParams& q, int s, int lane, int* grp, float* max_change) {
    const KtfOptimSeg sg = q.segs[s];
    const int64_t b = opt_clamp(sg.begin, 0, q.total), e = opt_clamp(sg.end, 0, q.total);
    *grp = (int)opt_clamp(sg.group, 0, q.n_groups - 1);
    *max_change = sg.max_change;
    double sum = 0.0;
    if (e > b) {
        const int64_t s0 = b / KTF_OPTIM_SLOT_ELEMS;
        int64_t s1 = (e + KTF_OPTIM_SLOT_ELEMS - 1) / KTF_OPTIM_SLOT_ELEMS;
        s1 = s1 < q.nslots ? s1 : q.nslots;
#pragma unroll 4
        for (int64_t i = s0 + lane; i < s1; i += 64) sum += q.partial[i];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    return sum;
}

// rule 1: G and c. One workgroup; wave w takes the segments w, w + 16, ...
__global__ __launch_bounds__(OPT_FIN_THREADS) void optim_clip_finalize_kernel(OptParams q) {
    const int lane = threadIdx.x & 63;
    for (int s = threadIdx.x >> 6; s < q.n_seg; s += OPT_FIN_THREADS / 64) {
        int grp;
        float mc;
        const double sum = opt_segment_sum(q, s, lane, &grp, &mc);
        if (lane == 0) q.segsum[s] = sum;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int s = 0; s < q.n_seg; ++s) sum += q.segsum[s];
    const double G = sqrt(sum);
    q.scal[SC_G] = G;
    q.scal[SC_C] = G > q.clip_norm ? q.clip_norm / G : 1.0;
    q.scal[SC_SKIPPED] = opt_finite(G) ? 0.0 : 1.0;
}

// rule 6: sigma_s, N and sigma; rule 10
__global__ __launch_bounds__(OPT_FIN_THREADS) void optim_change_finalize_kernel(OptParams q) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int s = threadIdx.x >> 6; s < q.n_seg; s += OPT_FIN_THREADS / 64) {
        int grp;
        float mc;
        const double sum = opt_segment_sum(q, s, lane, &grp, &mc);
        if (lane != 0) continue;
        const double Ns = q.lr[grp] * sqrt(sum);
        const double limit = (double)mc;
        const double sigma_s = (limit > 0.0 && Ns > limit) ? limit / Ns : 1.0;
        const double t = sigma_s * Ns;
        q.scal[SC_SEG + s] = sigma_s;
        q.segsum[s] = t * t;
        if (!opt_finite(Ns)) bad = 1;                     // every writer stores the same value
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int s = 0; s < q.n_seg; ++s) sum += q.segsum[s];
    const double N = sqrt(sum);
    q.scal[SC_N] = N;
    q.scal[SC_SIGMA] = (q.change_global > 0.0 && N > q.change_global) ? q.change_global / N : 1.0;
    const double before = q.has_clip ? q.scal[SC_SKIPPED] : 0.0;
    q.scal[SC_SKIPPED] = (before != 0.0 || bad || !opt_finite(N)) ? 1.0 : 0.0;
}

struct OptSizes {
    int64_t nslots, slot_bytes, scal_bytes, bytes;
};

int opt_sizes(const char* who, int64_t total, int32_t n_seg, OptSizes* s) {
    KTF_REQUIRE(total >= 0, "%s: negative total", who);
    KTF_REQUIRE(total < (1ll << 40), "%s: total reaches 2^40", who);
    KTF_REQUIRE(n_seg >= 0, "%s: negative n_seg", who);
    s->nslots = (total + KTF_OPTIM_SLOT_ELEMS - 1) / KTF_OPTIM_SLOT_ELEMS;
    s->slot_bytes = al256((s->nslots > 0 ? s->nslots : 1) * 8);
    s->scal_bytes = al256((5 + (int64_t)n_seg) * 8);
    s->bytes = s->slot_bytes + s->scal_bytes + al256((n_seg > 0 ? (int64_t)n_seg : 1) * 8);
    return KTF_OK;
}

bool opt_overlap(const float* a, const float* b, int64_t n) {
    if (!a || !b || n <= 0) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b, bytes = (uintptr_t)n * 4;
    return a0 < b0 + bytes && b0 < a0 + bytes;
}

bool opt_limit_ok(double x) { return x >= 0.0 && x < INFINITY; }      // false for NaN

template <int KIND, int PASS>
void opt_launch(bool vec, unsigned grid, hipStream_t st, const OptParams& q) {
    if (vec) hipLaunchKernelGGL((optim_kernel<KIND, true, PASS>), dim3(grid), dim3(OPT_THREADS), 0, st, q);
    else hipLaunchKernelGGL((optim_kernel<KIND, false, PASS>), dim3(grid), dim3(OPT_THREADS), 0, st, q);
}

template <int PASS>
void opt_launch_kind(int kind, bool vec, unsigned grid, hipStream_t st, const OptParams& q) {
    if (kind == KTF_OPTIM_SGD) opt_launch<KTF_OPTIM_SGD, PASS>(vec, grid, st, q);
    else opt_launch<KTF_OPTIM_ADAM, PASS>(vec, grid, st, q);
}

}  // namespace

// ------------------------------------------------------------------------------------ entry points
extern "C" int64_t ktf_optim_slot_elems(void) { return KTF_OPTIM_SLOT_ELEMS; }

extern "C" int64_t ktf_optim_workspace_bytes(int64_t total, int32_t n_seg) {
    OptSizes s;
    if (int rc = opt_sizes("ktf_optim_workspace_bytes", total, n_seg, &s)) return rc;
    return s.bytes;
}

extern "C" int ktf_optim_step(float* p, const float* g, float* m, float* v, int64_t total, const KtfOptimSeg* segs_host,
                              const KtfOptimSeg* segs_dev, int32_t n_seg, const KtfOptimGroup* groups, int32_t n_groups, int32_t kind,
                              double momentum, int32_t nesterov, double beta1, double beta2, double eps, int64_t step, int32_t decoupled,
                              double clip_norm, double max_change_global, double* stats, void* workspace, size_t workspace_bytes,
                              void* stream) {
    const char* who = "ktf_optim_step";
    KTF_REQUIRE(p && g && segs_host && segs_dev && groups && workspace, "%s: null argument", who);
    KTF_REQUIRE(kind == KTF_OPTIM_SGD || kind == KTF_OPTIM_ADAM, "%s: unknown kind %d", who, (int)kind);
    OptSizes sz;
    if (int rc = opt_sizes(who, total, n_seg, &sz)) return rc;
    KTF_REQUIRE(n_groups >= 1 && n_groups <= KTF_OPTIM_MAX_GROUPS, "%s: n_groups %d outside [1, %d]", who, (int)n_groups,
                KTF_OPTIM_MAX_GROUPS);
    for (int i = 0; i < n_groups; ++i) {
        KTF_REQUIRE(opt_limit_ok(groups[i].lr), "%s: lr of group %d negative or not finite", who, i);
        KTF_REQUIRE(opt_limit_ok(groups[i].weight_decay), "%s: weight_decay of group %d negative or not finite", who, i);
    }
    bool has_change = max_change_global > 0.0;
    int64_t prev_end = 0;
    for (int s = 0; s < n_seg; ++s) {
        const KtfOptimSeg& sg = segs_host[s];
        KTF_REQUIRE(sg.begin >= 0 && sg.begin % KTF_OPTIM_SLOT_ELEMS == 0, "%s: segment %d begin %lld is no multiple of %d", who, s,
                    (long long)sg.begin, KTF_OPTIM_SLOT_ELEMS);
        KTF_REQUIRE(sg.end >= sg.begin, "%s: segment %d ends before it begins", who, s);
        KTF_REQUIRE(sg.end <= total, "%s: segment %d end %lld beyond total %lld", who, s, (long long)sg.end, (long long)total);
        KTF_REQUIRE(sg.begin >= prev_end, "%s: segment %d begins before segment %d ends (ascending, no overlap)", who, s, s - 1);
        KTF_REQUIRE(sg.group >= 0 && sg.group < n_groups, "%s: segment %d group %d outside [0, %d)", who, s, (int)sg.group, (int)n_groups);
        KTF_REQUIRE(opt_limit_ok((double)sg.max_change), "%s: segment %d max_change negative or not finite", who, s);
        has_change = has_change || sg.max_change > 0.0f;
        prev_end = sg.end;
    }
    KTF_REQUIRE(opt_limit_ok(clip_norm), "%s: clip_norm negative or not finite", who);
    KTF_REQUIRE(opt_limit_ok(max_change_global), "%s: max_change_global negative or not finite", who);
    bool has_m = false;
    if (kind == KTF_OPTIM_SGD) {
        KTF_REQUIRE(momentum >= 0.0 && momentum < 1.0, "%s: momentum outside [0, 1)", who);
        KTF_REQUIRE(!nesterov || momentum > 0.0, "%s: nesterov needs a momentum above 0", who);
        has_m = momentum != 0.0;
        KTF_REQUIRE(!has_m || m, "%s: null m with momentum", who);
    } else {
        KTF_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "%s: beta outside [0, 1)", who);
        KTF_REQUIRE(eps > 0.0 && eps < INFINITY, "%s: eps must be positive and finite", who);
        KTF_REQUIRE(step >= 1, "%s: step %lld below 1", who, (long long)step);
        KTF_REQUIRE(m && v, "%s: null m or v for Adam", who);
        has_m = true;
    }
    if (int rc = ktf_check_workspace(who, workspace, workspace_bytes, sz.bytes)) return rc;
    float* um = has_m ? m : nullptr;                       // the arrays this call uses
    float* uv = kind == KTF_OPTIM_ADAM ? v : nullptr;
    KTF_REQUIRE(!opt_overlap(p, g, total) && !opt_overlap(p, um, total) && !opt_overlap(p, uv, total) && !opt_overlap(g, um, total) &&
                    !opt_overlap(g, uv, total) && !opt_overlap(um, uv, total),
                "%s: p, g, m, v overlap", who);

    hipStream_t st = (hipStream_t)stream;
    OptParams q = {};
    q.p = p; q.g = g; q.m = um; q.v = uv; q.total = total;
    q.segs = segs_dev; q.n_seg = n_seg; q.n_groups = n_groups; q.nslots = (int)sz.nslots;
    for (int i = 0; i < KTF_OPTIM_MAX_GROUPS; ++i) {
        q.lr[i] = i < n_groups ? groups[i].lr : 0.0;
        q.wd[i] = i < n_groups ? groups[i].weight_decay : 0.0;
    }
    q.mu = momentum; q.has_m = kind == KTF_OPTIM_SGD && has_m; q.nesterov = nesterov != 0; q.decoupled = decoupled != 0;
    if (kind == KTF_OPTIM_ADAM) {
        q.beta1 = beta1; q.beta2 = beta2; q.om_beta1 = 1.0 - beta1; q.om_beta2 = 1.0 - beta2; q.eps = eps;
        q.bc1 = 1.0 - pow(beta1, (double)step);
        q.bc2_sqrt = sqrt(1.0 - pow(beta2, (double)step));
    }
    q.has_clip = clip_norm > 0.0; q.has_change = has_change; q.clip_norm = clip_norm; q.change_global = max_change_global;
    char* ws = reinterpret_cast<char*>(workspace);
    q.partial = reinterpret_cast<double*>(ws);
    q.scal = reinterpret_cast<double*>(ws + sz.slot_bytes);
    q.segsum = reinterpret_cast<double*>(ws + sz.slot_bytes + sz.scal_bytes);
    q.stats = stats;
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)um | (uintptr_t)uv) & 15) == 0;   // rule 9
    const unsigned grid = (unsigned)(sz.nslots > 0 ? sz.nslots : 1);

    if (q.has_clip) {
        if (sz.nslots > 0) {
            opt_launch<KTF_OPTIM_SGD, PASS_G>(vec, grid, st, q);       // the kind does not enter the sum of g^2
            KTF_CHECK_LAUNCH(who);
        }
        hipLaunchKernelGGL(optim_clip_finalize_kernel, dim3(1), dim3(OPT_FIN_THREADS), 0, st, q);
        KTF_CHECK_LAUNCH(who);
    }
    if (q.has_change) {
        if (sz.nslots > 0) {
            opt_launch_kind<PASS_D>(kind, vec, grid, st, q);
            KTF_CHECK_LAUNCH(who);
        }
        hipLaunchKernelGGL(optim_change_finalize_kernel, dim3(1), dim3(OPT_FIN_THREADS), 0, st, q);
        KTF_CHECK_LAUNCH(who);
    }
    opt_launch_kind<PASS_APPLY>(kind, vec, grid, st, q);               // one slot at least: workgroup 0 writes the statistics
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
