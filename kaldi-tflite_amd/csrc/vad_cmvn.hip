// VAD -> per-utterance compaction -> sliding-window CMVN for gfx950.
//
// One 1024-thread workgroup (VC_THREADS) owns one utterance (utterances are independent, so a batch is
// B workgroups; no inter-workgroup traffic). The energy VAD needs the utterance mean of C0
// (block reduction), a (2*ctx+1)-tap vote with the reference's edge denominators, and a
// block-wide exclusive scan (wave ballots + LDS) to compact the kept frame numbers.
// CMVN evaluates the windowed sums S[s] = sum_{i<N} x[s+i] for every window start s with a
// chunked sliding update (direct sum for the first window of each 32-start chunk, then
// add-new/subtract-old), which is more accurate than the reference's difference of fp32
// cumulative sums and embarrassingly parallel over (chunk, feature).
//
// Replaces: layers/dsp/vad.py:156-203, models/kaldi/xvector_extractor.py:163-165,
//           layers/normalization/cmvn.py:186-250 of the reference.
#include "common.h"
// phase stamps of workgroup 0 (probe builds only: tools/vc_phase_probe.py)
#define VC_PROBE(k)
#include "vad_cmvn_common.h"

// Compacts kept frame numbers of one utterance into idx[0..count) (and into idx2, if given); returns count (block-uniform).
__device__ int vad_compact(const float* __restrict__ e, int64_t es, int64_t T, const KtfVadCfg& c, float thr,
                           int32_t* __restrict__ idx, int32_t* __restrict__ idx2, int* scan /* VC_WAVES+1 ints in LDS */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int64_t t0 = 0; t0 < T; t0 += VC_THREADS) {
        const int64_t t = t0 + threadIdx.x;
        const bool keep = (t < T) && vad_keep(e, es, T, c, thr, t);
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) scan[wave] = __popcll(m);
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < VC_WAVES; ++w) {
            const int cw = scan[w];
            if (w < wave) woff += cw;
            tot += cw;
        }
        if (keep) {
            idx[base + woff + before] = (int32_t)t;
            if (idx2) idx2[base + woff + before] = (int32_t)t;
        }
        base += tot;
    }
    return base;
}

__global__ __launch_bounds__(VC_THREADS) void vad_mask_kernel(const float* __restrict__ feats, int64_t T, int D,
                                                              KtfVadCfg c, float* __restrict__ mask) {
    __shared__ float red[VC_WAVES];
    const float* f = feats + (int64_t)blockIdx.x * T * D;
    const float thr = vad_threshold(f, T, D, c, red);
    for (int64_t t = threadIdx.x; t < T; t += VC_THREADS)
        mask[(int64_t)blockIdx.x * T + t] = vad_keep(f + c.energy_coeff, D, T, c, thr, t) ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(VC_THREADS) void vad_index_kernel(const float* __restrict__ feats, int64_t T, int D,
                                                               KtfVadCfg c, int32_t* __restrict__ idx,
                                                               int32_t* __restrict__ lens) {
    __shared__ float red[VC_WAVES];
    __shared__ int scan[VC_WAVES + 1];
    const float* f = feats + (int64_t)blockIdx.x * T * D;
    const float thr = vad_threshold(f, T, D, c, red);
    const int n = vad_compact(f + c.energy_coeff, D, T, c, thr, idx + (int64_t)blockIdx.x * T, nullptr, scan);
    if (threadIdx.x == 0) lens[blockIdx.x] = n;
}

// LDSF: the utterance is staged in LDS -- a pointer that is LDS in one launch and the global workspace in another compiles to flat
// loads (80 of them in the window phase, ~300 ns per dependent access); the two forms are two instantiations instead.
template <bool LDSF>
__global__ __launch_bounds__(VC_THREADS) void cmvn_kernel(const float* __restrict__ x, int64_t T, int D, int64_t ldx,
                                                          const int32_t* __restrict__ lens, KtfCmvnCfg c,
                                                          float* __restrict__ out, int64_t ldo,
                                                          int32_t* __restrict__ out_lens, float* __restrict__ work,
                                                          int64_t stage_floats, int64_t bs_floats) {
    extern __shared__ __attribute__((aligned(16))) float vc_lds[];
    float* gm = vc_lds;                      // VC_GM floats
    float* bsp = bs_floats ? vc_lds + VC_GM : nullptr;
    float* stage = vc_lds + VC_GM + bs_floats;
    const int b = blockIdx.x;
    const int len = lens ? lens[b] : (int)T;
    int* ol = out_lens ? out_lens + b : nullptr;
    float* xs = LDSF ? stage : work + (int64_t)b * T * 2 * D;
    cmvn_block<float>(x + (int64_t)b * T * ldx, ldx, nullptr, len, D, c, out + (int64_t)b * T * ldo, ldo, xs, gm, ol, bsp);
}

template <typename OutT, bool LDSF>
__global__ __launch_bounds__(VC_THREADS) void vad_cmvn_kernel(const float* __restrict__ feats, int64_t T, int D,
                                                              KtfVadCfg vc, KtfCmvnCfg cc, OutT* __restrict__ out,
                                                              int64_t ldo, int32_t* __restrict__ lens,
                                                              int32_t* __restrict__ idx_work,
                                                              float* __restrict__ work, int64_t stage_floats,
                                                              int64_t bs_floats, int64_t pos_ints, int64_t col_floats) {
    extern __shared__ __attribute__((aligned(16))) float vc_lds[];
    float* gm = vc_lds;                      // VC_GM floats (also the reduction scratch of the VAD phase)
    const int b = blockIdx.x;
    const int split = blockIdx.y, nsplit = gridDim.y;     // (every split repeats the VAD: it needs the whole frame -> row map)
    int32_t* idx = idx_work + (int64_t)b * T;
    // compacted row -> frame: T ints of LDS (and, from the first split, a copy in the caller's idx_work); a recording too long for
    // that (pos_ints == 0, > 38,400 frames) keeps only the copy in idx_work (written and read by this workgroup: same CU, same L1)
    int32_t* inv = (LDSF || pos_ints) ? reinterpret_cast<int32_t*>(vc_lds + VC_GM) : idx;
    float* bsp = bs_floats ? vc_lds + VC_GM + pos_ints : nullptr;
    float* col = col_floats ? vc_lds + VC_GM + pos_ints + bs_floats : nullptr;       // the energy column (vote input)
    float* stage = vc_lds + VC_GM + pos_ints + bs_floats + col_floats;
    float* red = gm;
    int* scan = reinterpret_cast<int*>(gm + 64);
    const float* f = feats + (int64_t)b * T * D;
    VC_PROBE(0)
    const float thr = vad_threshold(f, T, D, vc, red, col);
    VC_PROBE(1)
    const int n = LDSF ? vad_compact(col, 1, T, vc, thr, inv, split == 0 ? idx : nullptr, scan)
                       : vad_compact(col ? col : f + vc.energy_coeff, col ? 1 : D, T, vc, thr, inv, (pos_ints && split == 0) ? idx : nullptr, scan);
    __syncthreads();  // inv[] written by this workgroup is read below by other threads of it
    VC_PROBE(2)
    int* ol = lens + b;
    float* xs = LDSF ? stage : (((int64_t)n * D <= stage_floats) ? stage : work + (int64_t)b * T * 2 * D);
    cmvn_block<OutT>(f, D, inv, n, D, cc, out + (int64_t)b * T * ldo, ldo, xs, gm, ol, bsp, split, nsplit);
    VC_PROBE(7)
}

static int check_vad(const char* who, const float* feats, int64_t B, int64_t T, int32_t D, const KtfVadCfg* c) {
    KTF_REQUIRE(feats && c, "%s: null argument", who);
    KTF_REQUIRE(B >= 0 && T >= 0 && D > 0, "%s: bad sizes", who);
    KTF_REQUIRE(c->energy_coeff >= 0 && c->energy_coeff < D, "%s: energy_coeff %d outside [0,%d)", who, c->energy_coeff, D);
    KTF_REQUIRE(c->frames_context >= 0, "%s: frames_context must be >= 0", who);
    KTF_REQUIRE(c->energy_mean_scale >= 0.0f, "%s: energy_mean_scale must be >= 0", who);
    KTF_REQUIRE(T < (1ll << 31), "%s: T too large", who);
    return KTF_OK;
}

extern "C" int ktf_vad_mask_f32(const float* feats, int64_t B, int64_t T, int32_t D, const KtfVadCfg* cfg,
                                float* mask, void* stream) {
    int rc = check_vad("ktf_vad_mask_f32", feats, B, T, D, cfg);
    if (rc) return rc;
    KTF_REQUIRE(mask, "ktf_vad_mask_f32: null mask");
    if (B * T == 0) return KTF_OK;
    hipLaunchKernelGGL(vad_mask_kernel, dim3((unsigned)B), dim3(VC_THREADS), 0, (hipStream_t)stream, feats, T, D, *cfg, mask);
    KTF_CHECK_LAUNCH("ktf_vad_mask_f32");
    return KTF_OK;
}

extern "C" int ktf_vad_index(const float* feats, int64_t B, int64_t T, int32_t D, const KtfVadCfg* cfg, int32_t* idx,
                             int32_t* lens, void* stream) {
    int rc = check_vad("ktf_vad_index", feats, B, T, D, cfg);
    if (rc) return rc;
    KTF_REQUIRE(idx && lens, "ktf_vad_index: null output");
    if (B == 0) return KTF_OK;
    hipLaunchKernelGGL(vad_index_kernel, dim3((unsigned)B), dim3(VC_THREADS), 0, (hipStream_t)stream, feats, T, D, *cfg, idx, lens);
    KTF_CHECK_LAUNCH("ktf_vad_index");
    return KTF_OK;
}

// floats of LDS used to stage one utterance (0 = stage in the global workspace): whole utterances up to 148 KiB
static int64_t vc_stage_floats(int64_t T, int32_t D) {
    const int64_t need = T * D;
    return (need * 4 <= 148 * 1024) ? need : 0;
}

// ---------------------------------------------------------------------------------------------- where the working data lives
// The one place both launchers decide it (and ktf_cmvn_plan / ktf_vad_cmvn_plan report it): a chain of "does it still fit in
// 158 KiB beside what is already placed" tests, in the order map -> rows -> block sums -> energy column.
static const int64_t VC_LDS_FIT = 158 * 1024;

static void vc_plan_finish(KtfVcPlan* p) {
    p->lds_bytes = (VC_GM + p->pos_ints + p->bs_floats + p->col_floats + p->stage_floats) * (int64_t)sizeof(float);
}

// ktf_cmvn_f32: rows in LDS (cmvn_kernel<true>) or in `work`; block sums only when they fit beside the staged utterance
static void cmvn_plan(int64_t T, int32_t D, int64_t ldo, KtfVcPlan* p) {
    p->pos_ints = 0;
    p->col_floats = 0;
    p->stage_floats = vc_stage_floats(T, D);
    p->bs_floats = 2 * ((T + CMVN_CHUNK - 1) / CMVN_CHUNK) * ldo;
    if ((VC_GM + p->bs_floats + p->stage_floats) * 4 > VC_LDS_FIT) p->bs_floats = 0;
    p->nsplit = 1;
    p->lds_form = p->stage_floats ? 1 : 0;
    vc_plan_finish(p);
}

// ktf_vad_cmvn. The frame -> compacted-row map lives in LDS while (T + VC_GM) * 4 B <= 158 KiB (utterances up to ~6.4 min at
// 10 ms); beyond that it lives in idx_work (which then holds the map, not a copy of it). Small batches: up to eight workgroups
// share an utterance (cmvn_block) while the map, the energy column and the rows are all staged in LDS (a split workgroup of the
// global-workspace form would write rows its siblings write too); that is also the LDSF instantiation.
static void vad_cmvn_plan(int64_t B, int64_t T, int32_t D, int64_t ldo, KtfVcPlan* p) {
    int64_t pos_ints = (T + 3) & ~3ll;
    if ((VC_GM + pos_ints) * 4 > VC_LDS_FIT) pos_ints = 0;
    int64_t stage_floats = vc_stage_floats(T, D);
    if ((VC_GM + pos_ints + stage_floats) * 4 > VC_LDS_FIT) stage_floats = 0;
    int64_t bs_floats = 2 * ((T + CMVN_CHUNK - 1) / CMVN_CHUNK) * ldo;
    if ((VC_GM + pos_ints + bs_floats + stage_floats) * 4 > VC_LDS_FIT) bs_floats = 0;
    int64_t col_floats = (T + 3) & ~3ll;
    if ((VC_GM + pos_ints + bs_floats + col_floats + stage_floats) * 4 > VC_LDS_FIT) col_floats = 0;
    p->pos_ints = pos_ints;
    p->stage_floats = stage_floats;
    p->bs_floats = bs_floats;
    p->col_floats = col_floats;
    p->lds_form = (pos_ints && stage_floats && col_floats) ? 1 : 0;
    p->nsplit = 1;
    if (p->lds_form) p->nsplit = (int32_t)(B >= 256 ? 1 : (256 / B > 8 ? 8 : 256 / B));
    vc_plan_finish(p);
}

static int check_cmvn(const char* who, const KtfCmvnCfg* c) {
    KTF_REQUIRE(c, "%s: null cmvn config", who);
    KTF_REQUIRE(c->window > 0, "%s: window must be > 0", who);
    return KTF_OK;
}

extern "C" int ktf_cmvn_f32(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const int32_t* lens,
                            const KtfCmvnCfg* cfg, float* out, int64_t ldo, int32_t* out_lens, float* work,
                            void* stream) {
    int rc = check_cmvn("ktf_cmvn_f32", cfg);
    if (rc) return rc;
    KTF_REQUIRE(x && out && work, "ktf_cmvn_f32: null argument");
    KTF_REQUIRE(B >= 0 && T >= 0 && D > 0 && ldx >= D && ldo >= D, "ktf_cmvn_f32: bad sizes");
    KTF_REQUIRE(ldo <= VC_GM / 4, "ktf_cmvn_f32: ldo > %d", VC_GM / 4);
    KTF_REQUIRE(T < (1ll << 31) / (ldo > 0 ? ldo : 1), "ktf_cmvn_f32: T*ldo too large");
    if (B * T == 0) return KTF_OK;
    KtfVcPlan pl;
    cmvn_plan(T, D, ldo, &pl);
    const int64_t stage_floats = pl.stage_floats, bs_floats = pl.bs_floats;
    const size_t lds = (size_t)pl.lds_bytes;
    if (stage_floats) {
        KTF_LDS_ONCE(160 * 1024, cmvn_kernel<true>);
        hipLaunchKernelGGL(cmvn_kernel<true>, dim3((unsigned)B), dim3(VC_THREADS), lds, (hipStream_t)stream, x, T, D, ldx, lens, *cfg,
                           out, ldo, out_lens, work, stage_floats, bs_floats);
    } else {
        KTF_LDS_ONCE(160 * 1024, cmvn_kernel<false>);
        hipLaunchKernelGGL(cmvn_kernel<false>, dim3((unsigned)B), dim3(VC_THREADS), lds, (hipStream_t)stream, x, T, D, ldx, lens, *cfg,
                           out, ldo, out_lens, work, stage_floats, bs_floats);
    }
    KTF_CHECK_LAUNCH("ktf_cmvn_f32");
    return KTF_OK;
}

extern "C" int ktf_vad_cmvn(const float* feats, int64_t B, int64_t T, int32_t D, const KtfVadCfg* vad,
                            const KtfCmvnCfg* cmvn, void* out, int32_t out_dtype, int64_t ldo, int32_t* lens,
                            int32_t* idx_work, float* work, void* stream) {
    int rc = check_vad("ktf_vad_cmvn", feats, B, T, D, vad);
    if (rc) return rc;
    rc = check_cmvn("ktf_vad_cmvn", cmvn);
    if (rc) return rc;
    KTF_REQUIRE(out && lens && idx_work && work, "ktf_vad_cmvn: null argument");
    KTF_REQUIRE(ldo >= D && ldo <= VC_GM / 4, "ktf_vad_cmvn: ldo must be in [D, %d]", VC_GM / 4);
    KTF_REQUIRE(out_dtype == KTF_F32 || out_dtype == KTF_BF16, "ktf_vad_cmvn: bad out_dtype");
    KTF_REQUIRE(T < (1ll << 31) / (ldo > 0 ? ldo : 1), "ktf_vad_cmvn: T*ldo too large");
    if (B == 0) return KTF_OK;
    if (T == 0) {
        (void)hipMemsetAsync(lens, 0, sizeof(int32_t) * B, (hipStream_t)stream);
        return KTF_OK;
    }
    hipStream_t st = (hipStream_t)stream;
    KtfVcPlan pl;
    vad_cmvn_plan(B, T, D, ldo, &pl);
    const int64_t pos_ints = pl.pos_ints, stage_floats = pl.stage_floats, bs_floats = pl.bs_floats, col_floats = pl.col_floats;
    const size_t lds = (size_t)pl.lds_bytes;
    const dim3 grid((unsigned)B, (unsigned)pl.nsplit);
    const bool ldsf = pl.lds_form != 0;       // map, energy column and rows all in LDS
#define VC_LAUNCH(OutT, F)                                                                                             \
    {                                                                                                                  \
        KTF_LDS_ONCE(160 * 1024, (vad_cmvn_kernel<OutT, F>));                                                          \
        hipLaunchKernelGGL((vad_cmvn_kernel<OutT, F>), grid, dim3(VC_THREADS), lds, st, feats, T, D, *vad, *cmvn, (OutT*)out, ldo, \
                           lens, idx_work, work, stage_floats, bs_floats, pos_ints, col_floats);                       \
    }
    if (out_dtype == KTF_F32) {
        if (ldsf) VC_LAUNCH(float, true) else VC_LAUNCH(float, false)
    } else {
        if (ldsf) VC_LAUNCH(unsigned short, true) else VC_LAUNCH(unsigned short, false)
    }
#undef VC_LAUNCH
    KTF_CHECK_LAUNCH("ktf_vad_cmvn");
    return KTF_OK;
}

// The placements the two launchers above choose, for callers (and tests) that want to know which of them an input takes.
// Host arithmetic only: no HIP call, so both work without a GPU.
static int check_plan(const char* who, int64_t B, int64_t T, int32_t D, int64_t ldo, const KtfVcPlan* plan) {
    KTF_REQUIRE(plan, "%s: null plan", who);
    KTF_REQUIRE(B > 0 && T > 0 && D > 0, "%s: bad sizes", who);
    KTF_REQUIRE(ldo >= D && ldo <= VC_GM / 4, "%s: ldo must be in [D, %d]", who, VC_GM / 4);
    KTF_REQUIRE(T < (1ll << 31) / ldo, "%s: T*ldo too large", who);
    return KTF_OK;
}

extern "C" int ktf_cmvn_plan(int64_t T, int32_t D, int64_t ldo, KtfVcPlan* plan) {
    int rc = check_plan("ktf_cmvn_plan", 1, T, D, ldo, plan);
    if (rc) return rc;
    cmvn_plan(T, D, ldo, plan);
    return KTF_OK;
}

extern "C" int ktf_vad_cmvn_plan(int64_t B, int64_t T, int32_t D, int64_t ldo, KtfVcPlan* plan) {
    int rc = check_plan("ktf_vad_cmvn_plan", B, T, D, ldo, plan);
    if (rc) return rc;
    vad_cmvn_plan(B, T, D, ldo, plan);
    return KTF_OK;
}

// ------------------------------------------------------------------------------------ per-utterance routing by voiced length
// XvectorExtractor.route_short_utterances: lens (B) -> lens_main (utterances of at least `min_frames` voiced frames keep their length,
// the others 0) and lens_short (the complement; utterances without a voiced frame stay 0 in both), and -- for the host, which
// decides whether the second pass is enqueued at all -- the number of short utterances, written to PINNED HOST memory followed by
// the call's sequence number (system-scope release): the host polls the sequence number while the GPU works through the first
// pass's launches; no copy, no event, no stream synchronisation. One workgroup.
__global__ __launch_bounds__(1024) void route_short_kernel(const int32_t* __restrict__ lens, int64_t B, int32_t min_frames, int32_t* __restrict__ lens_main,
                                                           int32_t* __restrict__ lens_short, int32_t* host_flag, int32_t seq) {
    __shared__ int part[16];
    int n = 0;
    for (int64_t b = threadIdx.x; b < B; b += blockDim.x) {
        const int len = lens[b];
        const bool is_short = len > 0 && len < min_frames;
        lens_main[b] = len >= min_frames ? len : 0;
        lens_short[b] = is_short ? len : 0;
        n += is_short ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0 && host_flag) {
        int tot = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += part[w];
        __hip_atomic_store(host_flag, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_flag + 1, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

extern "C" int ktf_route_short(const int32_t* lens, int64_t B, int32_t min_frames, int32_t* lens_main, int32_t* lens_short, int32_t* host_flag,
                               int32_t seq, void* stream) {
    KTF_REQUIRE(lens && lens_main && lens_short, "ktf_route_short: null argument");
    KTF_REQUIRE(B >= 0 && min_frames >= 0, "ktf_route_short: bad size");
    if (B == 0 && !host_flag) return KTF_OK;
    hipLaunchKernelGGL(route_short_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, lens, B, min_frames, lens_main, lens_short, host_flag, seq);
    KTF_CHECK_LAUNCH("ktf_route_short");
    return KTF_OK;
}
