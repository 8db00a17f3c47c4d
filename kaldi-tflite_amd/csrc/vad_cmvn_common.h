// VAD and sliding-window CMVN device helpers shared by vad_cmvn.hip (the per-utterance hot path) and diar_windows.hip
// (per-segment CMN of diarization windows): one definition, so both produce the same bits. Moved unchanged from vad_cmvn.hip.
#pragma once
#include "common.h"
#include <type_traits>

#define VC_THREADS 1024
#define VC_RG (VC_THREADS / 32)      // row groups of the (row group, 32 columns) thread map
#define VC_GM (2 * VC_RG * 32)        // floats of LDS scratch in front of the staging area
#define VC_WAVES (VC_THREADS / KTF_WAVE)
#define CMVN_CHUNK 32

// phase stamps of workgroup 0 (probe builds of vad_cmvn.hip only: tools/vc_phase_probe.py defines them there)
#ifndef VC_PROBE
#define VC_PROBE(k)
#endif

// m * m rounded to fp32 before anything is subtracted from it (cmvn.py:206, 222: tf.pow(mean, 2) is a tensor of its own). HIP contracts
// a * b - c into a fused multiply-add by default (and __fmul_rn is a plain product there); with ONE frame the reference's variance is
// exactly 0 and its output 0 / 0, a fused form leaves the rounding residual of the square instead.
__device__ __forceinline__ float sq_rounded(float m) {
#pragma clang fp contract(off)
    return m * m;
}

__device__ __forceinline__ float block_sum(float v, float* red /* VC_WAVES floats in LDS */) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < VC_WAVES; ++w) t += red[w];
    return t;
}

// keep[t] of VAD.call for one utterance; e[u * es] = the energy coefficient of frame u (the feature rows themselves: e = feats +
// energy_coeff, es = D; or a copy of that column: es = 1).
__device__ __forceinline__ bool vad_keep(const float* __restrict__ e, int64_t es, int64_t T, const KtfVadCfg& c, float thr,
                                         int64_t t) {
    const int ctx = c.frames_context;
    if (ctx == 0) return e[t * es] > thr;
    int cnt = 0;
    for (int k = -ctx; k <= ctx; ++k) {
        const int64_t u = t + k;
        if (u >= 0 && u < T) cnt += (e[u * es] > thr) ? 1 : 0;
    }
    // vad.py:124-135,187-193: denominators at the edges = number of taps inside the sequence
    int den = 2 * ctx + 1;
    if (T >= 2 * (int64_t)ctx) {
        if (t < ctx) den = ctx + 1 + (int)t;
        else if (t >= T - ctx) den = ctx + (int)(T - t);
    } else {
        // fewer than 2*ctx frames: the reference scatters the edge sizes ctx+1 .. 2ctx (left) then 2ctx .. ctx+1 (right) at
        // indexes floormod(i + T, T), i = 0 .. ctx-1, -ctx .. -1, in that order, and the LAST write to a frame stands
        bool hit = false;
        for (int j = ctx - 1; j >= 0 && !hit; --j) {
            int64_t i = (T - ctx + j) % T;
            if (i < 0) i += T;
            if (i == t) { den = 2 * ctx - j; hit = true; }
        }
        for (int j = ctx - 1; j >= 0 && !hit; --j)
            if ((int64_t)j % T == t) { den = ctx + 1 + j; hit = true; }
    }
    return ((float)cnt / (float)den) >= c.proportion_threshold;
}

// (col: when given, the energy column is also copied there -- T floats of LDS the vote then reads instead of the feature rows)
__device__ __forceinline__ float vad_threshold(const float* __restrict__ f, int64_t T, int D, const KtfVadCfg& c,
                                               float* red, float* __restrict__ col = nullptr) {
    float thr = c.energy_threshold;
    if (c.energy_mean_scale > 0.0f || col) {
        float s = 0.0f;
        for (int64_t t = threadIdx.x; t < T; t += VC_THREADS) {
            const float v = f[t * D + c.energy_coeff];
            if (col) col[t] = v;
            s += v;
        }
        if (c.energy_mean_scale > 0.0f) {
            const float mean = block_sum(s, red) / (float)T;
            thr += c.energy_mean_scale * mean;
        } else {
            __syncthreads();
        }
    }
    return thr;
}

template <typename OutT>
__device__ __forceinline__ void store_out(OutT* p, float v);
template <>
__device__ __forceinline__ void store_out<float>(float* p, float v) { *p = v; }
template <>
__device__ __forceinline__ void store_out<unsigned short>(unsigned short* p, float v) { *p = f2bf(v); }

// CMVN of one utterance: rows r < len, row r read at x[(inv ? inv[r] : r) * ldx + d].
// The (compacted) rows are first staged contiguously into `xs` (len*D floats: LDS when the utterance fits, else the
// caller's global workspace), which removes the idx indirection and the global-memory latency from the sliding loops.
// Then every (chunk of CMVN_CHUNK window starts, column) item computes its first window sum directly, slides it, and
// writes the normalised frames itself — no window-sum array, no second pass. Pad columns [D, ldo) are written as zeros.
// gm: VC_GM floats of LDS scratch for the whole-utterance branch.
// split / nsplit: the workgroup is one of nsplit that share the utterance (small batches: one workgroup per utterance leaves 255 CUs
// idle and its window phase is bound by ONE CU's vector issue). A split owns a contiguous range of the window-start chunks; it stages
// only the rows its windows read and writes only its frames -- every value is computed exactly as the unsplit workgroup computes it.
template <typename OutT>
__device__ __forceinline__ void cmvn_block(const float* __restrict__ x, int64_t ldx, const int32_t* __restrict__ inv, int len, int D,
                           const KtfCmvnCfg& c, OutT* __restrict__ out, int64_t ldo, float* __restrict__ xs, float* gm,
                           int* out_len, float* __restrict__ bs = nullptr, int split = 0, int nsplit = 1) {
    const int N = c.window;
    const int tid = threadIdx.x;
    const int ldo_i = (int)ldo;
    if (len <= N && split) return;                         // whole-utterance statistics: the first split does all of it
    // this split's chunks [cA, cB) of window starts and the rows [r_lo, r_hi) they read
    int cA = 0, cB = 0, r_lo = 0, r_hi = len;
    if (len > N) {
        const int nstart_ = len - N + 1, nchunk_ = (nstart_ + CMVN_CHUNK - 1) / CMVN_CHUNK;
        cA = (int)((int64_t)nchunk_ * split / nsplit);
        cB = (int)((int64_t)nchunk_ * (split + 1) / nsplit);
        if (cB <= cA) return;
        r_lo = cA * CMVN_CHUNK;
        r_hi = min(cB * CMVN_CHUNK, nstart_) + N - 1;
    }
    // staging: the rows this split reads, up to 32 independent global loads in flight per thread (one load behind each store
    // would serialise the ~1 us latencies); kept frames are mostly consecutive, so a row group's loads stay coalesced
    {
        const int rs = tid >> 5, dl = tid & 31;
        for (int d0 = 0; d0 < D; d0 += 32) {
            const int d = d0 + dl;
            if (d < D)
                for (int r = r_lo + rs; r < r_hi; r += VC_RG * 16) {
                    float v[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        const int rr = r + u * VC_RG;
                        const bool ok = rr < r_hi;
                        const int t = ok ? (inv ? inv[rr] : rr) : 0;
                        v[u] = ok ? x[(int64_t)t * ldx + d] : 0.0f;
                    }
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        const int rr = r + u * VC_RG;
                        if (rr < r_hi) xs[rr * D + d] = v[u];
                    }
                }
        }
    }
    __syncthreads();
    VC_PROBE(3)
    if (len <= N) {
        // cmvn.py:214-222: statistics over all frames. VC_RG row groups x 32 columns per pass.
        const int rg = tid >> 5, dl = tid & 31;
        for (int d0 = 0; d0 < ldo_i; d0 += 32) {
            const int d = d0 + dl;
            float s = 0.0f, s2 = 0.0f;
            if (d < D)
                for (int r = rg; r < len; r += VC_RG) {
                    const float v = xs[r * D + d];
                    s += v;
                    s2 += v * v;
                }
            gm[rg * 32 + dl] = s;
            gm[VC_RG * 32 + rg * 32 + dl] = s2;
            __syncthreads();
            float mean = 0.0f, sd = 1.0f;
            {
                float ts = 0.0f, ts2 = 0.0f;
#pragma unroll
                for (int g = 0; g < VC_RG; ++g) {
                    ts += gm[g * 32 + dl];
                    ts2 += gm[VC_RG * 32 + g * 32 + dl];
                }
                mean = ts / (float)len;
                if (c.norm_vars) sd = sqrtf(ts2 / (float)len - sq_rounded(mean));      // (cmvn.py:206, 222: the square is rounded before the
                                                                                             // subtraction, no fused multiply-add: one frame -> exactly 0)
            }
            // VALID keeps the frames [N/2, len - (N-1)/2) (cmvn.py:238-243): none of an utterance shorter than the window, one of an
            // utterance exactly as long
            const int r0 = c.valid ? N / 2 : 0, nout = c.valid ? (len == N ? 1 : 0) : len;
            for (int r = rg; r < nout; r += VC_RG) {
                if (d < ldo_i) {
                    float v = 0.0f;
                    if (d < D) {
                        v = xs[(r0 + r) * D + d] - mean;
                        if (c.norm_vars) v = v / sd;
                    }
                    store_out<OutT>(out + (int64_t)r * ldo + d, v);
                }
            }
            __syncthreads();
        }
        if (out_len && tid == 0) *out_len = c.valid ? (len == N ? 1 : 0) : len;
        return;
    }
    // cmvn.py:172-182: frame t uses the window starting at clamp(t - N/2, 0, len - N); VALID keeps [N/2, len-(N-1)/2)
    const int nstart = len - N + 1;
    const int nchunk = (nstart + CMVN_CHUNK - 1) / CMVN_CHUNK;
    const int half = N / 2;
    const float fN = (float)N;
    // sums of the CMVN_CHUNK-row blocks of every column (bs: [2][nblk][ldo] floats of LDS, when the launcher found room):
    // the first window of a chunk starts on a block boundary, so its sum is N/CMVN_CHUNK block sums plus a short tail
    // instead of a chain of N dependent LDS reads per item
    const int nblk = len / CMVN_CHUNK;                 // complete blocks
    if (bs) {
        float* bs2 = bs + (size_t)((len + CMVN_CHUNK - 1) / CMVN_CHUNK) * ldo_i;
        const int kB = min(nblk, cB - 1 + N / CMVN_CHUNK);         // the blocks this split's first windows are made of
        for (int item = cA * ldo_i + tid; item < kB * ldo_i; item += VC_THREADS) {
            const int k = item / ldo_i, d = item - k * ldo_i;
            float a = 0.0f, a2 = 0.0f;
            if (d < D) {
                const float* p = xs + k * CMVN_CHUNK * D + d;
#pragma unroll 8
                for (int i = 0; i < CMVN_CHUNK; ++i) {
                    const float v = p[i * D];
                    a += v;
                    a2 += v * v;
                }
            }
            bs[item] = a;
            bs2[item] = a2;
        }
        __syncthreads();
    }
    VC_PROBE(4)
    (void)nchunk;
    for (int item = cA * ldo_i + tid; item < cB * ldo_i; item += VC_THREADS) {
        const int ch = item / ldo_i, d = item - ch * ldo_i;
        const int s0 = ch * CMVN_CHUNK;
        const int s1 = min(s0 + CMVN_CHUNK, nstart);
        const bool real = d < D;
        float a = 0.0f, a2 = 0.0f;
        if (real) {
            int i = 0;
            if (bs) {
                const float* bs2 = bs + (size_t)((len + CMVN_CHUNK - 1) / CMVN_CHUNK) * ldo_i;
                const int nb = N / CMVN_CHUNK;       // whole blocks inside the window (all complete: s0 + N <= len)
#pragma unroll 4
                for (int k = 0; k < nb; ++k) {
                    a += bs[(ch + k) * ldo_i + d];
                    a2 += bs2[(ch + k) * ldo_i + d];
                }
                i = nb * CMVN_CHUNK;
            }
            const float* p = xs + s0 * D + d;
#pragma unroll 4
            for (; i < N; ++i) {
                const float v = p[i * D];
                a += v;
                a2 += v * v;
            }
        }
        // the slide, fully unrolled and branch-free but for the store: eight starts' operands are read ahead of their arithmetic,
        // ~28 instructions per start. (A loop over the starts with its conditions inside compiles to ~100 per start, most of them
        // branches, and with one or two waves of items per SIMD the instruction count IS the time: 7.5 of the kernel's 20 us.)
        // Pad columns run the arithmetic on column 0 and store zeros; an utterance's last chunk may be short: the starts behind
        // its end repeat the last one's operands and store nothing.
        {
            const int cnt = s1 - s0;
            const int dd = real ? d : 0;
            const float* pn = xs + (s0 + N - 1) * D + dd;          // frame entering the window of start s0 + i: pn[i * D]
            const float* po = xs + (s0 - 1) * D + dd;              // frame leaving it: po[i * D] (i >= 1)
            const float* pc = xs + (s0 + half) * D + dd;           // the frame the window is centred on
            OutT* op = out + (s0 + (c.valid ? 0 : half)) * ldo_i + d;      // (T * ldo < 2^31: the launcher checks)
            const int last = (cnt - 1) * D;
            auto chunk = [&](auto nv_tag) {
                constexpr bool NV = decltype(nv_tag)::value;
                float mean = 0.0f, sd = 1.0f, mean0 = 0.0f, sd0 = 1.0f, meanl = 0.0f, sdl = 1.0f;
#pragma unroll
                for (int q = 0; q < CMVN_CHUNK / 8; ++q) {
                    float vn[8], vo[8], xc[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int i = q * 8 + k;
                        const int o = min(i * D, last);
                        vn[k] = i ? pn[o] : 0.0f;
                        vo[k] = i ? po[o] : 0.0f;
                        xc[k] = pc[o];
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const int i = q * 8 + k;
                        if (i) {
                            a += vn[k] - vo[k];
                            if (NV) a2 += vn[k] * vn[k] - vo[k] * vo[k];
                        }
                        mean = a / fN;
                        if (NV) sd = sqrtf(a2 / fN - sq_rounded(mean));
                        if (i == 0) { mean0 = mean; sd0 = sd; }
                        if (i == cnt - 1) { meanl = mean; sdl = sd; }
                        float v = xc[k] - mean;
                        if (NV) v = v / sd;
                        if (i < cnt) store_out<OutT>(op + i * ldo_i, real ? v : 0.0f);
                    }
                }
                // the first / last window also serve the N/2 edge frames before / after it (SAME): their statistics are parked
                // in LDS and those ~N frames are written by the whole workgroup below
                if (!c.valid) {
                    if (s0 == 0) { gm[d] = real ? mean0 : 0.0f; gm[ldo_i + d] = real ? sd0 : 1.0f; }
                    if (s1 == nstart) { gm[2 * ldo_i + d] = real ? meanl : 0.0f; gm[3 * ldo_i + d] = real ? sdl : 1.0f; }
                }
            };
            if (c.norm_vars) chunk(std::true_type{});
            else chunk(std::false_type{});
        }
    }
    VC_PROBE(5)
    if (!c.valid) {
        __syncthreads();
        const int n_head = half;                              // frames [0, half) use the first window
        const int t_tail = nstart + half;                     // frames [t_tail, len) use the last window
        const int e_lo = cA == 0 ? 0 : n_head;                // (the split that owns the first / last chunk holds its statistics)
        const int e_hi = cB == nchunk ? n_head + (len - t_tail) : n_head;
        for (int e = e_lo * ldo_i + tid; e < e_hi * ldo_i; e += VC_THREADS) {
            const int k = e / ldo_i, d = e - k * ldo_i;
            const bool tail = k >= n_head;
            const int t = tail ? t_tail + (k - n_head) : k;
            float v = 0.0f;
            if (d < D) {
                v = xs[t * D + d] - gm[(tail ? 2 * ldo_i : 0) + d];
                if (c.norm_vars) v = v / gm[(tail ? 3 * ldo_i : ldo_i) + d];
            }
            store_out<OutT>(out + (int64_t)t * ldo + d, v);
        }
    }
    VC_PROBE(6)
    if (out_len && tid == 0 && cA == 0) *out_len = c.valid ? nstart : len;     // (the split that owns the first chunk)
}
