// Sliding-window x-vector front end of diarization for gfx950: from the MFCC of R recordings laid end to end
// (one frame stream, recording r at frames [off[r], off[r + 1])) to the padded feature batches of the windows.
//
//   diar_segments_kernel  one 1024-thread workgroup per recording: the energy VAD over the recording's own frames (the threshold and
//                         vote of vad_cmvn.hip, same helpers), run starts and ends marked and compacted with ballot scans into a
//                         per-recording segment table at the recording's frame offset (a recording of T frames has fewer than T runs)
//   diar_windows_kernel   one workgroup per recording: the window count of every segment, an exclusive block scan, the windows
//                         themselves at the recording's frame offset (fewer windows than frames: the period is >= 1 frame)
//   diar_compact_kernel   after the host has read the counts: the compact (recording, start, end) tables, one workgroup per recording
//   diar_cmn_kernel       one workgroup per segment: cmvn_block over the segment's rows as one utterance (ktf_cmvn_f32's LDS
//                         decisions, so the bits are those of ktf_cmvn_f32 on the segment alone), written at the same frame positions
//   diar_gather_kernel    one 256-thread workgroup per window: its CMN'd rows, staged through LDS with 16-byte loads, into the
//                         (window, Tw, ldo) feature batch in the activation dtype with 16-byte stores, plus the window lengths
#include "vad_cmvn_common.h"

#define DW_THREADS 256
#define DW_STAGE 8192                  // floats of LDS staging per gather piece (32 KiB)

// exclusive scan of one int per thread over the VC_THREADS threads; *total = the sum (block-uniform). scan: VC_WAVES ints of LDS.
__device__ __forceinline__ int block_excl_scan(int v, int* scan, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    __syncthreads();
    if (lane == 63) scan[wave] = incl;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < VC_WAVES; ++w) {
        const int cw = scan[w];
        if (w < wave) woff += cw;
        tot += cw;
    }
    *total = tot;
    return woff + incl - v;
}

__global__ __launch_bounds__(VC_THREADS) void diar_segments_kernel(const float* __restrict__ mfcc, int D, const int32_t* __restrict__ off,
                                                                   KtfVadCfg c, int32_t* __restrict__ seg, int32_t* __restrict__ counts) {
    __shared__ float red[VC_WAVES];
    __shared__ int scan[VC_WAVES];
    const int r = blockIdx.x;
    const int64_t o = off[r];
    const int64_t T = off[r + 1] - o;
    if (T <= 0) {
        if (threadIdx.x == 0) counts[r] = 0;
        return;
    }
    const float* f = mfcc + o * D;
    const float thr = vad_threshold(f, T, D, c, red);          // (the mean over this recording's T frames: VAD.call on it alone)
    const float* e = f + c.energy_coeff;
    int32_t* s2 = seg + 2 * o;                                  // slot j: (start, end) of the j-th run
    int base_s = 0, base_e = 0;
    for (int64_t t0 = 0; t0 < T; t0 += VC_THREADS) {
        const int64_t t = t0 + threadIdx.x;
        const bool k = t < T && vad_keep(e, D, T, c, thr, t);
        const bool st = k && !(t > 0 && vad_keep(e, D, T, c, thr, t - 1));
        const bool en = k && !(t + 1 < T && vad_keep(e, D, T, c, thr, t + 1));
        int ts = 0, te = 0;
        const int ps = block_excl_scan(st ? 1 : 0, scan, &ts);
        const int pe = block_excl_scan(en ? 1 : 0, scan, &te);
        if (st) s2[2 * (base_s + ps)] = (int32_t)t;
        if (en) s2[2 * (base_e + pe) + 1] = (int32_t)(t + 1);
        base_s += ts;
        base_e += te;
    }
    if (threadIdx.x == 0) counts[r] = base_s;
}

__global__ __launch_bounds__(VC_THREADS) void diar_windows_kernel(const int32_t* __restrict__ seg, const int32_t* __restrict__ off, int32_t R,
                                                                  int32_t W, int32_t P, int32_t M, int32_t* __restrict__ win,
                                                                  int32_t* __restrict__ counts) {
    __shared__ int scan[VC_WAVES];
    const int r = blockIdx.x;
    const int64_t o = off[r];
    const int64_t T = off[r + 1] - o;
    const int n = counts[r];
    const int32_t* s2 = seg + 2 * o;
    int32_t* w2 = win + 2 * o;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += VC_THREADS) {
        const int i = i0 + threadIdx.x;
        int s = 0, e = 0, nw = 0;
        if (i < n) {
            s = s2[2 * i];
            e = s2[2 * i + 1];
            const int L = e - s;
            // emit [a, a + W) and advance by P while more than W + M frames are left, then [a, e)
            if (L > 0) nw = L > W + M ? 1 + (L - W - M + P - 1) / P : 1;
        }
        int tot = 0;
        const int pos = block_excl_scan(nw, scan, &tot);
        for (int j = 0; j < nw; ++j) {
            const int64_t q = (int64_t)base + pos + j;
            if (q >= T) break;                                  // (cannot happen for disjoint segments inside [0, T))
            const int a = s + j * P;
            w2[2 * q] = a;
            w2[2 * q + 1] = j == nw - 1 ? e : a + W;
        }
        base += tot;
    }
    if (threadIdx.x == 0) counts[R + r] = (int32_t)(base < T ? base : T);
}

// counts: nseg[R] then nwin[R]; G / S: the sizes of the compact tables the host allocated from them
__global__ __launch_bounds__(DW_THREADS) void diar_compact_kernel(const int32_t* __restrict__ seg, const int32_t* __restrict__ win,
                                                                  const int32_t* __restrict__ counts, const int32_t* __restrict__ off,
                                                                  int32_t R, int64_t G, int64_t S, int32_t* __restrict__ segs_out,
                                                                  int32_t* __restrict__ wins_out) {
    __shared__ long long part[2][DW_THREADS / KTF_WAVE];
    const int r = blockIdx.x;
    long long gs = 0, ws = 0;
    for (int q = threadIdx.x; q < r; q += DW_THREADS) {
        gs += counts[q];
        ws += counts[R + q];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        gs += __shfl_xor(gs, o, 64);
        ws += __shfl_xor(ws, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = gs;
        part[1][threadIdx.x >> 6] = ws;
    }
    __syncthreads();
    long long goff = 0, woff = 0;
#pragma unroll
    for (int w = 0; w < DW_THREADS / KTF_WAVE; ++w) {
        goff += part[0][w];
        woff += part[1][w];
    }
    const int64_t o = off[r];
    const int ns = counts[r], nw = counts[R + r];
    for (int i = threadIdx.x; i < ns; i += DW_THREADS) {
        if (goff + i >= G) break;
        int32_t* d = segs_out + 3 * (goff + i);
        d[0] = r;
        d[1] = seg[2 * (o + i)];
        d[2] = seg[2 * (o + i) + 1];
    }
    for (int i = threadIdx.x; i < nw; i += DW_THREADS) {
        if (woff + i >= S) break;
        int32_t* d = wins_out + 3 * (woff + i);
        d[0] = r;
        d[1] = win[2 * (o + i)];
        d[2] = win[2 * (o + i) + 1];
    }
}

// ktf_cmvn_f32 on one utterance of `len` rows: the rows staged in LDS up to 148 KiB, the block sums beside them while everything fits
// in 158 KiB -- decided here per segment by the same rule, since the block sums change the summation order of the window sums
__device__ __forceinline__ void dw_cmvn_plan(int len, int D, int64_t* stage, int64_t* bs) {
    const int64_t need = (int64_t)len * D;
    *stage = need * 4 <= 148 * 1024 ? need : 0;
    *bs = 2 * (int64_t)((len + CMVN_CHUNK - 1) / CMVN_CHUNK) * D;
    if ((VC_GM + *bs + *stage) * 4 > 158 * 1024) *bs = 0;
}

__global__ __launch_bounds__(VC_THREADS) void diar_cmn_kernel(const float* __restrict__ mfcc, int D, const int32_t* __restrict__ off, int32_t R,
                                                              const int32_t* __restrict__ segs, KtfCmvnCfg c, float* __restrict__ out,
                                                              float* __restrict__ work) {
    extern __shared__ __attribute__((aligned(16))) float dw_lds[];
    const int g = blockIdx.x;
    const int r = segs[3 * g], s = segs[3 * g + 1], e = segs[3 * g + 2];
    if (r < 0 || r >= R) return;
    const int64_t o = off[r];
    if (s < 0 || e <= s || (int64_t)e > off[r + 1] - o) return;
    const int len = e - s;
    int64_t stage, bsf;
    dw_cmvn_plan(len, D, &stage, &bsf);
    float* gm = dw_lds;
    float* bsp = bsf ? dw_lds + VC_GM : nullptr;
    const float* x = mfcc + (o + s) * D;
    float* y = out + (o + s) * D;
    if (stage) cmvn_block<float>(x, D, nullptr, len, D, c, y, D, dw_lds + VC_GM + bsf, gm, nullptr, bsp);
    else cmvn_block<float>(x, D, nullptr, len, D, c, y, D, work + (o + s) * D, gm, nullptr, bsp);
}

template <typename OutT>
__device__ __forceinline__ OutT dw_cvt(float v);
template <>
__device__ __forceinline__ float dw_cvt<float>(float v) { return v; }
template <>
__device__ __forceinline__ unsigned short dw_cvt<unsigned short>(float v) { return f2bf(v); }

// windows [w0, w0 + gridDim.x) -> out (gridDim.x, Tw, ldo) of OutT, rows >= the window's length and columns >= D zero; lens (gridDim.x)
template <typename OutT>
__global__ __launch_bounds__(DW_THREADS) void diar_gather_kernel(const float* __restrict__ cmn, int D, const int32_t* __restrict__ off, int32_t R,
                                                                 const int32_t* __restrict__ wins, int64_t w0, int32_t Tw, OutT* __restrict__ out,
                                                                 int32_t ldo, int32_t* __restrict__ lens) {
    __shared__ __attribute__((aligned(16))) float st[DW_STAGE + 4];
    constexpr int V = 16 / sizeof(OutT);                        // elements per 16-byte store
    const int64_t i = w0 + blockIdx.x;
    const int r = wins[3 * i], a = wins[3 * i + 1], b = wins[3 * i + 2];
    int len = 0;
    int64_t src = 0;                                            // float index of the window's first row in the frame stream
    if (r >= 0 && r < R) {
        const int64_t o = off[r];
        if (a >= 0 && b > a && (int64_t)b <= off[r + 1] - o) {
            len = min(b - a, Tw);
            src = (o + a) * D;
        }
    }
    if (threadIdx.x == 0) lens[blockIdx.x] = len;
    OutT* dst = out + (int64_t)blockIdx.x * Tw * ldo;
    const int rp = (DW_STAGE - 4) / D;                          // rows per piece
    const int nv = ldo / V;
    for (int t0 = 0; t0 < Tw; t0 += rp) {
        const int rows = min(rp, Tw - t0);
        const int vr = max(0, min(len - t0, rows));             // rows of this piece inside the window
        const int64_t g0 = src + (int64_t)t0 * D;
        const int64_t ga = g0 & ~3ll;                          // 16-byte aligned start (the stream is allocated with 4 floats of slack)
        const int sh = (int)(g0 - ga);
        const int nvec = (sh + vr * D + 3) >> 2;
        for (int k = threadIdx.x; k < nvec; k += DW_THREADS)
            *reinterpret_cast<float4*>(st + 4 * k) = *reinterpret_cast<const float4*>(cmn + ga + 4 * k);
        __syncthreads();
        for (int k = threadIdx.x; k < rows * nv; k += DW_THREADS) {
            const int t = k / nv, c0 = (k - t * nv) * V;
            union { OutT e[V]; float4 v; } u;
#pragma unroll
            for (int q = 0; q < V; ++q) {
                const int cc = c0 + q;
                u.e[q] = dw_cvt<OutT>(t < vr && cc < D ? st[sh + t * D + cc] : 0.0f);
            }
            *reinterpret_cast<float4*>(dst + (int64_t)(t0 + t) * ldo + c0) = u.v;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------------ C-ABI
static int dw_check_streams(const char* who, const int32_t* frames, const int32_t* offsets, int32_t R, int32_t D) {
    KTF_REQUIRE(frames && offsets, "%s: null argument", who);
    KTF_REQUIRE(R >= 0, "%s: R must be >= 0", who);
    KTF_REQUIRE(D > 0 && D <= VC_GM / 4, "%s: D must be in [1, %d]", who, VC_GM / 4);
    int64_t F = 0;
    for (int32_t r = 0; r < R; ++r) {
        KTF_REQUIRE(frames[r] >= 0, "%s: frames[%d] = %d < 0", who, r, frames[r]);
        F += frames[r];
    }
    KTF_REQUIRE(F * D < (1ll << 31), "%s: %lld frames x %d features: too many", who, (long long)F, D);
    return KTF_OK;
}

extern "C" int ktf_diar_segments(const float* mfcc, int32_t D, const int32_t* frames, const int32_t* offsets, int32_t R, const KtfVadCfg* vad,
                                 int32_t* seg_work, int32_t* counts, void* stream) {
    int rc = dw_check_streams("ktf_diar_segments", frames, offsets, R, D);
    if (rc) return rc;
    KTF_REQUIRE(mfcc && vad && seg_work && counts, "ktf_diar_segments: null argument");
    KTF_REQUIRE(vad->energy_coeff >= 0 && vad->energy_coeff < D, "ktf_diar_segments: energy_coeff %d outside [0,%d)", vad->energy_coeff, D);
    KTF_REQUIRE(vad->frames_context >= 0, "ktf_diar_segments: frames_context must be >= 0");
    KTF_REQUIRE(vad->energy_mean_scale >= 0.0f, "ktf_diar_segments: energy_mean_scale must be >= 0");
    if (R == 0) return KTF_OK;
    hipLaunchKernelGGL(diar_segments_kernel, dim3((unsigned)R), dim3(VC_THREADS), 0, (hipStream_t)stream, mfcc, D, offsets, *vad, seg_work, counts);
    KTF_CHECK_LAUNCH("ktf_diar_segments");
    return KTF_OK;
}

extern "C" int ktf_diar_windows(const int32_t* seg_work, const int32_t* frames, const int32_t* offsets, int32_t R, int32_t W, int32_t P,
                                int32_t M, int32_t* win_work, int32_t* counts, void* stream) {
    int rc = dw_check_streams("ktf_diar_windows", frames, offsets, R, 1);
    if (rc) return rc;
    KTF_REQUIRE(seg_work && win_work && counts, "ktf_diar_windows: null argument");
    KTF_REQUIRE(W > 0 && P > 0 && P <= W && M >= 0, "ktf_diar_windows: need W > 0, 0 < P <= W, M >= 0 (got %d, %d, %d)", W, P, M);
    KTF_REQUIRE((int64_t)W + M < (1ll << 30), "ktf_diar_windows: W + M too large");
    if (R == 0) return KTF_OK;
    hipLaunchKernelGGL(diar_windows_kernel, dim3((unsigned)R), dim3(VC_THREADS), 0, (hipStream_t)stream, seg_work, offsets, R, W, P, M, win_work,
                       counts);
    KTF_CHECK_LAUNCH("ktf_diar_windows");
    return KTF_OK;
}

extern "C" int ktf_diar_compact(const int32_t* seg_work, const int32_t* win_work, const int32_t* counts, const int32_t* frames,
                                const int32_t* offsets, int32_t R, int64_t G, int64_t S, int32_t* segments, int32_t* windows, void* stream) {
    int rc = dw_check_streams("ktf_diar_compact", frames, offsets, R, 1);
    if (rc) return rc;
    KTF_REQUIRE(seg_work && win_work && counts, "ktf_diar_compact: null argument");
    KTF_REQUIRE(G >= 0 && S >= 0 && (G == 0 || segments) && (S == 0 || windows), "ktf_diar_compact: bad output tables");
    if (R == 0 || G + S == 0) return KTF_OK;
    hipLaunchKernelGGL(diar_compact_kernel, dim3((unsigned)R), dim3(DW_THREADS), 0, (hipStream_t)stream, seg_work, win_work, counts, offsets, R, G,
                       S, segments, windows);
    KTF_CHECK_LAUNCH("ktf_diar_compact");
    return KTF_OK;
}

extern "C" int ktf_diar_segment_cmn(const float* mfcc, int32_t D, const int32_t* frames, const int32_t* offsets, int32_t R,
                                    const int32_t* segments, int64_t G, const KtfCmvnCfg* cmvn, float* out, float* work, void* stream) {
    int rc = dw_check_streams("ktf_diar_segment_cmn", frames, offsets, R, D);
    if (rc) return rc;
    KTF_REQUIRE(mfcc && cmvn && out && work && (G == 0 || segments), "ktf_diar_segment_cmn: null argument");
    KTF_REQUIRE(cmvn->window > 0, "ktf_diar_segment_cmn: window must be > 0");
    KTF_REQUIRE(!cmvn->valid, "ktf_diar_segment_cmn: VALID padding would move the rows (SAME only)");
    KTF_REQUIRE(G >= 0 && G < (1ll << 31), "ktf_diar_segment_cmn: bad segment count");
    if (G == 0) return KTF_OK;
    KTF_LDS_ONCE(160 * 1024, diar_cmn_kernel);
    hipLaunchKernelGGL(diar_cmn_kernel, dim3((unsigned)G), dim3(VC_THREADS), 158 * 1024, (hipStream_t)stream, mfcc, D, offsets, R, segments, *cmvn,
                       out, work);
    KTF_CHECK_LAUNCH("ktf_diar_segment_cmn");
    return KTF_OK;
}

extern "C" int ktf_diar_gather(const float* cmn, int32_t D, const int32_t* frames, const int32_t* offsets, int32_t R, const int32_t* windows,
                               int64_t S, int64_t w0, int64_t n, int32_t Tw, void* out, int32_t out_dtype, int32_t ldo, int32_t* lens,
                               void* stream) {
    int rc = dw_check_streams("ktf_diar_gather", frames, offsets, R, D);
    if (rc) return rc;
    KTF_REQUIRE(cmn && out && lens && windows, "ktf_diar_gather: null argument");
    KTF_REQUIRE(out_dtype == KTF_F32 || out_dtype == KTF_BF16, "ktf_diar_gather: out_dtype must be KTF_F32 or KTF_BF16");
    KTF_REQUIRE(ldo >= D && ldo % 8 == 0, "ktf_diar_gather: ldo must be >= D and a multiple of 8");
    KTF_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)cmn & 15) == 0, "ktf_diar_gather: cmn and out must be 16-byte aligned");
    KTF_REQUIRE(Tw > 0 && w0 >= 0 && n >= 0 && w0 + n <= S && n < (1ll << 31), "ktf_diar_gather: bad window range");
    if (n == 0) return KTF_OK;
    if (out_dtype == KTF_F32)
        hipLaunchKernelGGL(diar_gather_kernel<float>, dim3((unsigned)n), dim3(DW_THREADS), 0, (hipStream_t)stream, cmn, D, offsets, R, windows, w0,
                           Tw, (float*)out, ldo, lens);
    else
        hipLaunchKernelGGL(diar_gather_kernel<unsigned short>, dim3((unsigned)n), dim3(DW_THREADS), 0, (hipStream_t)stream, cmn, D, offsets, R,
                           windows, w0, Tw, (unsigned short*)out, ldo, lens);
    KTF_CHECK_LAUNCH("ktf_diar_gather");
    return KTF_OK;
}
