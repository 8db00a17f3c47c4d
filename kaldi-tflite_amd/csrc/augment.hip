// Waveform augmentation (include/ktf_augment.h): RIR reverberation as a uniformly partitioned overlap-save convolution, noise mixing
// at an SNR against the early-reverberation energy, power normalisation and the output window.
//
// Partitions of P = 1024 samples. Input block i of a row is the window x[(i-1)P, (i+1)P) (zero outside [0, n)), i = 0 .. ceil(n/P);
// its packed spectrum X_i (augment_fft.h) is P complex fp32. Partition p of an RIR is h[pP, (p+1)P) followed by P zeros, spectrum
// H_p. Output block j, y[jP, (j+1)P), is the second half of the inverse transform of Y_j = sum_p X_{j-p} H_p, the sum taken in
// registers in ascending p. A workgroup owns AUG_J consecutive output blocks of one row: it keeps the AUG_J input spectra a step
// needs in registers, moves them down one block per step and loads one new X and one H_p per step, so every H_p and every X_i it
// loads feeds AUG_J products. The same pass against the spectra of h[s0:s1] only sums the squares of its output (fp64).
// A filter of at most KTF_AUG_DIRECT_TAPS taps (h, or h[s0:s1]) is applied in the time domain by the same workgroups instead: it is
// cheaper there, and a one-tap RIR then scales the signal exactly, which a transform of 2P points does not.
//
// Launches: aug_forward (x -> X_i, the partial sums of x^2, and y = x for rows without an RIR), aug_conv<false> (y),
// aug_conv<true> (partial sums of the early output), aug_powers (p_before, p_sig) -- ktf_aug_convolve; aug_gains (g per additive),
// aug_add (the adds in list order per sample, then the partial sums of y^2), aug_scale (p_after, the scale), aug_write (the window,
// the scale, fp32 or int16) -- ktf_aug_mix. Every fp64 sum is a per-block partial in a fixed order (thread, wave butterfly, the
// four waves in order) followed by a fixed-order sum of the partials of the row: no floating-point atomics anywhere, and nothing
// a row computes reads another row.
//
// Workspace of B rows, S = ceil(max n / P) + ceil(max L / P) + 1 blocks per row: y (B x S P floats), X (B x (ceil(max n / P) + 1)
// x 2P floats, only when a row has an RIR), three partial-sum arrays (B x S doubles), the gains (one double per additive).
#include <math.h>

#include "augment_fft.h"

namespace {

constexpr int AUG_J = 4;            // output blocks per workgroup of the convolution
constexpr int AUG_DIRECT = KTF_AUG_DIRECT_TAPS;     // filters up to this many taps are applied in the time domain

struct AugLayout {
    int64_t S, nxb, ldy, y, X, part, gains, total;      // offsets in bytes; part: 3 arrays of B * S doubles
    int32_t max_n, max_L;
    bool any_rir;
};

inline int64_t blocks_of(int64_t samples) { return (samples + AUG_P - 1) / AUG_P; }
inline int32_t aug_pre(int32_t fs) { return (int32_t)nearbyint(0.001 * (double)fs); }
inline int32_t aug_post(int32_t fs) { return (int32_t)nearbyint(0.05 * (double)fs); }
inline int32_t early_partitions(int32_t fs) { return (int32_t)blocks_of((int64_t)aug_pre(fs) + aug_post(fs)); }

int check_rows(const char* who, const int32_t* n, const int32_t* rir_ids, int32_t B, const int32_t* rir_lengths, int32_t R, int32_t fs,
               int64_t num_additives) {
    KTF_REQUIRE(B >= 0 && R >= 0, "%s: negative size (B = %d, R = %d)", who, (int)B, (int)R);
    KTF_REQUIRE(num_additives >= 0 && num_additives < (1ll << 31), "%s: negative size (%lld additives)", who, (long long)num_additives);
    KTF_REQUIRE(fs > 0, "%s: fs = %d, must be positive", who, (int)fs);
    KTF_REQUIRE(B == 0 || (n && rir_ids), "%s: null argument", who);
    KTF_REQUIRE(R == 0 || rir_lengths, "%s: null argument", who);
    for (int32_t r = 0; r < R; ++r)
        KTF_REQUIRE(rir_lengths[r] >= 1 && rir_lengths[r] <= KTF_AUG_MAX_SAMPLES, "%s: RIR %d has %d taps (1 .. 2^30)", who, (int)r,
                    (int)rir_lengths[r]);
    for (int32_t b = 0; b < B; ++b) {
        KTF_REQUIRE(n[b] >= 0 && n[b] <= KTF_AUG_MAX_SAMPLES, "%s: negative size (row %d has n = %d; 0 .. 2^30)", who, (int)b, (int)n[b]);
        KTF_REQUIRE(rir_ids[b] >= -1 && rir_ids[b] < R, "%s: row %d: RIR id %d out of range (-1 .. %d)", who, (int)b, (int)rir_ids[b],
                    (int)R - 1);
    }
    return KTF_OK;
}

// (after check_rows)
AugLayout layout_of(const int32_t* n, const int32_t* rir_ids, int32_t B, const int32_t* rir_lengths, int64_t num_additives) {
    AugLayout l;
    l.max_n = 0;
    l.max_L = 1;
    l.any_rir = false;
    for (int32_t b = 0; b < B; ++b) {
        if (n[b] > l.max_n) l.max_n = n[b];
        if (rir_ids[b] >= 0) {
            l.any_rir = true;
            if (rir_lengths[rir_ids[b]] > l.max_L) l.max_L = rir_lengths[rir_ids[b]];
        }
    }
    l.nxb = blocks_of(l.max_n) + 1;
    l.S = blocks_of(l.max_n) + blocks_of(l.max_L) + 1;
    l.ldy = l.S * AUG_P;
    int64_t o = 0;
    l.y = o; o += al256((int64_t)B * l.ldy * 4);
    l.X = o; o += l.any_rir ? al256((int64_t)B * l.nxb * 2 * AUG_P * 4) : 0;
    l.part = o; o += al256(3 * (int64_t)B * l.S * 8);
    l.gains = o; o += al256(num_additives * 8);
    l.total = o;
    return l;
}

__global__ __launch_bounds__(AUG_THREADS) void aug_tables_kernel(float2* __restrict__ t) {
    const int k = blockIdx.x * AUG_THREADS + threadIdx.x;      // 0 .. 2P - 1
    double s, c;
    if (k < AUG_P) sincospi(-2.0 * (double)k / (double)AUG_P, &s, &c);
    else sincospi(-(double)(k - AUG_P) / (double)AUG_P, &s, &c);
    t[k] = make_float2((float)c, (float)s);
}

// ---- the RIR bank
__global__ __launch_bounds__(AUG_THREADS) void aug_rir_peak_kernel(const float* __restrict__ h, const int32_t* __restrict__ offsets, int R,
                                                                   int pre, int post, int npe, int32_t* __restrict__ meta) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int off = offsets[r], L = offsets[r + 1] - off;
    float best = -INFINITY;
    constexpr int NONE = 0x7fffffff;
    int at = NONE;
    for (int i = tid; i < L; i += AUG_THREADS) {               // ascending i: the lowest index of the thread's maximum
        const float v = h[off + i];
        if (at == NONE || v > best) { best = v; at = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(at, o, 64);
        if (oi != NONE && (at == NONE || ov > best || (ov == best && oi < at))) { best = ov; at = oi; }
    }
    if ((tid & 63) == 0) { bv[tid >> 6] = best; bi[tid >> 6] = at; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (bi[w] != NONE && (bi[0] == NONE || bv[w] > bv[0] || (bv[w] == bv[0] && bi[w] < bi[0]))) { bv[0] = bv[w]; bi[0] = bi[w]; }
        const int k = bi[0] == NONE ? 0 : bi[0];
        const int s0 = max(0, k - pre), s1 = min(L, k + post);
        const int full0 = off / AUG_P + r;                      // >= the partitions of every RIR before this one
        const int early0 = offsets[R] / AUG_P + R + r * npe;
        int32_t* m = meta + (int64_t)r * KTF_AUG_META;
        m[0] = k; m[1] = s0; m[2] = s1; m[3] = L; m[4] = full0; m[5] = early0; m[6] = 0; m[7] = 0;
    }
}

// workgroup (p, r, kind): the spectrum of partition p of h_r (kind 0) or of h_r[s0:s1] (kind 1)
__global__ __launch_bounds__(AUG_THREADS) void aug_rir_spectra_kernel(const float* __restrict__ h, const int32_t* __restrict__ offsets,
                                                                      const int32_t* __restrict__ meta, const float* __restrict__ tables,
                                                                      float* __restrict__ spectra) {
    __shared__ __attribute__((aligned(16))) float2 tw[2 * AUG_P];
    __shared__ __attribute__((aligned(16))) float2 bufA[AUG_BUF], bufB[AUG_BUF];
    const int tid = threadIdx.x, p = blockIdx.x, r = blockIdx.y, early = blockIdx.z;
    const int32_t* m = meta + (int64_t)r * KTF_AUG_META;
    const int lo = early ? m[1] : 0, hi = early ? m[2] : m[3];
    if ((int64_t)p * AUG_P >= hi - lo) return;
    const float* src = h + offsets[r];
    aug_load_tables(tables, tw, tid);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int mm = tid + AUG_THREADS * q;                   // z[mm] = (a[2 mm], a[2 mm + 1]); a = the partition, then P zeros
        float2 z = make_float2(0.f, 0.f);
        if (mm < AUG_P / 2) {
            const int g = lo + p * AUG_P + 2 * mm;
            if (g < hi) z.x = src[g];
            if (g + 1 < hi) z.y = src[g + 1];
        }
        bufA[PADI(mm)] = z;
    }
    aug_fft(bufA, bufB, tw, tid);
    float2* out = reinterpret_cast<float2*>(spectra) + ((int64_t)(early ? m[5] : m[4]) + p) * AUG_P;
    aug_real_spectrum(bufB, tw + AUG_P, out, tid);
}

// ---- the signals
template <bool I16>
__device__ __forceinline__ float aug_sample(const void* row, int g) {
    if constexpr (I16) return (float)reinterpret_cast<const short*>(row)[g];
    else return reinterpret_cast<const float*>(row)[g];
}

// workgroup (i, b): input block i of row b
template <bool I16>
__global__ __launch_bounds__(AUG_THREADS) void aug_forward_kernel(const void* __restrict__ x, int64_t ldx, const int32_t* __restrict__ n_,
                                                                  const int32_t* __restrict__ rir_ids, const float* __restrict__ tables,
                                                                  float* __restrict__ y, int64_t ldy, float* __restrict__ X, int64_t nxb_max,
                                                                  double* __restrict__ part_before, int64_t S) {
    __shared__ __attribute__((aligned(16))) float2 tw[2 * AUG_P];
    __shared__ __attribute__((aligned(16))) float2 bufA[AUG_BUF], bufB[AUG_BUF];
    __shared__ double red[4];
    const int tid = threadIdx.x, i = blockIdx.x, b = blockIdx.y;
    const int n = n_[b];
    if (n == 0 || i > (n + AUG_P - 1) / AUG_P) return;
    const bool conv = rir_ids[b] >= 0;
    const void* row = I16 ? (const void*)(reinterpret_cast<const short*>(x) + (int64_t)b * ldx)
                          : (const void*)(reinterpret_cast<const float*>(x) + (int64_t)b * ldx);
    if (conv) aug_load_tables(tables, tw, tid);
    double sq = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int mm = tid + AUG_THREADS * q;
        const int64_t g = ((int64_t)i - 1) * AUG_P + 2 * mm;
        float2 z = make_float2(0.f, 0.f);
        if (g >= 0 && g < n) z.x = aug_sample<I16>(row, (int)g);
        if (g + 1 >= 0 && g + 1 < n) z.y = aug_sample<I16>(row, (int)g + 1);
        if (q >= 2) {                                           // the window's second half: the row's samples [iP, (i+1)P)
            sq += (double)z.x * (double)z.x;
            sq += (double)z.y * (double)z.y;
            if (!conv) {
                if (g < n) y[(int64_t)b * ldy + g] = z.x;
                if (g + 1 < n) y[(int64_t)b * ldy + g + 1] = z.y;
            }
        }
        if (conv) bufA[PADI(mm)] = z;
    }
    sq = aug_block_sum(sq, red, tid);
    if (tid == 0) part_before[(int64_t)b * S + i] = sq;
    if (!conv) return;
    aug_fft(bufA, bufB, tw, tid);
    aug_real_spectrum(bufB, tw + AUG_P, reinterpret_cast<float2*>(X) + ((int64_t)b * nxb_max + i) * AUG_P, tid);
}

// acc += x h on the two packed bins of a float4; `first`: its .xy is bin 0, two real products
__device__ __forceinline__ void aug_mac(float4& acc, const float4 x, const float4 h, bool first) {
    if (first) {
        acc.x += x.x * h.x;
        acc.y += x.y * h.y;
    } else {
        acc.x += x.x * h.x - x.y * h.y;
        acc.y += x.x * h.y + x.y * h.x;
    }
    acc.z += x.z * h.z - x.w * h.w;
    acc.w += x.z * h.w + x.w * h.z;
}

// workgroup (g, b): output blocks g AUG_J .. g AUG_J + AUG_J - 1 of row b. Thread t owns bins 2t, 2t + 1, P/2 + 2t, P/2 + 2t + 1.
template <bool EARLY>
__global__ __launch_bounds__(AUG_THREADS) void aug_conv_kernel(const int32_t* __restrict__ n_, const int32_t* __restrict__ rir_ids,
                                                               const int32_t* __restrict__ meta, const float* __restrict__ spectra,
                                                               const float* __restrict__ tables, const float* __restrict__ X,
                                                               int64_t nxb_max, float* __restrict__ y, int64_t ldy,
                                                               double* __restrict__ part_sig, int64_t S, const void* __restrict__ x,
                                                               int x_i16, int64_t ldx, const float* __restrict__ taps,
                                                               const int32_t* __restrict__ offsets) {
    __shared__ __attribute__((aligned(16))) float2 tw[2 * AUG_P];
    __shared__ __attribute__((aligned(16))) float2 bufA[AUG_BUF], bufB[AUG_BUF];
    __shared__ double red[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int j0 = blockIdx.x * AUG_J;
    const int n = n_[b], rir = rir_ids[b];
    if (n == 0 || rir < 0) return;
    const int32_t* m = meta + (int64_t)rir * KTF_AUG_META;
    const int Lh = EARLY ? m[2] - m[1] : m[3];
    const int64_t ylen = (int64_t)n + Lh - 1;
    const int ny = (int)((ylen + AUG_P - 1) / AUG_P);
    if (j0 >= ny) return;
    if (Lh <= AUG_DIRECT) {
        // a filter this short in the time domain: out[g] = sum_t h[t] x[g - t], fp64 fused multiply-adds in ascending t, rounded
        // to fp32 once (64 sequential fp32 adds measured 6e-7 of the largest sample, three times the transform path's error)
        __shared__ float hs[AUG_DIRECT];
        if (tid < Lh) hs[tid] = taps[offsets[rir] + (EARLY ? m[1] : 0) + tid];
        __syncthreads();
        const void* row = x_i16 ? (const void*)(reinterpret_cast<const short*>(x) + (int64_t)b * ldx)
                                : (const void*)(reinterpret_cast<const float*>(x) + (int64_t)b * ldx);
        for (int jj = 0; jj < AUG_J; ++jj) {
            const int j = j0 + jj;
            if (j >= ny) break;
            double sq = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t g = (int64_t)j * AUG_P + tid + AUG_THREADS * q;
                if (g >= ylen) continue;
                double s = 0.0;
                for (int t = 0; t < Lh; ++t) {
                    const int64_t i = g - t;
                    if (i >= 0 && i < n) s = fma((double)hs[t], (double)(x_i16 ? aug_sample<true>(row, (int)i) : aug_sample<false>(row, (int)i)), s);
                }
                const float v = (float)s;
                if constexpr (EARLY) sq += (double)v * (double)v;
                else y[(int64_t)b * ldy + g] = v;
            }
            if constexpr (EARLY) {
                sq = aug_block_sum(sq, red, tid);
                if (tid == 0) part_sig[(int64_t)b * S + j] = sq;
            }
        }
        return;
    }
    const int np = (Lh + AUG_P - 1) / AUG_P;
    const int nxb = (n + AUG_P - 1) / AUG_P + 1;
    aug_load_tables(tables, tw, tid);
    const float4* Xb = reinterpret_cast<const float4*>(X) + (int64_t)b * nxb_max * (AUG_P / 2);
    const float4* Hb = reinterpret_cast<const float4*>(spectra) + (int64_t)(EARLY ? m[5] : m[4]) * (AUG_P / 2);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 acc[AUG_J][2], xr[AUG_J][2];
#pragma unroll
    for (int jj = 0; jj < AUG_J; ++jj) {
        acc[jj][0] = zero;
        acc[jj][1] = zero;
        const int i = j0 + jj;
        const bool in = i < nxb;
        xr[jj][0] = zero;
        xr[jj][1] = zero;
        if (in) {                                               // (a branch, not a select between two addresses: the loads stay global)
            xr[jj][0] = Xb[(int64_t)i * (AUG_P / 2) + tid];
            xr[jj][1] = Xb[(int64_t)i * (AUG_P / 2) + AUG_THREADS + tid];
        }
    }
    const int pend = min(np, j0 + AUG_J);                      // past it every X index is negative
    for (int p = 0; p < pend; ++p) {
        if (p > 0) {
#pragma unroll
            for (int jj = AUG_J - 1; jj > 0; --jj) {
                xr[jj][0] = xr[jj - 1][0];
                xr[jj][1] = xr[jj - 1][1];
            }
            const int i = j0 - p;
            const bool in = i >= 0 && i < nxb;
            xr[0][0] = zero;
            xr[0][1] = zero;
            if (in) {
                xr[0][0] = Xb[(int64_t)i * (AUG_P / 2) + tid];
                xr[0][1] = Xb[(int64_t)i * (AUG_P / 2) + AUG_THREADS + tid];
            }
        }
        const float4 h0 = Hb[(int64_t)p * (AUG_P / 2) + tid], h1 = Hb[(int64_t)p * (AUG_P / 2) + AUG_THREADS + tid];
#pragma unroll
        for (int jj = 0; jj < AUG_J; ++jj) {
            aug_mac(acc[jj][0], xr[jj][0], h0, tid == 0);
            aug_mac(acc[jj][1], xr[jj][1], h1, false);
        }
    }
    constexpr float INV_P = 1.0f / (float)AUG_P;
#pragma unroll
    for (int jj = 0; jj < AUG_J; ++jj) {
        const int j = j0 + jj;
        if (j >= ny) break;                                     // (workgroup-uniform)
        bufA[PADI(2 * tid)] = make_float2(acc[jj][0].x, acc[jj][0].y);
        bufA[PADI(2 * tid + 1)] = make_float2(acc[jj][0].z, acc[jj][0].w);
        bufA[PADI(AUG_P / 2 + 2 * tid)] = make_float2(acc[jj][1].x, acc[jj][1].y);
        bufA[PADI(AUG_P / 2 + 2 * tid + 1)] = make_float2(acc[jj][1].z, acc[jj][1].w);
        __syncthreads();
        aug_real_spectrum_inv(bufA, bufB, tw + AUG_P, tid);
        aug_fft(bufB, bufA, tw, tid);                           // bufA = conj(P z'): the block is the transform's second half
        double sq = 0.0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int mm = AUG_P / 2 + tid + AUG_THREADS * q;
            const float2 r = bufA[PADI(mm)];
            const float v0 = r.x * INV_P, v1 = -r.y * INV_P;
            const int64_t g = (int64_t)j * AUG_P + 2 * (mm - AUG_P / 2);
            if constexpr (EARLY) {
                if (g < ylen) sq += (double)v0 * (double)v0;
                if (g + 1 < ylen) sq += (double)v1 * (double)v1;
            } else {
                float* dst = y + (int64_t)b * ldy + g;
                if (g + 1 < ylen) *reinterpret_cast<float2*>(dst) = make_float2(v0, v1);
                else if (g < ylen) dst[0] = v0;
            }
        }
        if constexpr (EARLY) {
            sq = aug_block_sum(sq, red, tid);
            if (tid == 0) part_sig[(int64_t)b * S + j] = sq;
        }
        __syncthreads();
    }
}

// the sum of part[0 .. count) in a fixed order (one workgroup)
__device__ __forceinline__ double aug_sum_parts(const double* __restrict__ part, int count, double* red, int tid) {
    double s = 0.0;
    for (int i = tid; i < count; i += AUG_THREADS) s += part[i];
    return aug_block_sum(s, red, tid);
}

// workgroup b: p_before and p_sig of row b
__global__ __launch_bounds__(AUG_THREADS) void aug_powers_kernel(const int32_t* __restrict__ n_, const int32_t* __restrict__ rir_ids,
                                                                 const int32_t* __restrict__ meta, const double* __restrict__ part_before,
                                                                 const double* __restrict__ part_sig, int64_t S, double* __restrict__ stats) {
    __shared__ double red[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n = n_[b], rir = rir_ids[b];
    double pb = 0.0, ps = 0.0;
    if (n > 0) {
        pb = aug_sum_parts(part_before + (int64_t)b * S, (n + AUG_P - 1) / AUG_P + 1, red, tid) / (double)n;
        ps = pb;
        if (rir >= 0) {
            const int32_t* m = meta + (int64_t)rir * KTF_AUG_META;
            const int64_t elen = (int64_t)n + (m[2] - m[1]) - 1;
            ps = elen > 0 ? aug_sum_parts(part_sig + (int64_t)b * S, (int)((elen + AUG_P - 1) / AUG_P), red, tid) / (double)elen : 0.0;
        }
    }
    if (tid == 0) {
        double* st = stats + (int64_t)b * KTF_AUG_STATS;
        st[0] = pb; st[1] = ps; st[2] = 0.0; st[3] = 1.0;
    }
}

// ---- mixing
__device__ __forceinline__ int64_t aug_ylen(int n, int rir, const int32_t* __restrict__ meta) {
    if (n == 0) return 0;
    return rir < 0 ? (int64_t)n : (int64_t)n + meta[(int64_t)rir * KTF_AUG_META + 3] - 1;
}

// t mod m for 0 <= t < 2^31 (an additive's duration is an int32)
__device__ __forceinline__ int64_t aug_wrap(int64_t t, int64_t m) {
    return t < m ? t : (int64_t)((unsigned)t % (unsigned)m);
}

// workgroup b: the gain of each additive of row b
__global__ __launch_bounds__(AUG_THREADS) void aug_gains_kernel(const int32_t* __restrict__ add_offsets, const KtfAugAdditive* __restrict__ adds,
                                                                const float* __restrict__ noise, const int64_t* __restrict__ noise_offsets,
                                                                const double* __restrict__ stats, double* __restrict__ gains) {
    __shared__ double red[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const double p_sig = stats[(int64_t)b * KTF_AUG_STATS + 1];
    for (int a = add_offsets[b]; a < add_offsets[b + 1]; ++a) {
        const KtfAugAdditive ad = adds[a];
        const int64_t off = noise_offsets[ad.noise], mlen = noise_offsets[ad.noise + 1] - off;
        const int64_t d = ad.duration > 0 ? (int64_t)ad.duration : mlen;
        double s = 0.0;
        for (int64_t t = tid; t < d; t += AUG_THREADS) {
            const double v = (double)noise[off + aug_wrap(t, mlen)];
            s += v * v;
        }
        s = aug_block_sum(s, red, tid);
        if (tid == 0) {
            const double p_nu = s / (double)d;
            gains[a] = p_nu > 0.0 ? sqrt(pow(10.0, -(double)ad.snr_db / 10.0) * p_sig / p_nu) : 0.0;
        }
        __syncthreads();
    }
}

// workgroup (blk, b): samples [blk P, (blk+1) P) of y_b: the adds in list order, then the block's sum of squares
__global__ __launch_bounds__(AUG_THREADS) void aug_add_kernel(const int32_t* __restrict__ n_, const int32_t* __restrict__ rir_ids,
                                                              const int32_t* __restrict__ meta, const int32_t* __restrict__ add_offsets,
                                                              const KtfAugAdditive* __restrict__ adds, const float* __restrict__ noise,
                                                              const int64_t* __restrict__ noise_offsets, const double* __restrict__ gains,
                                                              float* __restrict__ y, int64_t ldy, double* __restrict__ part_after, int64_t S) {
    __shared__ double red[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t ylen = aug_ylen(n_[b], rir_ids[b], meta);
    const int64_t g0 = (int64_t)blockIdx.x * AUG_P;
    if (g0 >= ylen) return;
    const int a0 = add_offsets[b], a1 = add_offsets[b + 1];
    float* yb = y + (int64_t)b * ldy;
    double sq = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t g = g0 + tid + AUG_THREADS * q;
        if (g >= ylen) continue;
        float v = yb[g];
        for (int a = a0; a < a1; ++a) {
            const KtfAugAdditive ad = adds[a];
            const int64_t off = noise_offsets[ad.noise], mlen = noise_offsets[ad.noise + 1] - off;
            const int64_t d = ad.duration > 0 ? (int64_t)ad.duration : mlen;
            const int64_t t = g - ad.start;
            if (t >= 0 && t < d) v = v + (float)gains[a] * noise[off + aug_wrap(t, mlen)];
        }
        if (a1 > a0) yb[g] = v;
        sq += (double)v * (double)v;
    }
    sq = aug_block_sum(sq, red, tid);
    if (tid == 0) part_after[(int64_t)b * S + blockIdx.x] = sq;
}

// workgroup b: p_after and the scale of row b
__global__ __launch_bounds__(AUG_THREADS) void aug_scale_kernel(const int32_t* __restrict__ n_, const int32_t* __restrict__ rir_ids,
                                                                const int32_t* __restrict__ meta, const double* __restrict__ part_after,
                                                                int64_t S, int normalize, double volume, double* __restrict__ stats) {
    __shared__ double red[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t ylen = aug_ylen(n_[b], rir_ids[b], meta);
    double pa = 0.0;
    if (ylen > 0) pa = aug_sum_parts(part_after + (int64_t)b * S, (int)((ylen + AUG_P - 1) / AUG_P), red, tid) / (double)ylen;
    if (tid == 0) {
        double* st = stats + (int64_t)b * KTF_AUG_STATS;
        st[2] = pa;
        st[3] = volume > 0.0 ? volume : (normalize && pa > 0.0 ? sqrt(st[0] / pa) : 1.0);
    }
}

// out[b][t] = scale y_b[k + t] for t below the row's output length, 0 up to T_out
template <bool I16>
__global__ __launch_bounds__(AUG_THREADS) void aug_write_kernel(const int32_t* __restrict__ n_, const int32_t* __restrict__ rir_ids,
                                                                const int32_t* __restrict__ meta, const float* __restrict__ y, int64_t ldy,
                                                                const double* __restrict__ stats, int shift, void* __restrict__ out,
                                                                int64_t ldo, int64_t T_out) {
    const int b = blockIdx.y;
    const int n = n_[b], rir = rir_ids[b];
    const int64_t len = shift ? (int64_t)n : aug_ylen(n, rir, meta);
    const int k = (shift && rir >= 0) ? meta[(int64_t)rir * KTF_AUG_META] : 0;
    const float scale = (float)stats[(int64_t)b * KTF_AUG_STATS + 3];
    const float* yb = y + (int64_t)b * ldy + k;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t t = (int64_t)blockIdx.x * AUG_P + threadIdx.x + AUG_THREADS * q;
        if (t >= T_out) continue;
        const float v = t < len ? yb[t] * scale : 0.0f;
        if constexpr (I16) {
            const float r = fminf(fmaxf(rintf(v), -32768.0f), 32767.0f);
            reinterpret_cast<short*>(out)[(int64_t)b * ldo + t] = (short)(int)r;
        } else {
            reinterpret_cast<float*>(out)[(int64_t)b * ldo + t] = v;
        }
    }
}

}  // namespace

extern "C" int32_t ktf_aug_partition(void) { return AUG_P; }

extern "C" int64_t ktf_aug_tables_floats(void) { return AUG_TABLE_FLOATS; }

extern "C" int ktf_aug_tables(float* tables, void* stream) {
    KTF_REQUIRE(tables, "ktf_aug_tables: null argument");
    KTF_REQUIRE(((uintptr_t)tables & 15) == 0, "ktf_aug_tables: tables not 16-byte aligned");
    hipLaunchKernelGGL(aug_tables_kernel, dim3(2 * AUG_P / AUG_THREADS), dim3(AUG_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<float2*>(tables));
    KTF_CHECK_LAUNCH("ktf_aug_tables");
    return KTF_OK;
}

static int check_bank(const char* who, const int32_t* offsets, int32_t R, int32_t fs) {
    KTF_REQUIRE(R >= 0, "%s: negative size (R = %d)", who, (int)R);
    KTF_REQUIRE(fs > 0, "%s: fs = %d, must be positive", who, (int)fs);
    KTF_REQUIRE(offsets, "%s: null argument", who);
    KTF_REQUIRE(offsets[0] == 0, "%s: offsets[0] = %d, must be 0", who, (int)offsets[0]);
    for (int32_t r = 0; r < R; ++r)
        KTF_REQUIRE(offsets[r + 1] > offsets[r], "%s: RIR %d has no taps (offsets must ascend)", who, (int)r);
    KTF_REQUIRE(offsets[R] <= KTF_AUG_MAX_SAMPLES, "%s: %d taps in all, above 2^30", who, (int)offsets[R]);
    return KTF_OK;
}

extern "C" int64_t ktf_aug_rir_spectra_floats(const int32_t* offsets, int32_t R, int32_t fs) {
    const int rc = check_bank("ktf_aug_rir_spectra_floats", offsets, R, fs);
    if (rc != KTF_OK) return rc;
    return ((int64_t)offsets[R] / AUG_P + R + (int64_t)R * early_partitions(fs)) * 2 * AUG_P;
}

extern "C" int ktf_aug_rir_prepare(const float* h, const int32_t* offsets, const int32_t* offsets_dev, int32_t R, int32_t fs,
                                   const float* tables, int32_t* meta, float* spectra, void* stream) {
    const char* who = "ktf_aug_rir_prepare";
    const int rc = check_bank(who, offsets, R, fs);
    if (rc != KTF_OK) return rc;
    if (R == 0) return KTF_OK;
    KTF_REQUIRE(R < 65536, "%s: R = %d RIRs, at most 65535 per bank", who, (int)R);
    KTF_REQUIRE(h && offsets_dev && tables && meta && spectra, "%s: null argument", who);
    KTF_REQUIRE(((uintptr_t)spectra & 15) == 0 && ((uintptr_t)tables & 15) == 0, "%s: spectra / tables not 16-byte aligned", who);
    int32_t max_L = 1;
    for (int32_t r = 0; r < R; ++r) max_L = offsets[r + 1] - offsets[r] > max_L ? offsets[r + 1] - offsets[r] : max_L;
    hipStream_t st = (hipStream_t)stream;
    const int npe = early_partitions(fs);
    hipLaunchKernelGGL(aug_rir_peak_kernel, dim3((unsigned)R), dim3(AUG_THREADS), 0, st, h, offsets_dev, (int)R, (int)aug_pre(fs),
                       (int)aug_post(fs), npe, meta);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(aug_rir_spectra_kernel, dim3((unsigned)blocks_of(max_L), (unsigned)R, 2), dim3(AUG_THREADS), 0, st, h, offsets_dev,
                       (const int32_t*)meta, tables, spectra);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int64_t ktf_aug_workspace_bytes(const int32_t* n, const int32_t* rir_ids, int32_t B, const int32_t* rir_lengths, int32_t R,
                                           int32_t fs, int64_t num_additives) {
    const int rc = check_rows("ktf_aug_workspace_bytes", n, rir_ids, B, rir_lengths, R, fs, num_additives);
    if (rc != KTF_OK) return rc;
    return layout_of(n, rir_ids, B, rir_lengths, num_additives).total;
}

extern "C" int ktf_aug_convolve(const void* x, int32_t x_i16, int64_t ldx, const int32_t* n, const int32_t* n_dev, const int32_t* rir_ids,
                                const int32_t* rir_ids_dev, int32_t B, const int32_t* rir_lengths, int32_t R, int32_t fs,
                                const float* h, const int32_t* offsets_dev, const int32_t* meta, const float* spectra, const float* tables,
                                int64_t num_additives, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_aug_convolve";
    int rc = check_rows(who, n, rir_ids, B, rir_lengths, R, fs, num_additives);
    if (rc != KTF_OK) return rc;
    KTF_REQUIRE(ldx >= 0, "%s: negative size (ldx = %lld)", who, (long long)ldx);
    if (B == 0) return KTF_OK;
    KTF_REQUIRE(B < 65536, "%s: B = %d rows, at most 65535 per call (chunk them)", who, (int)B);
    const AugLayout l = layout_of(n, rir_ids, B, rir_lengths, num_additives);
    KTF_REQUIRE(ldx >= l.max_n, "%s: row stride %lld below the longest row (%d)", who, (long long)ldx, (int)l.max_n);
    KTF_REQUIRE(n_dev && rir_ids_dev && stats && workspace && (x || l.max_n == 0), "%s: null argument", who);
    KTF_REQUIRE(!l.any_rir || (h && offsets_dev && meta && spectra && tables),
                "%s: null argument (a row has an RIR: h, offsets_dev, meta, spectra, tables)", who);
    KTF_REQUIRE(!l.any_rir || (((uintptr_t)spectra & 15) == 0 && ((uintptr_t)tables & 15) == 0), "%s: spectra / tables not 16-byte aligned", who);
    rc = ktf_check_workspace(who, workspace, workspace_bytes, l.total);
    if (rc != KTF_OK) return rc;
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    float* y = reinterpret_cast<float*>(ws + l.y);
    float* X = reinterpret_cast<float*>(ws + l.X);
    double* part_before = reinterpret_cast<double*>(ws + l.part);
    double* part_sig = part_before + (int64_t)B * l.S;
    hipStream_t st = (hipStream_t)stream;
    if (l.max_n > 0) {
        const dim3 grid((unsigned)l.nxb, (unsigned)B);
        if (x_i16)
            hipLaunchKernelGGL(aug_forward_kernel<true>, grid, dim3(AUG_THREADS), 0, st, x, ldx, n_dev, rir_ids_dev, tables, y, l.ldy, X, l.nxb,
                               part_before, l.S);
        else
            hipLaunchKernelGGL(aug_forward_kernel<false>, grid, dim3(AUG_THREADS), 0, st, x, ldx, n_dev, rir_ids_dev, tables, y, l.ldy, X, l.nxb,
                               part_before, l.S);
        KTF_CHECK_LAUNCH(who);
        if (l.any_rir) {
            const int64_t ny = blocks_of((int64_t)l.max_n + l.max_L - 1);
            const int64_t nye = blocks_of((int64_t)l.max_n + aug_pre(fs) + aug_post(fs) - 1);
            hipLaunchKernelGGL(aug_conv_kernel<false>, dim3((unsigned)ktf_cdiv(ny, AUG_J), (unsigned)B), dim3(AUG_THREADS), 0, st, n_dev,
                               rir_ids_dev, meta, spectra, tables, (const float*)X, l.nxb, y, l.ldy, part_sig, l.S, x, (int)(x_i16 != 0), ldx,
                               h, offsets_dev);
            KTF_CHECK_LAUNCH(who);
            hipLaunchKernelGGL(aug_conv_kernel<true>, dim3((unsigned)ktf_cdiv(ny < nye ? ny : nye, AUG_J), (unsigned)B), dim3(AUG_THREADS), 0, st,
                               n_dev, rir_ids_dev, meta, spectra, tables, (const float*)X, l.nxb, y, l.ldy, part_sig, l.S, x, (int)(x_i16 != 0), ldx,
                               h, offsets_dev);
            KTF_CHECK_LAUNCH(who);
        }
    }
    hipLaunchKernelGGL(aug_powers_kernel, dim3((unsigned)B), dim3(AUG_THREADS), 0, st, n_dev, rir_ids_dev, meta, (const double*)part_before,
                       (const double*)part_sig, l.S, stats);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_aug_mix(const int32_t* n, const int32_t* n_dev, const int32_t* rir_ids, const int32_t* rir_ids_dev, int32_t B,
                           const int32_t* rir_lengths, int32_t R, int32_t fs, const int32_t* meta, const int32_t* add_offsets,
                           const int32_t* add_offsets_dev, const KtfAugAdditive* adds, const KtfAugAdditive* adds_dev, const float* noise,
                           const int64_t* noise_offsets, const int64_t* noise_offsets_dev, int32_t M, int32_t shift_output,
                           int32_t normalize_output, double volume, void* out, int32_t out_i16, int64_t ldo, int64_t T_out, double* stats,
                           void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_aug_mix";
    KTF_REQUIRE(B < 0 || add_offsets, "%s: null argument", who);
    const int64_t A = (B >= 0 && add_offsets) ? (int64_t)add_offsets[B] : 0;
    int rc = check_rows(who, n, rir_ids, B, rir_lengths, R, fs, A);
    if (rc != KTF_OK) return rc;
    KTF_REQUIRE(M >= 0 && ldo >= 0 && T_out >= 0, "%s: negative size (M = %d, ldo = %lld, T_out = %lld)", who, (int)M, (long long)ldo,
                (long long)T_out);
    KTF_REQUIRE(isfinite(volume), "%s: volume is not finite", who);
    KTF_REQUIRE(add_offsets[0] == 0, "%s: add_offsets[0] = %d, must be 0", who, (int)add_offsets[0]);
    for (int32_t b = 0; b < B; ++b)
        KTF_REQUIRE(add_offsets[b + 1] >= add_offsets[b], "%s: add_offsets must not descend (row %d)", who, (int)b);
    KTF_REQUIRE(A == 0 || (adds && noise_offsets), "%s: null argument", who);
    if (M > 0 || A > 0) {
        KTF_REQUIRE(noise_offsets, "%s: null argument", who);
        KTF_REQUIRE(noise_offsets[0] == 0, "%s: noise_offsets[0] must be 0", who);
        for (int32_t i = 0; i < M; ++i)
            KTF_REQUIRE(noise_offsets[i + 1] > noise_offsets[i], "%s: noise %d has no samples (offsets must ascend)", who, (int)i);
    }
    for (int64_t a = 0; a < A; ++a) {
        KTF_REQUIRE(adds[a].noise >= 0 && adds[a].noise < M, "%s: additive %lld: noise id %d out of range (0 .. %d)", who, (long long)a,
                    (int)adds[a].noise, (int)M - 1);
        KTF_REQUIRE(isfinite(adds[a].snr_db), "%s: additive %lld: snr_db is not finite", who, (long long)a);
        KTF_REQUIRE(adds[a].start >= 0, "%s: additive %lld: start o = %d < 0", who, (long long)a, (int)adds[a].start);
        KTF_REQUIRE(adds[a].duration >= 0, "%s: additive %lld: negative size (duration %d)", who, (long long)a, (int)adds[a].duration);
    }
    if (B == 0) return KTF_OK;
    KTF_REQUIRE(B < 65536, "%s: B = %d rows, at most 65535 per call (chunk them)", who, (int)B);
    const AugLayout l = layout_of(n, rir_ids, B, rir_lengths, A);
    int64_t max_out = 0;
    for (int32_t b = 0; b < B; ++b) {
        const int64_t len = (shift_output || n[b] == 0 || rir_ids[b] < 0) ? n[b] : (int64_t)n[b] + rir_lengths[rir_ids[b]] - 1;
        max_out = len > max_out ? len : max_out;
    }
    KTF_REQUIRE(T_out >= max_out && ldo >= T_out, "%s: T_out = %lld, ldo = %lld: need ldo >= T_out >= %lld (the longest output row)", who,
                (long long)T_out, (long long)ldo, (long long)max_out);
    KTF_REQUIRE(n_dev && rir_ids_dev && add_offsets_dev && stats && workspace && (out || T_out == 0), "%s: null argument", who);
    KTF_REQUIRE(A == 0 || (adds_dev && noise && noise_offsets_dev), "%s: null argument", who);
    KTF_REQUIRE(!l.any_rir || meta, "%s: null argument (a row has an RIR: meta)", who);
    rc = ktf_check_workspace(who, workspace, workspace_bytes, l.total);
    if (rc != KTF_OK) return rc;
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    float* y = reinterpret_cast<float*>(ws + l.y);
    double* part_after = reinterpret_cast<double*>(ws + l.part) + 2 * (int64_t)B * l.S;
    double* gains = reinterpret_cast<double*>(ws + l.gains);
    hipStream_t st = (hipStream_t)stream;
    if (A > 0) {
        hipLaunchKernelGGL(aug_gains_kernel, dim3((unsigned)B), dim3(AUG_THREADS), 0, st, add_offsets_dev, adds_dev, noise, noise_offsets_dev,
                           (const double*)stats, gains);
        KTF_CHECK_LAUNCH(who);
    }
    if (l.max_n > 0) {
        hipLaunchKernelGGL(aug_add_kernel, dim3((unsigned)l.S, (unsigned)B), dim3(AUG_THREADS), 0, st, n_dev, rir_ids_dev, meta, add_offsets_dev,
                           adds_dev, noise, noise_offsets_dev, (const double*)gains, y, l.ldy, part_after, l.S);
        KTF_CHECK_LAUNCH(who);
    }
    hipLaunchKernelGGL(aug_scale_kernel, dim3((unsigned)B), dim3(AUG_THREADS), 0, st, n_dev, rir_ids_dev, meta, (const double*)part_after, l.S,
                       (int)(normalize_output != 0), volume, stats);
    KTF_CHECK_LAUNCH(who);
    if (T_out > 0) {
        const dim3 grid((unsigned)blocks_of(T_out), (unsigned)B);
        if (out_i16)
            hipLaunchKernelGGL(aug_write_kernel<true>, grid, dim3(AUG_THREADS), 0, st, n_dev, rir_ids_dev, meta, (const float*)y, l.ldy,
                               (const double*)stats, (int)(shift_output != 0), out, ldo, T_out);
        else
            hipLaunchKernelGGL(aug_write_kernel<false>, grid, dim3(AUG_THREADS), 0, st, n_dev, rir_ids_dev, meta, (const float*)y, l.ldy,
                               (const double*)stats, (int)(shift_output != 0), out, ldo, T_out);
        KTF_CHECK_LAUNCH(who);
    }
    return KTF_OK;
}
