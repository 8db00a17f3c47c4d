// The transform of the partitioned convolution (augment.hip): a 2P-point real FFT run as a P-point complex Stockham radix-4 FFT in
// LDS by one 256-thread workgroup (P = 1024: five stages, one butterfly per thread and stage, a barrier between stages), and the
// passes between the complex transform and the packed real spectrum.
//
// Packed spectrum of a real a[0 .. 2P): S[0] = (A[0], A[P]) (both real), S[k] = A[k] for 0 < k < P.
// LDS buffers hold P float2 at index PADI(i) = i + (i >> 4): the stage writes are strided by 4 s points, and one extra slot per 16
// spreads the first stage's 16 lanes of a ds_write_b64 group over 16 distinct bank pairs (unpadded they fall on 4). That is reasoning
// from the bank rules; no conflict counter was read with and without the padding.
#pragma once
#include "common.h"
#include "../../include/ktf_augment.h"

#define AUG_P KTF_AUG_PARTITION
#define AUG_THREADS 256
#define AUG_BUF (AUG_P + AUG_P / 16)        // float2 slots of a padded buffer
#define AUG_TABLE_FLOATS (4 * AUG_P)        // W_P^k, k < P, then W_2P^k, k < P (float2 each)

static_assert(AUG_P == 4 * AUG_THREADS, "one radix-4 butterfly per thread and stage");
static_assert(AUG_P == 1024, "five radix-4 stages");

__device__ __forceinline__ int PADI(int i) { return i + (i >> 4); }

__device__ __forceinline__ float2 aug_cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// the tables -> LDS (tw: 2P float2); the caller's next barrier publishes them
__device__ __forceinline__ void aug_load_tables(const float* __restrict__ tables, float2* tw, int tid) {
    const float4* src = reinterpret_cast<const float4*>(tables);
    float4* dst = reinterpret_cast<float4*>(tw);
    for (int i = tid; i < AUG_TABLE_FLOATS / 4; i += AUG_THREADS) dst[i] = src[i];
}

// Forward P-point FFT of a (written by the workgroup, no barrier yet) -> b. Five stages a -> b -> a -> b -> a -> b; ends with a
// barrier: b is readable, a is free. W[k] = exp(-2 pi i k / P).
__device__ __forceinline__ void aug_fft(float2* a, float2* b, const float2* __restrict__ W, int tid) {
    float2* x = a;
    float2* y = b;
    __syncthreads();
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        const int ls = 2 * st, s = 1 << ls;
        const int n1 = (AUG_P >> ls) >> 2;                       // a quarter of the current sub-transform size
        const int p = tid >> ls, q = tid & (s - 1);
        const float2 va = x[PADI(q + s * p)], vb = x[PADI(q + s * (p + n1))], vc = x[PADI(q + s * (p + 2 * n1))],
                     vd = x[PADI(q + s * (p + 3 * n1))];
        const float2 w1 = W[p * s], w2 = W[2 * p * s], w3 = W[3 * p * s];
        const float2 apc = make_float2(va.x + vc.x, va.y + vc.y), amc = make_float2(va.x - vc.x, va.y - vc.y);
        const float2 bpd = make_float2(vb.x + vd.x, vb.y + vd.y);
        const float2 jbmd = make_float2(-(vb.y - vd.y), vb.x - vd.x);          // i (b - d)
        y[PADI(q + s * (4 * p + 0))] = make_float2(apc.x + bpd.x, apc.y + bpd.y);
        y[PADI(q + s * (4 * p + 1))] = aug_cmul(w1, make_float2(amc.x - jbmd.x, amc.y - jbmd.y));
        y[PADI(q + s * (4 * p + 2))] = aug_cmul(w2, make_float2(apc.x - bpd.x, apc.y - bpd.y));
        y[PADI(q + s * (4 * p + 3))] = aug_cmul(w3, make_float2(amc.x + jbmd.x, amc.y + jbmd.y));
        __syncthreads();
        float2* t = x;
        x = y;
        y = t;
    }
}

// Z = FFT_P(z), z[m] = a[2m] + i a[2m + 1], in LDS buffer zb -> the packed spectrum of a, to global memory. WN[k] = exp(-pi i k / P).
__device__ __forceinline__ void aug_real_spectrum(const float2* zb, const float2* __restrict__ WN, float2* __restrict__ out, int tid) {
    for (int k = tid; k <= AUG_P / 2; k += AUG_THREADS) {
        if (k == 0) {
            const float2 z0 = zb[0];
            out[0] = make_float2(z0.x + z0.y, z0.x - z0.y);
            continue;
        }
        const float2 u = zb[PADI(k)], v = zb[PADI(AUG_P - k)];
        const float2 e = make_float2(0.5f * (u.x + v.x), 0.5f * (u.y - v.y));          // (Z[k] + conj Z[P-k]) / 2
        const float2 o = make_float2(0.5f * (u.y + v.y), -0.5f * (u.x - v.x));         // (Z[k] - conj Z[P-k]) / 2i
        const float2 wo = aug_cmul(WN[k], o);
        out[k] = make_float2(e.x + wo.x, e.y + wo.y);
        if (k != AUG_P / 2) out[AUG_P - k] = make_float2(e.x - wo.x, -(e.y - wo.y));   // conj(E - w O)
    }
}

// The packed spectrum Y in LDS buffer yb -> conj(Z') in zb, Z' the P-point spectrum whose inverse transform holds the real signal's
// even samples in its real and the odd ones in its imaginary part; a forward aug_fft of zb then gives conj(P z').
__device__ __forceinline__ void aug_real_spectrum_inv(const float2* yb, float2* zb, const float2* __restrict__ WN, int tid) {
    for (int k = tid; k <= AUG_P / 2; k += AUG_THREADS) {
        if (k == 0) {
            const float2 y0 = yb[0];
            zb[0] = make_float2(0.5f * (y0.x + y0.y), -0.5f * (y0.x - y0.y));
            continue;
        }
        const float2 u = yb[PADI(k)], v = yb[PADI(AUG_P - k)];
        const float2 e = make_float2(0.5f * (u.x + v.x), 0.5f * (u.y - v.y));          // (Y[k] + conj Y[P-k]) / 2
        const float2 d = make_float2(0.5f * (u.x - v.x), 0.5f * (u.y + v.y));          // (Y[k] - conj Y[P-k]) / 2
        const float2 w = WN[k];
        const float2 o = aug_cmul(make_float2(w.x, -w.y), d);                          // ... times W_2P^-k
        // Z'[k] = E + i O, Z'[P-k] = conj(E) + i conj(O); stored conjugated
        zb[PADI(k)] = make_float2(e.x - o.y, -(e.y + o.x));
        if (k != AUG_P / 2) zb[PADI(AUG_P - k)] = make_float2(e.x + o.y, -(o.x - e.y));
    }
}

// the workgroup's sum of v in a fixed order: wave butterflies, then the four wave sums in order (red: 4 doubles of LDS)
__device__ __forceinline__ double aug_block_sum(double v, double* red, int tid) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
