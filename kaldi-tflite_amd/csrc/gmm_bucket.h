// Stable bucketing of (frame, slot) pairs by Gaussian, shared by the second-order statistics of ivector_train.hip and the GMM
// statistics of gmm_train.hip: integer histograms per chunk of SEC_CH pairs, exclusive scans, then one wave per chunk that ranks
// equal Gaussians by lane order. A bucket lists its pairs in ascending pair id, so a sum taken over it row after row has the same
// bits on every run. Every translation unit that includes this gets its own copy of the kernels.
#pragma once
#include "common.h"

namespace {

constexpr int SEC_CH = 8192;        // pairs per bucketing chunk (one wave scatters a chunk in pair order)

inline int64_t sec_al256(int64_t b) { return (b + 255) & ~(int64_t)255; }

struct SecLayout {
    int64_t counts, total, start, pairs, bytes;
    int64_t nch;
};

SecLayout sec_layout(int64_t F, int64_t I, int64_t n) {
    SecLayout l;
    const int64_t np = F * n;
    l.nch = (np + SEC_CH - 1) / SEC_CH;
    int64_t at = 0;
    l.counts = at; at += sec_al256(l.nch * I * 4);
    l.total = at;  at += sec_al256(I * 4);
    l.start = at;  at += sec_al256((I + 1) * 4);
    l.pairs = at;  at += sec_al256(np * 4);
    l.bytes = at;
    return l;
}

// counts[chunk][g] = the chunk's pairs of Gaussian g (integer counts: the LDS atomics cannot change the result)
__global__ void __launch_bounds__(256) sec_hist_kernel(const int* __restrict__ gauss, int64_t np, int I, int* __restrict__ counts) {
    extern __shared__ int sec_lds[];
    const int tid = threadIdx.x;
    for (int g = tid; g < I; g += 256) sec_lds[g] = 0;
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * SEC_CH;
    for (int64_t e = e0 + tid; e < e0 + SEC_CH && e < np; e += 256) {
        const int g = gauss[e];
        if (g >= 0 && g < I) atomicAdd(&sec_lds[g], 1);
    }
    __syncthreads();
    for (int g = tid; g < I; g += 256) counts[(int64_t)blockIdx.x * I + g] = sec_lds[g];
}

// counts[chunk][g] -> the pairs of g in earlier chunks; total[g]
__global__ void sec_scan_kernel(int* __restrict__ counts, int64_t nch, int I, int* __restrict__ total) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= I) return;
    int run = 0;
    for (int64_t c = 0; c < nch; ++c) {
        const int v = counts[c * I + g];
        counts[c * I + g] = run;
        run += v;
    }
    total[g] = run;
}

// start[g] = sum of total[< g], start[I] = all pairs kept (one workgroup)
__global__ void __launch_bounds__(256) sec_start_kernel(const int* __restrict__ total, int I, int* __restrict__ start) {
    __shared__ int seg[256];
    const int tid = threadIdx.x, per = (I + 255) / 256;
    const int g0 = tid * per, g1 = g0 + per < I ? g0 + per : I;
    int s = 0;
    for (int g = g0; g < g1; ++g) s += total[g];
    seg[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) {
            const int v = seg[t];
            seg[t] = run;
            run += v;
        }
        start[I] = run;
    }
    __syncthreads();
    int run = seg[tid];
    for (int g = g0; g < g1; ++g) {
        start[g] = run;
        run += total[g];
    }
}

// one wave per chunk, 64 pairs per step in pair order: a pair's slot is its bucket's cursor + the number of lower lanes with the
// same Gaussian, and the highest such lane moves the cursor on. Every slot index is < start[I] <= np by the counts above.
__global__ void __launch_bounds__(64) sec_scatter_kernel(const int* __restrict__ gauss, int64_t np, int I, const int* __restrict__ counts,
                                                          const int* __restrict__ start, int* __restrict__ pairs) {
    extern __shared__ int sec_lds[];
    const int lane = threadIdx.x;
    for (int g = lane; g < I; g += 64) sec_lds[g] = start[g] + counts[(int64_t)blockIdx.x * I + g];
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * SEC_CH;
    for (int64_t eb = e0; eb < e0 + SEC_CH && eb < np; eb += 64) {
        const int64_t e = eb + lane;
        int g = e < np ? gauss[e] : -1;
        if (g >= I) g = -1;
        int rank = 0;
        bool later = false;
        for (int j = 0; j < 64; ++j) {
            const int gj = __shfl(g, j);
            if (gj == g) {
                rank += j < lane;
                later |= j > lane;
            }
        }
        int pos = 0;
        if (g >= 0) {
            pos = sec_lds[g] + rank;
            pairs[pos] = (int)e;
        }
        __syncthreads();
        if (g >= 0 && !later) sec_lds[g] = pos + 1;
        __syncthreads();
    }
}

// The four launches: start[g] .. start[g + 1] of `pairs` then lists the pairs of Gaussian g (gauss outside [0, I) dropped).
int sec_bucket(const char* who, const int* gauss, int64_t np, int I, const SecLayout& l, char* ws, hipStream_t st) {
    int* counts = (int*)(ws + l.counts);
    int* total = (int*)(ws + l.total);
    int* start = (int*)(ws + l.start);
    int* pairs = (int*)(ws + l.pairs);
    const size_t lds = (size_t)I * sizeof(int);
    hipLaunchKernelGGL(sec_hist_kernel, dim3((unsigned)l.nch), dim3(256), lds, st, gauss, np, I, counts);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(sec_scan_kernel, dim3(ktf_cdiv(I, 256)), dim3(256), 0, st, counts, l.nch, I, total);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(sec_start_kernel, dim3(1), dim3(256), 0, st, (const int*)total, I, start);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(sec_scatter_kernel, dim3((unsigned)l.nch), dim3(64), lds, st, gauss, np, I, (const int*)counts, (const int*)start,
                       pairs);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

}  // namespace
