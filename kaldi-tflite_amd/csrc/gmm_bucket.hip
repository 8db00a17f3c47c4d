// The bucketing of gmm_bucket.h: a counting sort of (frame, slot) pairs by Gaussian, and the cut of buckets into work items.
// Integer counts throughout: no atomic can change a result.
#include "gmm_bucket.h"

namespace {

// counts[chunk][g] = the chunk's pairs of Gaussian g (integer counts: the LDS atomics cannot change the result)
__global__ void __launch_bounds__(256) sec_hist_kernel(const int* __restrict__ gauss, int64_t np, int I, int ch, int* __restrict__ counts) {
    extern __shared__ int sec_lds[];
    const int tid = threadIdx.x;
    for (int g = tid; g < I; g += 256) sec_lds[g] = 0;
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * ch;
    for (int64_t e = e0 + tid; e < e0 + ch && e < np; e += 256) {
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

// 256 threads per chunk: a pair's slot is its bucket's cursor, an LDS counter, so the order inside a chunk's share of a bucket is
// whatever the atomics give. Every slot index is < start[I] <= np by the counts above.
__global__ void __launch_bounds__(256) sec_scatter_any_kernel(const int* __restrict__ gauss, int64_t np, int I, const int* __restrict__ counts,
                                                              const int* __restrict__ start, int* __restrict__ pairs) {
    extern __shared__ int sec_lds[];
    const int tid = threadIdx.x;
    for (int g = tid; g < I; g += 256) sec_lds[g] = start[g] + counts[(int64_t)blockIdx.x * I + g];
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * SEC_CH_ANY;
    for (int64_t e = e0 + tid; e < e0 + SEC_CH_ANY && e < np; e += 256) {
        const int g = gauss[e];
        if (g >= 0 && g < I) pairs[atomicAdd(&sec_lds[g], 1)] = (int)e;
    }
}

// buckets cut into items of `rows` rows: istart and (nullable) pstart as gmm_bucket.h states them (one workgroup)
__global__ void __launch_bounds__(256) bucket_items_kernel(const int* __restrict__ start, int I, int rows, int* __restrict__ istart,
                                                           int* __restrict__ pstart) {
    __shared__ int si[256];
    __shared__ int sp[256];
    const int tid = threadIdx.x, per = (I + 255) / 256;
    const int g0 = tid * per < I ? tid * per : I, g1 = g0 + per < I ? g0 + per : I;
    int a = 0, b = 0;
    for (int g = g0; g < g1; ++g) {
        const int it = (start[g + 1] - start[g] + rows - 1) / rows;
        a += it;
        b += it > 1 ? it : 0;
    }
    si[tid] = a;
    sp[tid] = b;
    __syncthreads();
    if (tid == 0) {
        int ra = 0, rb = 0;
        for (int t = 0; t < 256; ++t) {
            const int va = si[t], vb = sp[t];
            si[t] = ra;
            sp[t] = rb;
            ra += va;
            rb += vb;
        }
        istart[I] = ra;
        if (pstart) pstart[I] = rb;
    }
    __syncthreads();
    a = si[tid];
    b = sp[tid];
    for (int g = g0; g < g1; ++g) {
        const int it = (start[g + 1] - start[g] + rows - 1) / rows;
        istart[g] = a;
        if (pstart) pstart[g] = b;
        a += it;
        b += it > 1 ? it : 0;
    }
}

}  // namespace

int bucket_check_pairs(const char* who, int64_t F, int32_t I, int32_t n) {
    KTF_REQUIRE(I >= 1 && I <= KTF_IVECTOR_MAX_GAUSS, "%s: %d Gaussians outside 1 .. %d", who, (int)I, KTF_IVECTOR_MAX_GAUSS);
    KTF_REQUIRE(n >= 1 && n <= KTF_IVECTOR_MAX_GSELECT, "%s: %d slots per frame outside 1 .. %d", who, (int)n, KTF_IVECTOR_MAX_GSELECT);
    // (F < 2^31 follows from F * n < 2^31 in exact arithmetic; stated first, it keeps the product inside an int64)
    KTF_REQUIRE(F >= 0 && F < ((int64_t)1 << 31) && F * n < ((int64_t)1 << 31), "%s: frame count %lld out of range (F * n < 2^31)", who,
                (long long)F);
    return KTF_OK;
}

int bucket_check_shape(const char* who, int64_t F, int32_t I, int32_t D, int32_t n) {
    KTF_REQUIRE(D >= 1 && D <= KTF_IVECTOR_MAX_FEAT_DIM, "%s: feature dim %d outside 1 .. %d", who, (int)D, KTF_IVECTOR_MAX_FEAT_DIM);
    return bucket_check_pairs(who, F, I, n);
}

int sec_bucket(const char* who, const int* gauss, int64_t np, int I, const SecLayout& l, char* ws, hipStream_t st) {
    int* counts = (int*)(ws + l.counts);
    int* total = (int*)(ws + l.total);
    int* start = (int*)(ws + l.start);
    int* pairs = (int*)(ws + l.pairs);
    const size_t lds = (size_t)I * sizeof(int);
    hipLaunchKernelGGL(sec_hist_kernel, dim3((unsigned)l.nch), dim3(256), lds, st, gauss, np, I, l.ordered ? SEC_CH : SEC_CH_ANY, counts);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(sec_scan_kernel, dim3(ktf_cdiv(I, 256)), dim3(256), 0, st, counts, l.nch, I, total);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(sec_start_kernel, dim3(1), dim3(256), 0, st, (const int*)total, I, start);
    KTF_CHECK_LAUNCH(who);
    if (l.ordered)
        hipLaunchKernelGGL(sec_scatter_kernel, dim3((unsigned)l.nch), dim3(64), lds, st, gauss, np, I, (const int*)counts,
                           (const int*)start, pairs);
    else
        hipLaunchKernelGGL(sec_scatter_any_kernel, dim3((unsigned)l.nch), dim3(256), lds, st, gauss, np, I, (const int*)counts,
                           (const int*)start, pairs);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

int bucket_items(const char* who, const int* start, int I, int rows, int* istart, int* pstart, hipStream_t st) {
    hipLaunchKernelGGL(bucket_items_kernel, dim3(1), dim3(256), 0, st, start, I, rows, istart, pstart);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
