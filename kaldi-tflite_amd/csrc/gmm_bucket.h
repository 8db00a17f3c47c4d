// Bucketing of (frame, slot) pairs by Gaussian (gmm_bucket.hip), shared by the full-covariance posteriors of fgmm.hip, the GMM
// statistics of gmm_train.hip and the second-order statistics of ivector_train.hip: a counting sort with integer histograms per
// chunk of pairs, exclusive scans and a scatter per chunk. The ordered scatter (one wave per chunk of SEC_CH pairs, equal Gaussians
// ranked by lane order) is stable: a bucket lists its pairs in ascending pair id, so a sum taken over it row after row has the same
// bits on every run. The unordered one (256 threads per chunk of SEC_CH_ANY pairs, LDS counters) is faster and leaves the order
// inside a chunk's share of a bucket to the atomics: for clients that compute every pair's value alone. A bucket may then be cut
// into work items of a fixed number of rows, one workgroup each, so that a popular Gaussian is spread over workgroups.
#pragma once
#include "common.h"

constexpr int SEC_CH = 8192;        // pairs per chunk of the ordered scatter (one wave walks a chunk in pair order)
constexpr int SEC_CH_ANY = 32768;   // pairs per chunk of the unordered scatter

struct SecLayout {
    int64_t counts, total, start, pairs, bytes;
    int64_t nch;
    bool ordered;
};

inline SecLayout sec_layout(int64_t F, int64_t I, int64_t n, bool ordered) {
    SecLayout l;
    const int64_t np = F * n;
    l.ordered = ordered;
    l.nch = ordered ? (np + SEC_CH - 1) / SEC_CH : (np + SEC_CH_ANY - 1) / SEC_CH_ANY;
    int64_t at = 0;
    l.counts = at; at += al256(l.nch * I * 4);
    l.total = at;  at += al256(I * 4);
    l.start = at;  at += al256((I + 1) * 4);
    l.pairs = at;  at += al256(np * 4);
    l.bytes = at;
    return l;
}

// I, n and F * n within what the bucketing indexes with an int; bucket_check_shape: the feature dim as well
int bucket_check_pairs(const char* who, int64_t F, int32_t I, int32_t n);
int bucket_check_shape(const char* who, int64_t F, int32_t I, int32_t D, int32_t n);

// Four launches: start[g] .. start[g + 1] of `pairs` (both in ws, at l.start and l.pairs) then lists the pairs of Gaussian g
// (gauss outside [0, I) dropped), in ascending pair id if l.ordered.
int sec_bucket(const char* who, const int* gauss, int64_t np, int I, const SecLayout& l, char* ws, hipStream_t st);

// One launch: istart[g] = sum_{h < g} ceil(cnt_h / rows) with cnt_h = start[h + 1] - start[h] and, unless pstart is null,
// pstart[g] = the same sum over the Gaussians with more than one item; entry I holds the totals. At most np / rows + I items.
int bucket_items(const char* who, const int* start, int I, int rows, int* istart, int* pstart, hipStream_t st);

struct BucketItem {
    int g, r0, r1, k, items;        // Gaussian, bucket rows [r0, r1), the item's index within its Gaussian and that Gaussian's items
};

// item w -> its Gaussian and rows; g = -1 beyond the last item
__device__ __forceinline__ BucketItem bucket_item(int w, const int* __restrict__ start, const int* __restrict__ istart, int I, int rows) {
    BucketItem it;
    it.g = -1;
    it.r0 = it.r1 = it.k = it.items = 0;
    if (w >= istart[I]) return it;
    int lo = 0, hi = I;                          // istart[lo] <= w < istart[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (istart[mid] <= w) lo = mid;
        else hi = mid;
    }
    it.g = lo;
    it.k = w - istart[lo];
    it.items = istart[lo + 1] - istart[lo];
    it.r0 = start[lo] + it.k * rows;
    it.r1 = it.r0 + rows < start[lo + 1] ? it.r0 + rows : start[lo + 1];
    return it;
}
