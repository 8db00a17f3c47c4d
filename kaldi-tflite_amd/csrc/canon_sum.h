// The one order of a sum over the frames of an utterance (include/ktf_attn.h rule 8, include/ktf_se.h rule 2), shared by
// attn_pool.hip and se_gate.hip: row t goes to group t mod 64, a group adds its rows in ascending order from +0, and ap_total
// combines the groups as ((g + g+16) + g+32) + g+48 for g = 0..15, then in ascending g. stats_pool_kernel (pool_post.hip) spells
// the same association out in place.
#pragma once
#include "common.h"

// the canonical total of one column of red[RG][..][CW] (slot g of RG at r[g * stride]); RG = 16: the slots are already the sums of
// their four groups
template <int RG>
__device__ __forceinline__ double ap_total(const double* r, int stride) {
    double s = 0.;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        if (RG == 16) s += r[g * stride];
        else s += ((r[g * stride] + r[(g + 16) * stride]) + r[(g + 32) * stride]) + r[(g + 48) * stride];
    }
    return s;
}

__device__ __forceinline__ int ap_len(const int32_t* lens, int b, int64_t T) {
    int len = lens ? lens[b] : (int)T;
    return len < 0 ? 0 : (len > (int)T ? (int)T : len);
}
