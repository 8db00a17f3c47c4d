// VB-HMM resegmentation of diarization output (Diez / Burget's VB diarization with an i-vector subspace, as Kaldi's
// diarization/VB_resegmentation.sh runs it), batched over the recordings of one call. Frames of all recordings lie end to end:
// recording r owns rows [offsets[r], offsets[r + 1]) of x and blocks [boffsets[r], boffsets[r + 1]) of q / lls; block b of a
// recording covers its frames [b d, (b + 1) d) with d = downsample. The posteriors are in vb_post.hip, the speakers' statistics,
// update and block log-likelihoods in vb_speaker.hip, forward-backward and the bound in vb_fb.hip; here is what they share.
// Every stage is per recording with a fixed reduction order: a recording's bits do not depend on its batch or position.
#pragma once
#include "common.h"

constexpr int FBC = KTF_VB_FB_CHUNK;
constexpr int FBK = KTF_VB_MAX_SPEAKERS;

// the recording that owns block (or chunk) w of the ascending table `tab` (N + 1 entries): the last r with tab[r] <= w; -1 beyond
__device__ __forceinline__ int vb_owner(const int* __restrict__ tab, int N, int64_t w) {
    if (w < tab[0] || w >= tab[N]) return -1;
    int lo = 0, hi = N;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab[mid] <= w) lo = mid;
        else hi = mid;
    }
    return lo;
}

inline int vb_check_tables(const char* who, int64_t F, int32_t D, int64_t ldx, int32_t N, int64_t TB, int32_t downsample, int32_t K) {
    KTF_REQUIRE(F >= 0 && F < ((int64_t)1 << 31), "%s: frame count %lld out of range", who, (long long)F);
    KTF_REQUIRE(D >= 1 && D <= KTF_IVECTOR_MAX_FEAT_DIM, "%s: feature dim %d outside 1 .. %d", who, (int)D, KTF_IVECTOR_MAX_FEAT_DIM);
    KTF_REQUIRE(ldx >= D, "%s: ldx %lld < D %d", who, (long long)ldx, (int)D);
    KTF_REQUIRE(N >= 1 && N <= 65535, "%s: %d recordings outside 1 .. 65535", who, (int)N);
    KTF_REQUIRE(TB >= 0 && TB <= F, "%s: %lld blocks for %lld frames", who, (long long)TB, (long long)F);
    KTF_REQUIRE(downsample >= 1, "%s: downsample %d < 1", who, (int)downsample);
    KTF_REQUIRE(K >= 1 && K <= KTF_VB_MAX_SPEAKERS, "%s: %d speakers outside 1 .. %d", who, (int)K, KTF_VB_MAX_SPEAKERS);
    return KTF_OK;
}
