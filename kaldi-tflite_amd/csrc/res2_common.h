// What res2_conv.hip (forward) and res2_grad.hip (backward) share: the fragment types, the 16-byte accessors that fall back to scalar
// accesses on a base that is not 16-byte aligned, the in-register bf16 round / split, and the shape check of include/ktf_res2.h rule 6.
#ifndef KTF_RES2_COMMON_H_
#define KTF_RES2_COMMON_H_

#include "common.h"
#include "../../include/ktf_res2.h"

#define R2_THREADS 512
#define R2_LDS_BYTES 163840      // gfx950: 160 KiB per workgroup
#define R2_MAX_TILE 128

static inline int r2_check_shape(const char* who, int32_t width, int32_t scale, int32_t dilation, int32_t gemm) {
    KTF_REQUIRE(scale >= 2 && scale <= 8, "%s: scale %d outside [2, 8]", who, (int)scale);
    KTF_REQUIRE(width >= 16 && width <= 128 && width % 16 == 0, "%s: group width %d is not a multiple of 16 in [16, 128]", who, (int)width);
    KTF_REQUIRE(dilation >= 1 && dilation <= 8, "%s: dilation %d outside [1, 8]", who, (int)dilation);
    KTF_REQUIRE(gemm == KTF_GEMM_F32 || gemm == KTF_GEMM_BF16 || gemm == KTF_GEMM_BF16X3, "%s: gemm %d is not KTF_GEMM_F32, _BF16 or _BF16X3", who,
                (int)gemm);
    return KTF_OK;
}

// B, T, C and the shape of every entry point that takes rows (rule 6); the group width comes back
static inline int r2_check_sizes(const char* who, int64_t B, int64_t T, int32_t C, int32_t scale, int32_t dilation, int32_t gemm, int32_t* wd) {
    KTF_REQUIRE(B >= 0 && T >= 0 && C > 0, "%s: negative size (B %lld, T %lld, C %d)", who, (long long)B, (long long)T, (int)C);
    KTF_REQUIRE(B <= KTF_RES2_MAX_BATCH && T <= KTF_RES2_MAX_ROWS, "%s: B %lld above %d or T %lld above %d", who, (long long)B, KTF_RES2_MAX_BATCH,
                (long long)T, KTF_RES2_MAX_ROWS);
    KTF_REQUIRE(scale >= 2 && scale <= 8, "%s: scale %d outside [2, 8]", who, (int)scale);
    KTF_REQUIRE(C % scale == 0, "%s: C %% scale != 0 (C %d, scale %d)", who, (int)C, (int)scale);
    *wd = C / scale;
    return r2_check_shape(who, *wd, scale, dilation, gemm);
}

#ifdef __HIPCC__
typedef __attribute__((ext_vector_type(8))) __bf16 r2_bfrag8;
typedef __attribute__((ext_vector_type(4))) unsigned r2_u32x4;
typedef __attribute__((ext_vector_type(4))) float r2_fv4;

__device__ __forceinline__ r2_fv4 r2_load4(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const r2_fv4*>(p);
    return r2_fv4{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ void r2_store4(float* p, r2_fv4 v, bool vec) {
    if (vec) {
        *reinterpret_cast<r2_fv4*>(p) = v;
    } else {
        p[0] = v[0], p[1] = v[1], p[2] = v[2], p[3] = v[3];
    }
}

// eight fp32 -> the lane's bf16 fragment: hi = bf16(v), round to nearest even; X3: lo = bf16(v - hi)
template <bool X3>
__device__ __forceinline__ void r2_split8(const float (&v)[8], r2_bfrag8& hi, r2_bfrag8& lo) {
    r2_u32x4 h, l = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned short h0 = f2bf(v[2 * i]), h1 = f2bf(v[2 * i + 1]);
        h[i] = (unsigned)h0 | ((unsigned)h1 << 16);
        if (X3) l[i] = (unsigned)f2bf(v[2 * i] - bf2f(h0)) | ((unsigned)f2bf(v[2 * i + 1] - bf2f(h1)) << 16);
    }
    hi = __builtin_bit_cast(r2_bfrag8, h);
    lo = __builtin_bit_cast(r2_bfrag8, l);
}
#endif
#endif
