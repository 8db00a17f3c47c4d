// The Res2Net dilated convolution in one launch (include/ktf_res2.h states the contract as numbered rules, INTEGRATION.md section 2s the
// use, DESIGN.md section 7 the design and the measurements): scale - 1 grouped convolutions of three taps at distance d, each fed by the
// one before it, on a row tile with a halo that carries all groups through LDS. x is read once, y written once.
//
// Work split. A workgroup of eight waves owns R output rows [t0, t0 + R) of one utterance (grid: x = tile, y = utterance; a tile at or
// beyond len_b exits at once) and walks the stages j = 1 .. s - 1 in order. Stage j computes Y_j on the extent [t0 - h_j, t0 + R + h_j),
// h_j = (s - 1 - j) d: the tile plus the halo the later stages will still read, cut to [0, len_b). A wave takes units of 32 rows (two
// 16-row blocks that share every W fragment) and all wd output columns, so a stage needs one barrier, at its end.
//
// LDS. Two row buffers of NR = R + 2 (s - 1) d rows of wd + 4 floats ping-pong: buffer row i is frame t0 - (s - 1) d + i. Stage j reads
// U_j from one and its epilogue writes U_{j+1} = Y_j + X_{j+1} into the other (X_{j+1} comes from global memory there; Y_j goes to y
// for the tile's own rows). Row indices are clamped to [0, len_b) where the fragments are READ, never where rows are stored, so a tile
// at an utterance's edge holds and needs nothing outside [max(t0 - halo, 0), min(t0 + R + halo, len_b)). The pitch wd + 4 puts the
// sixteen rows of a 16-byte fragment read on sixteen disjoint sets of four banks.
//
// Matrix instructions. The blocks are transposed: W is the first operand (M = output channel), U the second (N = row), so a lane of the
// 16 x 16 accumulator holds FOUR CHANNELS of ONE row. Output channel c = m NCB + cb for the m-th row of block cb (NCB = wd / 16 blocks):
// lane (n = lane & 15, h = lane >> 4) then owns the 4 NCB CONSECUTIVE channels from 4 h NCB of row n -- its stores to LDS and to y are
// 16-byte pieces of one contiguous run -- and its W fragment for all NCB blocks is NCB consecutive floats of one row of W. Lane group h
// supplies the eight consecutive reduction elements 32 chunk + 8 h .. + 7 of either operand in every mode: two 16-byte LDS reads of U,
// eight rows of W. F32 feeds them to eight v_mfma_f32_16x16x4_f32 (step s takes element s of every group), the 16-bit modes round or
// split them in registers into the fragment of one v_mfma_f32_16x16x32_bf16. W is read straight from global memory: every workgroup
// reads the same 3 wd wd floats per stage (48 KiB at wd = 64, 192 KiB at wd = 128), which live in L2, and one path serves every width.
#include "res2_common.h"

struct Res2Params {
    const float* x;
    const int32_t* lens;
    const float* w;
    const float* bias;
    const float* nscale;
    const float* nshift;
    float* y;
    int64_t T, ldx, ldy;
    int32_t scale, dil, act, R, NR;
    int32_t x_vec, y_vec, w_vec;     // the base pointer is 16-byte aligned: 16-byte accesses (the bits are the same without)
    float* a;                        // ktf_res2_conv_train with the norm pair: act(Z_i) before the norm, (B, T, lda), group i at (i - 1) wd
    int64_t lda;
    int32_t a_vec;
};

template <int MODE, int NCB>
__global__ __launch_bounds__(R2_THREADS) void res2_conv_kernel(Res2Params p) {
    constexpr int W = 16 * NCB, PITCH = W + 4, K = 3 * W, NCH = (K + 31) / 32, W4 = W / 4;
    constexpr bool X3 = MODE == KTF_GEMM_BF16X3;
    extern __shared__ __attribute__((aligned(16))) float r2_lds[];
    const int b = blockIdx.y;
    int len = p.lens ? p.lens[b] : (int)p.T;
    len = len < 0 ? 0 : (len > (int)p.T ? (int)p.T : len);
    const int R = p.R, t0 = (int)blockIdx.x * R;
    if (t0 >= len) return;                                   // (rule 5: an empty utterance has no tile that runs)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, h = lane >> 4;
    const int s = p.scale, d = p.dil, NR = p.NR;
    const int tb = t0 - (s - 1) * d;                         // frame of buffer row 0
    const float* xb = p.x + (int64_t)b * p.T * p.ldx;
    float* yb = p.y + (int64_t)b * p.T * p.ldy;
    const bool xv = p.x_vec, yv = p.y_vec;
    float* cur = r2_lds;
    float* nxt = r2_lds + NR * PITCH;

    // U_1 = X_1 on the whole buffer extent, and Y_0 = X_0 on the tile's rows
    for (int idx = tid; idx < NR * W4; idx += R2_THREADS) {
        const int i = idx / W4, c = (idx - i * W4) * 4, t = tb + i;
        if (t >= 0 && t < len) *reinterpret_cast<r2_fv4*>(cur + i * PITCH + c) = r2_load4(xb + (int64_t)t * p.ldx + W + c, xv);
    }
    for (int idx = tid; idx < R * W4; idx += R2_THREADS) {
        const int i = idx / W4, c = (idx - i * W4) * 4, t = t0 + i;
        if (t < len) r2_store4(yb + (int64_t)t * p.ldy + c, r2_load4(xb + (int64_t)t * p.ldx + c, xv), yv);
    }
    __syncthreads();

    for (int j = 1; j < s; ++j) {
        const int hj = (s - 1 - j) * d;
        const int ulo = t0 - hj > 0 ? t0 - hj : 0;
        const int uhi = t0 + R + hj < len ? t0 + R + hj : len;
        const float* wg = p.w + (int64_t)(j - 1) * K * W + n * NCB;         // the lane's NCB channels of row 0 of W_j
        const int nunits = (uhi - ulo + 31) >> 5;
        for (int u = wave; u < nunits; u += R2_THREADS / 64) {
            const int tu = ulo + 32 * u;
            const bool two = tu + 16 < uhi;                  // (wave-uniform: the unit's second block holds a row)
            int ro[2][3];                                    // LDS offsets of the lane's row at the three taps, per block
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                int t = tu + 16 * rb + n;
                t = t < uhi ? t : uhi - 1;                   // rows past the extent compute a copy of its last row and store nothing
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    int tt = t + (k - 1) * d;
                    tt = tt < 0 ? 0 : (tt > len - 1 ? len - 1 : tt);
                    ro[rb][k] = (tt - tb) * PITCH;
                }
            }
            f32x4 acc[2][NCB];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) acc[rb][cb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

            for (int ch = 0; ch < NCH; ++ch) {
                const int q0 = 32 * ch + 8 * h;              // the lane group's eight reduction elements: one tap, eight input channels
                const bool live = q0 < K;                    // (K % 32 == 16: the last chunk's upper half is zero products)
                const int tap = q0 / W, cin = q0 - tap * W;
                float bw[NCB][8], a[2][8];
                if (live) {
                    const float* wr = wg + (int64_t)q0 * W;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        if (NCB % 4 == 0 && p.w_vec) {
#pragma unroll
                            for (int c4 = 0; c4 < NCB / 4; ++c4) {
                                const r2_fv4 v = *reinterpret_cast<const r2_fv4*>(wr + e * W + 4 * c4);
#pragma unroll
                                for (int i = 0; i < 4; ++i) bw[4 * c4 + i][e] = v[i];
                            }
                        } else {
#pragma unroll
                            for (int cb = 0; cb < NCB; ++cb) bw[cb][e] = wr[e * W + cb];
                        }
                    }
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) {
                        if (rb == 1 && !two) continue;
                        const float* ur = cur + (tap == 0 ? ro[rb][0] : (tap == 1 ? ro[rb][1] : ro[rb][2])) + cin;
                        const r2_fv4 a0 = *reinterpret_cast<const r2_fv4*>(ur), a1 = *reinterpret_cast<const r2_fv4*>(ur + 4);
#pragma unroll
                        for (int i = 0; i < 4; ++i) a[rb][i] = a0[i], a[rb][4 + i] = a1[i];
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
#pragma unroll
                        for (int cb = 0; cb < NCB; ++cb) bw[cb][e] = 0.0f;
                        a[0][e] = a[1][e] = 0.0f;
                    }
                }
                if (!two) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) a[1][e] = 0.0f;
                }
                if constexpr (MODE == KTF_GEMM_F32) {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
#pragma unroll
                        for (int cb = 0; cb < NCB; ++cb) {
                            acc[0][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(bw[cb][e], a[0][e], acc[0][cb], 0, 0, 0);
                            if (two) acc[1][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(bw[cb][e], a[1][e], acc[1][cb], 0, 0, 0);
                        }
                } else {
                    r2_bfrag8 ah[2], al[2];
                    r2_split8<X3>(a[0], ah[0], al[0]);
                    r2_split8<X3>(a[1], ah[1], al[1]);
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) {
                        r2_bfrag8 bh, bl;
                        r2_split8<X3>(bw[cb], bh, bl);
#pragma unroll
                        for (int rb = 0; rb < 2; ++rb) {
                            if (rb == 1 && !two) continue;
                            acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, ah[rb], acc[rb][cb], 0, 0, 0);
                            if (X3) {
                                acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, al[rb], acc[rb][cb], 0, 0, 0);
                                acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl, ah[rb], acc[rb][cb], 0, 0, 0);
                            }
                        }
                    }
                }
            }

            // epilogue: the lane's 4 NCB consecutive channels from c0 of row t; element e of them is acc[rb][e % NCB][e / NCB]
            const int c0 = 4 * h * NCB, pc = (j - 1) * W + c0;
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                const int t = tu + 16 * rb + n;
                if ((rb == 1 && !two) || t >= uhi) continue;
                const bool own = t >= t0 && t < t0 + R;
#pragma unroll
                for (int q = 0; q < NCB; ++q) {
                    r2_fv4 v, av;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = 4 * q + i;
                        float z = acc[rb][e % NCB][e / NCB];
                        if (p.bias) z += p.bias[pc + e];
                        if (p.act == KTF_ACT_RELU) z = z < 0.0f ? 0.0f : z;
                        av[i] = z;
                        if (p.nscale) z = __fadd_rn(__fmul_rn(z, p.nscale[pc + e]), p.nshift[pc + e]);
                        v[i] = z;
                    }
                    const int c = c0 + 4 * q;
                    if (own) r2_store4(yb + (int64_t)t * p.ldy + j * W + c, v, yv);
                    if (own && p.a) r2_store4(p.a + ((int64_t)b * p.T + t) * p.lda + pc + 4 * q, av, p.a_vec);
                    if (j + 1 < s) {
                        const r2_fv4 xn = r2_load4(xb + (int64_t)t * p.ldx + (j + 1) * W + c, xv);
                        *reinterpret_cast<r2_fv4*>(nxt + (t - tb) * PITCH + c) = xn + v;
                    }
                }
            }
        }
        __syncthreads();
        float* sw = cur;
        cur = nxt;
        nxt = sw;
    }
}

// ------------------------------------------------------------------------------------ host
static int r2_lds_bytes(int R, int width, int scale, int dilation) { return 2 * (R + 2 * (scale - 1) * dilation) * (width + 4) * 4; }

extern "C" int32_t ktf_res2_row_tile(int32_t width, int32_t scale, int32_t dilation, int32_t gemm) {
    if (int rc = r2_check_shape("ktf_res2_row_tile", width, scale, dilation, gemm)) return rc;
    int R = R2_MAX_TILE;
    while (R > 16 && r2_lds_bytes(R, width, scale, dilation) > R2_LDS_BYTES) R -= 16;
    return R;                                                // (16 rows fit at every shape: 2 * 128 * 132 * 4 = 135 168 bytes)
}

template <auto KERNEL>
static void r2_launch_kernel(const Res2Params& p, dim3 grid, int lds, hipStream_t st) {
    KTF_LDS_ONCE(R2_LDS_BYTES, KERNEL);
    hipLaunchKernelGGL(KERNEL, grid, dim3(R2_THREADS), lds, st, p);
}

template <int MODE>
static void r2_launch_mode(const Res2Params& p, int ncb, dim3 grid, int lds, hipStream_t st) {
    switch (ncb) {
        case 1: return r2_launch_kernel<res2_conv_kernel<MODE, 1>>(p, grid, lds, st);
        case 2: return r2_launch_kernel<res2_conv_kernel<MODE, 2>>(p, grid, lds, st);
        case 3: return r2_launch_kernel<res2_conv_kernel<MODE, 3>>(p, grid, lds, st);
        case 4: return r2_launch_kernel<res2_conv_kernel<MODE, 4>>(p, grid, lds, st);
        case 5: return r2_launch_kernel<res2_conv_kernel<MODE, 5>>(p, grid, lds, st);
        case 6: return r2_launch_kernel<res2_conv_kernel<MODE, 6>>(p, grid, lds, st);
        case 7: return r2_launch_kernel<res2_conv_kernel<MODE, 7>>(p, grid, lds, st);
        default: return r2_launch_kernel<res2_conv_kernel<MODE, 8>>(p, grid, lds, st);
    }
}

// the forward of both entry points: `train` asks for a exactly when the norm pair is there (include/ktf_res2.h rule 7)
static int r2_forward(const char* who, bool train, const float* x, int64_t B, int64_t T, int32_t C, int64_t ldx, const int32_t* lens, int32_t scale,
                      int32_t dilation, const float* w, const float* bias, const float* nscale, const float* nshift, int32_t act, int32_t gemm,
                      float* y, int64_t ldy, float* a, int64_t lda, void* stream) {
    int32_t wd = 0;
    if (int rc = r2_check_sizes(who, B, T, C, scale, dilation, gemm, &wd)) return rc;
    KTF_REQUIRE(ldx >= C && ldy >= C, "%s: ldx %lld or ldy %lld below C %d", who, (long long)ldx, (long long)ldy, (int)C);
    KTF_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0, "%s: ldx %lld and ldy %lld must be multiples of 4", who, (long long)ldx, (long long)ldy);
    KTF_REQUIRE(ldx < (1ll << 31) && ldy < (1ll << 31), "%s: a leading dimension reaches 2^31", who);
    KTF_REQUIRE((nscale == nullptr) == (nshift == nullptr), "%s: nscale and nshift go together", who);
    KTF_REQUIRE(act == KTF_ACT_NONE || act == KTF_ACT_RELU, "%s: act %d is not KTF_ACT_NONE or KTF_ACT_RELU", who, (int)act);
    const int64_t rows = B * T;                              // < 2^46
    KTF_REQUIRE(rows == 0 || (x && y && w), "%s: null x, y or w", who);
    int64_t nx = 0, ny = 0;
    KTF_REQUIRE(!__builtin_mul_overflow(rows, ldx, &nx) && !__builtin_mul_overflow(rows, ldy, &ny) && nx < (1ll << 60) && ny < (1ll << 60),
                "%s: B * T * ldx or B * T * ldy reaches 2^60", who);
    if (rows > 0) {
        const uintptr_t x0 = (uintptr_t)x, y0 = (uintptr_t)y;
        const uintptr_t xn = (uintptr_t)(nx - ldx + C) * 4, yn = (uintptr_t)ny * 4;
        KTF_REQUIRE(!(x0 < y0 + yn && y0 < x0 + xn), "%s: y overlaps x", who);
    }
    if (train) {
        KTF_REQUIRE((a != nullptr) == (nscale != nullptr) || rows == 0, "%s: a goes with nscale / nshift: it is missing or misplaced", who);
        if (nscale) {
            const int64_t Ca = (int64_t)(scale - 1) * wd;
            int64_t na = 0;
            KTF_REQUIRE(lda >= Ca && lda % 4 == 0 && lda < (1ll << 31), "%s: lda %lld below %lld, not a multiple of 4 or at 2^31", who, (long long)lda,
                        (long long)Ca);
            KTF_REQUIRE(!__builtin_mul_overflow(rows, lda, &na) && na < (1ll << 60), "%s: B * T * lda reaches 2^60", who);
            if (rows > 0) {
                const uintptr_t a0 = (uintptr_t)a, an = (uintptr_t)na * 4, x0 = (uintptr_t)x, y0 = (uintptr_t)y;
                KTF_REQUIRE(!(a0 < x0 + (uintptr_t)nx * 4 && x0 < a0 + an) && !(a0 < y0 + (uintptr_t)ny * 4 && y0 < a0 + an), "%s: a overlaps x or y", who);
            }
        }
    }
    if (rows == 0) return KTF_OK;

    const int R = ktf_res2_row_tile(wd, scale, dilation, gemm);
    Res2Params p = {x, lens, w, bias, nscale, nshift, y, T, ldx, ldy, scale, dilation, act, R, R + 2 * (scale - 1) * dilation,
                    ((uintptr_t)x & 15) == 0, ((uintptr_t)y & 15) == 0, ((uintptr_t)w & 15) == 0, train ? a : nullptr, lda, ((uintptr_t)a & 15) == 0};
    const dim3 grid((unsigned)ktf_cdiv(T, R), (unsigned)B);
    const int lds = r2_lds_bytes(R, wd, scale, dilation);
    hipStream_t st = (hipStream_t)stream;
    if (gemm == KTF_GEMM_F32) r2_launch_mode<KTF_GEMM_F32>(p, wd / 16, grid, lds, st);
    else if (gemm == KTF_GEMM_BF16) r2_launch_mode<KTF_GEMM_BF16>(p, wd / 16, grid, lds, st);
    else r2_launch_mode<KTF_GEMM_BF16X3>(p, wd / 16, grid, lds, st);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_res2_conv(const float* x, int64_t B, int64_t T, int32_t C, int64_t ldx, const int32_t* lens, int32_t scale, int32_t dilation,
                             const float* w, const float* bias, const float* nscale, const float* nshift, int32_t act, int32_t gemm, float* y,
                             int64_t ldy, void* stream) {
    return r2_forward("ktf_res2_conv", false, x, B, T, C, ldx, lens, scale, dilation, w, bias, nscale, nshift, act, gemm, y, ldy, nullptr, 0, stream);
}

extern "C" int ktf_res2_conv_train(const float* x, int64_t B, int64_t T, int32_t C, int64_t ldx, const int32_t* lens, int32_t scale, int32_t dilation,
                                   const float* w, const float* bias, const float* nscale, const float* nshift, int32_t act, int32_t gemm, float* y,
                                   int64_t ldy, float* a, int64_t lda, void* stream) {
    return r2_forward("ktf_res2_conv_train", true, x, B, T, C, ldx, lens, scale, dilation, w, bias, nscale, nshift, act, gemm, y, ldy, a, lda, stream);
}
