// The backward of the Res2Net dilated convolution (include/ktf_res2.h rules 7 - 13): the data gradient in one
// launch, the parameter gradients in one launch over row slots plus a small launch that adds the slots in ascending order.
//
// Data gradient: the forward walked backwards. A workgroup of eight waves owns R rows [t0, t0 + R) of dx of one utterance and walks the
// stages j = s - 1 .. 1. Stage j holds dZ_j on [t0 - j d, t0 + R + j d) cut to [0, len) in one LDS row buffer and computes dU_j on
// [t0 - (j - 1) d, t0 + R + (j - 1) d): its epilogue stores dX_j = dU_j for the tile's own rows and writes
// dZ_{j-1} = (dU_j + G_{j-1}) nscale [A > 0] into the other buffer (G, the saved activation and nscale come from global memory, for
// the halo rows too; Gt_{j-1} = dU_j + G_{j-1} of the tile's own rows goes to the gt buffer for the weights kernel). The whole halo
// is (s - 1) d, as in the forward, and nothing is communicated between tiles. Three more LDS rows serve the transposed edge rule: the
// folded rows S_0[0] and S_2[len - 1] (fp32 sums in ascending t, built by every tile whose dU extent holds row 0 / row len - 1) and a
// row of zeros for the taps that fall outside the utterance. The product is the forward's: the reduction index is q = k wd + c_out,
// a lane group's eight elements are eight consecutive floats of one row of W[k] (two 16-byte loads), lane (n, h) owns 4 NCB
// consecutive input channels of row n.
//
// Parameter gradients: grid (slot, group, tap), four waves. The rows of the batch are cut into chunks of 32 frames of one utterance
// and a slot owns a contiguous run of chunks. Per chunk the workgroup stages dZ (formed from gt, the saved activation and nscale as
// above) and U at the tap's clamped rows (x + y, one fp32 add) TRANSPOSED into LDS, so that a lane's eight reduction elements (eight
// consecutive frames of one channel) are two 16-byte reads, and every wave accumulates its 16 x 16 blocks of the wd x wd product
// U^T dZ. The workgroup of tap 1 also sums dbias, dnscale and dnshift per column, rows ascending. Every slot writes a region of its own.
#include <type_traits>

#include "res2_common.h"

#define R2G_WTHREADS 256
#define R2G_TP 36                // floats per channel of a transposed chunk: 32 frames + 4 (16-byte aligned, h groups on disjoint banks)
#define R2G_CHUNK 32

struct Res2GradParams {
    const float* g;
    const int32_t* lens;
    const float* w;
    const float* nscale;
    const float* am;                 // the saved activation the mask is taken from: a (with the norm pair) or y
    float* dx;
    float* gt;
    int64_t T, ldg, ldam, lddx, ldgt;
    int32_t scale, dil, relu, R, NR, amoff;      // amoff: column of group 1 in am (0 in a, wd in y)
    int32_t g_vec, am_vec, dx_vec, gt_vec, w_vec;
};

// dZ = Gt nscale [A > 0] of four channels: one fp32 multiply, then the mask (rule 9)
__device__ __forceinline__ r2_fv4 r2g_dz4(r2_fv4 gt, const float* nscale, const float* am, bool relu, bool amv) {
    r2_fv4 v = gt;
    if (nscale) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = __fmul_rn(v[i], nscale[i]);
    }
    if (relu) {
        const r2_fv4 a = r2_load4(am, amv);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = a[i] > 0.0f ? v[i] : 0.0f;
    }
    return v;
}

template <int MODE, int NCB>
__global__ __launch_bounds__(R2_THREADS) void res2_grad_data_kernel(Res2GradParams p) {
    constexpr int W = 16 * NCB, PITCH = W + 4, K = 3 * W, NCH = (K + 31) / 32, W4 = W / 4;
    constexpr bool X3 = MODE == KTF_GEMM_BF16X3;
    extern __shared__ __attribute__((aligned(16))) float r2g_lds[];
    const int b = blockIdx.y;
    int len = p.lens ? p.lens[b] : (int)p.T;
    len = len < 0 ? 0 : (len > (int)p.T ? (int)p.T : len);
    const int R = p.R, t0 = (int)blockIdx.x * R;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, h = lane >> 4;
    const int s = p.scale, d = p.dil, NR = p.NR;
    const int tb = t0 - (s - 1) * d;                         // frame of buffer row 0
    const float* gb = p.g + (int64_t)b * p.T * p.ldg;
    const float* amb = p.am + (int64_t)b * p.T * p.ldam + p.amoff;
    float* dxb = p.dx + (int64_t)b * p.T * p.lddx;
    float* gtb = p.gt + (int64_t)b * p.T * p.ldgt;
    const bool gv = p.g_vec, av = p.am_vec, dv = p.dx_vec, tv = p.gt_vec, relu = p.relu;

    // rows of the tile at and beyond the length: dx is zero in [0, C)
    const int tend = t0 + R < (int)p.T ? t0 + R : (int)p.T;
    for (int idx = tid; idx < R * s * W4; idx += R2_THREADS) {
        const int i = idx / (s * W4), c = (idx - i * s * W4) * 4, t = t0 + i;
        if (t >= len && t < tend) r2_store4(dxb + (int64_t)t * p.lddx + c, r2_fv4{0.0f, 0.0f, 0.0f, 0.0f}, dv);
    }
    if (t0 >= len) return;

    float* cur = r2g_lds;
    float* nxt = r2g_lds + NR * PITCH;
    float* fold0 = r2g_lds + 2 * NR * PITCH;                 // S_0[0], then S_2[len - 1], then the row of zeros
    const int FOLD0 = 2 * NR * PITCH, FOLDL = FOLD0 + PITCH, ZERO = FOLDL + PITCH;
    for (int c = tid; c < PITCH; c += R2_THREADS) fold0[2 * PITCH + c] = 0.0f;

    // dX_0 = G_0 on the tile's rows; Gt_{s-1} = G_{s-1} and dZ_{s-1} on the whole buffer extent
    for (int idx = tid; idx < R * W4; idx += R2_THREADS) {
        const int i = idx / W4, c = (idx - i * W4) * 4, t = t0 + i;
        if (t < len) r2_store4(dxb + (int64_t)t * p.lddx + c, r2_load4(gb + (int64_t)t * p.ldg + c, gv), dv);
    }
    for (int idx = tid; idx < NR * W4; idx += R2_THREADS) {
        const int i = idx / W4, c = (idx - i * W4) * 4, t = tb + i;
        if (t < 0 || t >= len) continue;
        const int pc = (s - 2) * W + c;
        const r2_fv4 G = r2_load4(gb + (int64_t)t * p.ldg + (s - 1) * W + c, gv);
        if (t >= t0 && t < t0 + R) r2_store4(gtb + (int64_t)t * p.ldgt + pc, G, tv);
        *reinterpret_cast<r2_fv4*>(cur + i * PITCH + c) = r2g_dz4(G, p.nscale ? p.nscale + pc : nullptr, amb + (int64_t)t * p.ldam + pc, relu, av);
    }
    __syncthreads();

    for (int j = s - 1; j >= 1; --j) {
        const int hj = (j - 1) * d;
        const int ulo = t0 - hj > 0 ? t0 - hj : 0;
        const int uhi = t0 + R + hj < len ? t0 + R + hj : len;
        // the folded edge rows of dZ_j (rule 10): the rows they sum lie inside this stage's dZ extent whenever ulo = 0 / uhi = len
        if (ulo == 0 && tid < W) {
            const int last = d < len - 1 ? d : len - 1;
            float sum = 0.0f;
            for (int t = 0; t <= last; ++t) sum += cur[(t - tb) * PITCH + tid];
            fold0[tid] = sum;
        }
        if (uhi == len && tid >= 128 && tid < 128 + W) {
            const int first = len - 1 - d > 0 ? len - 1 - d : 0;
            float sum = 0.0f;
            for (int t = first; t <= len - 1; ++t) sum += cur[(t - tb) * PITCH + tid - 128];
            fold0[PITCH + tid - 128] = sum;
        }
        __syncthreads();

        const float* wg = p.w + (int64_t)(j - 1) * K * W + (int64_t)n * NCB * W;      // row c_in = n NCB of W_j[0]
        const int nunits = (uhi - ulo + 31) >> 5;
        const int cur0 = (int)(cur - r2g_lds);               // this stage's dZ buffer within the LDS
        for (int u = wave; u < nunits; u += R2_THREADS / 64) {
            const int tu = ulo + 32 * u;
            const bool two = tu + 16 < uhi;
            int ro[2][3];                                    // LDS offsets (from r2g_lds) of S_k of the lane's row, per block
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                int t = tu + 16 * rb + n;
                t = t < uhi ? t : uhi - 1;                   // rows past the extent compute a copy of its last row and store nothing
                ro[rb][1] = cur0 + (t - tb) * PITCH;
                ro[rb][0] = t == 0 ? FOLD0 : (t + d < len ? cur0 + (t + d - tb) * PITCH : ZERO);
                ro[rb][2] = t == len - 1 ? FOLDL : (t - d >= 0 ? cur0 + (t - d - tb) * PITCH : ZERO);
            }
            f32x4 acc[2][NCB];
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) acc[rb][cb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

            for (int ch = 0; ch < NCH; ++ch) {
                const int q0 = 32 * ch + 8 * h;              // the lane group's eight reduction elements: one tap, eight output channels
                const bool live = q0 < K;
                const int tap = q0 / W, co = q0 - tap * W;
                float bw[NCB][8], a[2][8];
                if (live) {
                    const float* wr = wg + (int64_t)tap * W * W + co;
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) {
                        const r2_fv4 w0 = r2_load4(wr + cb * W, p.w_vec), w1 = r2_load4(wr + cb * W + 4, p.w_vec);
#pragma unroll
                        for (int i = 0; i < 4; ++i) bw[cb][i] = w0[i], bw[cb][4 + i] = w1[i];
                    }
#pragma unroll
                    for (int rb = 0; rb < 2; ++rb) {
                        if (rb == 1 && !two) continue;
                        const float* zr = r2g_lds + (tap == 0 ? ro[rb][0] : (tap == 1 ? ro[rb][1] : ro[rb][2])) + co;
                        const r2_fv4 a0 = *reinterpret_cast<const r2_fv4*>(zr), a1 = *reinterpret_cast<const r2_fv4*>(zr + 4);
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

            // epilogue: the lane's 4 NCB consecutive input channels from c0 of row t; element e of them is acc[rb][e % NCB][e / NCB]
            const int c0 = 4 * h * NCB;
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                const int t = tu + 16 * rb + n;
                if ((rb == 1 && !two) || t >= uhi) continue;
                const bool own = t >= t0 && t < t0 + R;
#pragma unroll
                for (int q = 0; q < NCB; ++q) {
                    r2_fv4 v;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = 4 * q + i;
                        v[i] = acc[rb][e % NCB][e / NCB];
                    }
                    const int c = c0 + 4 * q;
                    if (own) r2_store4(dxb + (int64_t)t * p.lddx + j * W + c, v, dv);
                    if (j > 1) {
                        const int pc = (j - 2) * W + c;
                        const r2_fv4 Gt = r2_load4(gb + (int64_t)t * p.ldg + (j - 1) * W + c, gv) + v;
                        if (own) r2_store4(gtb + (int64_t)t * p.ldgt + pc, Gt, tv);
                        *reinterpret_cast<r2_fv4*>(nxt + (t - tb) * PITCH + c) =
                            r2g_dz4(Gt, p.nscale ? p.nscale + pc : nullptr, amb + (int64_t)t * p.ldam + pc, relu, av);
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

// ------------------------------------------------------------------------------------ parameter gradients
struct Res2GradWParams {
    const float* x;
    const float* y;
    const float* am;
    const float* gt;
    const float* nscale;
    const int32_t* lens;
    float* scratch;
    int64_t T, ldx, ldy, ldam, ldgt, per;        // per: floats of a slot's region
    int32_t scale, dil, relu, amoff, nct, cps, total;      // chunks per utterance, per slot, in all
    int32_t x_vec, y_vec, am_vec, gt_vec;
};

template <int MODE, int NCB>
__global__ __launch_bounds__(R2G_WTHREADS) void res2_grad_w_kernel(Res2GradWParams p) {
    constexpr int W = 16 * NCB, W4 = W / 4, MB = (NCB + 3) / 4, TP = R2G_TP;
    constexpr bool X3 = MODE == KTF_GEMM_BF16X3;
    extern __shared__ __attribute__((aligned(16))) float r2w_lds[];
    float* Ut = r2w_lds;                                     // [channel][frame of the chunk]
    float* Zt = Ut + W * TP;
    float* Gs = Zt + W * TP;                                 // Gt and A of the chunk: the tap-1 workgroup with the norm pair only
    float* As = Gs + W * TP;
    const int slot = blockIdx.x, i = blockIdx.y + 1, k = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, h = lane >> 4;
    const int d = p.dil, s = p.scale;
    const bool sums = k == 1, norm = p.nscale != nullptr, relu = p.relu;
    const int pc0 = (i - 1) * W;

    f32x4 acc[MB][NCB];
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
        for (int nb = 0; nb < NCB; ++nb) acc[mi][nb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float sb = 0.0f, sc = 0.0f, sh = 0.0f;                   // dbias, dnscale, dnshift of column tid

    const int c_lo = slot * p.cps, c_hi = c_lo + p.cps < p.total ? c_lo + p.cps : p.total;
    for (int cid = c_lo; cid < c_hi; ++cid) {
        const int b = cid / p.nct, r0 = (cid - b * p.nct) * R2G_CHUNK;
        int len = p.lens ? p.lens[b] : (int)p.T;
        len = len < 0 ? 0 : (len > (int)p.T ? (int)p.T : len);
        if (r0 >= len) continue;                             // (uniform: an empty utterance or a chunk beyond the length adds nothing)
        const int64_t row0 = (int64_t)b * p.T;
        for (int idx = tid; idx < R2G_CHUNK * W4; idx += R2G_WTHREADS) {
            const int r = idx / W4, c = (idx - r * W4) * 4, t = r0 + r;
            r2_fv4 z = {0.0f, 0.0f, 0.0f, 0.0f}, u = z, G = z, A = z;
            if (t < len) {
                G = r2_load4(p.gt + (row0 + t) * p.ldgt + pc0 + c, p.gt_vec);
                const float* am = p.am + (row0 + t) * p.ldam + p.amoff + pc0 + c;
                z = r2g_dz4(G, norm ? p.nscale + pc0 + c : nullptr, am, relu, p.am_vec);
                if (sums && norm) A = r2_load4(am, p.am_vec);
                int tt = t + (k - 1) * d;
                tt = tt < 0 ? 0 : (tt > len - 1 ? len - 1 : tt);
                u = r2_load4(p.x + (row0 + tt) * p.ldx + i * W + c, p.x_vec);
                if (i >= 2) u = u + r2_load4(p.y + (row0 + tt) * p.ldy + pc0 + c, p.y_vec);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                Ut[(c + e) * TP + r] = u[e];
                Zt[(c + e) * TP + r] = z[e];
                if (sums && norm) Gs[(c + e) * TP + r] = G[e], As[(c + e) * TP + r] = A[e];
            }
        }
        __syncthreads();
#pragma unroll
        for (int mi = 0; mi < MB; ++mi) {
            const int mb = wave + 4 * mi;
            if (mb >= NCB) continue;
            float a[8];
            {
                const float* ur = Ut + (mb * 16 + n) * TP + 8 * h;
                const r2_fv4 a0 = *reinterpret_cast<const r2_fv4*>(ur), a1 = *reinterpret_cast<const r2_fv4*>(ur + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = a0[e], a[4 + e] = a1[e];
            }
            r2_bfrag8 ah, al;
            if constexpr (MODE != KTF_GEMM_F32) r2_split8<X3>(a, ah, al);
#pragma unroll
            for (int nb = 0; nb < NCB; ++nb) {
                float bz[8];
                const float* zr = Zt + (nb * 16 + n) * TP + 8 * h;
                const r2_fv4 b0 = *reinterpret_cast<const r2_fv4*>(zr), b1 = *reinterpret_cast<const r2_fv4*>(zr + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) bz[e] = b0[e], bz[4 + e] = b1[e];
                if constexpr (MODE == KTF_GEMM_F32) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[mi][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], bz[e], acc[mi][nb], 0, 0, 0);
                } else {
                    r2_bfrag8 bh, bl;
                    r2_split8<X3>(bz, bh, bl);
                    acc[mi][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc[mi][nb], 0, 0, 0);
                    if (X3) {
                        acc[mi][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc[mi][nb], 0, 0, 0);
                        acc[mi][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc[mi][nb], 0, 0, 0);
                    }
                }
            }
        }
        if (sums && tid < W) {
            for (int r = 0; r < R2G_CHUNK; ++r) {
                sb += Zt[tid * TP + r];
                if (norm) {
                    const float gv = Gs[tid * TP + r];
                    sh += gv;
                    sc += __fmul_rn(gv, As[tid * TP + r]);
                }
            }
        }
        __syncthreads();
    }

    // the slot's region: dW as [g][k][c_in][c_out], then [g][dbias, dnscale, dnshift][wd]
    float* reg = p.scratch + (int64_t)slot * p.per;
    float* dwr = reg + ((int64_t)(i - 1) * 3 + k) * W * W;
#pragma unroll
    for (int mi = 0; mi < MB; ++mi) {
        const int mb = wave + 4 * mi;
        if (mb >= NCB) continue;
#pragma unroll
        for (int nb = 0; nb < NCB; ++nb)
#pragma unroll
            for (int e = 0; e < 4; ++e) dwr[(mb * 16 + 4 * h + e) * W + nb * 16 + n] = acc[mi][nb][e];
    }
    if (sums && tid < W) {
        float* sr = reg + (int64_t)(s - 1) * 3 * W * W + (int64_t)(i - 1) * 3 * W;
        sr[tid] = sb;
        sr[W + tid] = sc;
        sr[2 * W + tid] = sh;
    }
}

// the slots in ascending order; nslots = 0 writes zeros
__global__ __launch_bounds__(256) void res2_grad_reduce_kernel(const float* scratch, int nslots, int64_t per, int64_t nw, int W, float* dw,
                                                               float* dbias, float* dnscale, float* dnshift) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    float sum = 0.0f;
    for (int sl = 0; sl < nslots; ++sl) sum += scratch[(int64_t)sl * per + e];
    if (e < nw) {
        if (dw) dw[e] = sum;
        return;
    }
    const int q = (int)(e - nw), g = q / (3 * W), kind = (q / W) % 3, c = q % W;
    float* dst = kind == 0 ? dbias : (kind == 1 ? dnscale : dnshift);
    if (dst) dst[g * W + c] = sum;
}

// ------------------------------------------------------------------------------------ host
static int r2g_lds_bytes(int R, int width, int scale, int dilation) { return (2 * (R + 2 * (scale - 1) * dilation) + 3) * (width + 4) * 4; }

extern "C" int32_t ktf_res2_grad_row_tile(int32_t width, int32_t scale, int32_t dilation, int32_t gemm) {
    if (int rc = r2_check_shape("ktf_res2_grad_row_tile", width, scale, dilation, gemm)) return rc;
    int R = R2_MAX_TILE;
    while (R > 16 && r2g_lds_bytes(R, width, scale, dilation) > R2_LDS_BYTES) R -= 16;
    return R;                                                // (16 rows fit at every shape: (2 * 128 + 3) * 132 * 4 = 136 752 bytes)
}

static int r2g_check_sizes(const char* who, int64_t B, int64_t T, int32_t width, int32_t scale) {
    KTF_REQUIRE(B >= 0 && T >= 0, "%s: negative size (B %lld, T %lld)", who, (long long)B, (long long)T);
    KTF_REQUIRE(B <= KTF_RES2_MAX_BATCH && T <= KTF_RES2_MAX_ROWS, "%s: B %lld above %d or T %lld above %d", who, (long long)B, KTF_RES2_MAX_BATCH,
                (long long)T, KTF_RES2_MAX_ROWS);
    return r2_check_shape(who, width, scale, 1, KTF_GEMM_F32);
}

// slot rule (rule 12): chunks of 32 frames per utterance; min(chunks, clamp(ceil(768 / (3 (scale - 1))), 32, 64)) slots
static int64_t r2g_chunks(int64_t B, int64_t T) { return B * ((T + R2G_CHUNK - 1) / R2G_CHUNK); }
static int r2g_slots(int64_t B, int64_t T, int scale) {
    int want = (768 + 3 * (scale - 1) - 1) / (3 * (scale - 1));
    want = want < 32 ? 32 : (want > 64 ? 64 : want);
    const int64_t chunks = r2g_chunks(B, T);
    return (int)(chunks < want ? chunks : want);
}
static int64_t r2g_per(int width, int scale) { return (int64_t)(scale - 1) * 3 * width * (width + 1); }

extern "C" int32_t ktf_res2_grad_slots(int64_t B, int64_t T, int32_t width, int32_t scale) {
    if (int rc = r2g_check_sizes("ktf_res2_grad_slots", B, T, width, scale)) return rc;
    return r2g_slots(B, T, scale);
}

extern "C" int32_t ktf_res2_grad_scratch_floats(int64_t B, int64_t T, int32_t width, int32_t scale) {
    const char* who = "ktf_res2_grad_scratch_floats";
    if (int rc = r2g_check_sizes(who, B, T, width, scale)) return rc;
    const int64_t n = (int64_t)r2g_slots(B, T, scale) * r2g_per(width, scale);
    KTF_REQUIRE(n < (1ll << 31), "%s: %lld floats do not fit the answer", who, (long long)n);
    return (int32_t)n;
}

struct R2gSpan {
    const char* name;
    const void* p;
    int64_t floats;
};
// no output span may meet an input span (rule 13)
static int r2g_no_overlap(const char* who, const R2gSpan* outs, int no, const R2gSpan* ins, int ni) {
    for (int o = 0; o < no; ++o)
        for (int i = 0; i < ni; ++i) {
            if (!outs[o].p || !ins[i].p || outs[o].floats <= 0 || ins[i].floats <= 0) continue;
            const uintptr_t a = (uintptr_t)outs[o].p, an = (uintptr_t)outs[o].floats * 4, c = (uintptr_t)ins[i].p, cn = (uintptr_t)ins[i].floats * 4;
            KTF_REQUIRE(!(a < c + cn && c < a + an), "%s: %s overlaps %s", who, outs[o].name, ins[i].name);
        }
    return KTF_OK;
}

// the checks both gradient calls share; wd comes back
static int r2g_check_common(const char* who, int64_t B, int64_t T, int32_t C, int32_t scale, int32_t dilation, int32_t act, int32_t gemm,
                            const float* nscale, const float* a, int32_t* wd) {
    if (int rc = r2_check_sizes(who, B, T, C, scale, dilation, gemm, wd)) return rc;
    KTF_REQUIRE(act == KTF_ACT_NONE || act == KTF_ACT_RELU, "%s: act %d is not KTF_ACT_NONE or KTF_ACT_RELU", who, (int)act);
    KTF_REQUIRE((a != nullptr) == (nscale != nullptr) || B * T == 0, "%s: a goes with nscale: it is missing or misplaced", who);
    return KTF_OK;
}

static int r2g_check_ld(const char* who, const char* name, int64_t ld, int64_t width, int64_t rows) {
    KTF_REQUIRE(ld >= width, "%s: %s %lld below its width %lld", who, name, (long long)ld, (long long)width);
    KTF_REQUIRE(ld % 4 == 0, "%s: %s %lld must be a multiple of 4", who, name, (long long)ld);
    KTF_REQUIRE(ld < (1ll << 31), "%s: %s reaches 2^31", who, name);
    int64_t nn = 0;
    KTF_REQUIRE(!__builtin_mul_overflow(rows, ld, &nn) && nn < (1ll << 60), "%s: B * T * %s reaches 2^60", who, name);
    return KTF_OK;
}

template <auto KERNEL, typename P>
static void r2g_launch_kernel(const P& p, dim3 grid, int threads, int lds, hipStream_t st) {
    KTF_LDS_ONCE(R2_LDS_BYTES, KERNEL);
    hipLaunchKernelGGL(KERNEL, grid, dim3(threads), lds, st, p);
}

// one kernel instance of either launch: the parameter struct tells which
template <int MODE, int NCB, typename P>
static void r2g_launch_one(const P& p, dim3 grid, int lds, hipStream_t st) {
    if constexpr (std::is_same_v<P, Res2GradParams>) r2g_launch_kernel<res2_grad_data_kernel<MODE, NCB>>(p, grid, R2_THREADS, lds, st);
    else r2g_launch_kernel<res2_grad_w_kernel<MODE, NCB>>(p, grid, R2G_WTHREADS, lds, st);
}

template <typename P>
static void r2g_launch(const P& p, int gemm, int ncb, dim3 grid, int lds, hipStream_t st) {
#define R2G_CASE(N)                                                                                    \
    case N:                                                                                            \
        if (gemm == KTF_GEMM_F32) return r2g_launch_one<KTF_GEMM_F32, N>(p, grid, lds, st);            \
        if (gemm == KTF_GEMM_BF16) return r2g_launch_one<KTF_GEMM_BF16, N>(p, grid, lds, st);          \
        return r2g_launch_one<KTF_GEMM_BF16X3, N>(p, grid, lds, st);
    switch (ncb) {
        R2G_CASE(1) R2G_CASE(2) R2G_CASE(3) R2G_CASE(4) R2G_CASE(5) R2G_CASE(6) R2G_CASE(7) R2G_CASE(8)
    }
#undef R2G_CASE
}

extern "C" int ktf_res2_grad_data(const float* g, int64_t B, int64_t T, int32_t C, int64_t ldg, const int32_t* lens, int32_t scale, int32_t dilation,
                                  const float* w, const float* nscale, const float* y, int64_t ldy, const float* a, int64_t lda, int32_t act,
                                  int32_t gemm, float* dx, int64_t lddx, float* gt, int64_t ldgt, void* stream) {
    const char* who = "ktf_res2_grad_data";
    int32_t wd = 0;
    if (int rc = r2g_check_common(who, B, T, C, scale, dilation, act, gemm, nscale, a, &wd)) return rc;
    const int64_t rows = B * T, Ca = (int64_t)(scale - 1) * wd;
    if (int rc = r2g_check_ld(who, "ldg", ldg, C, rows)) return rc;
    if (int rc = r2g_check_ld(who, "ldy", ldy, C, rows)) return rc;
    if (int rc = r2g_check_ld(who, "lddx", lddx, C, rows)) return rc;
    if (int rc = r2g_check_ld(who, "ldgt", ldgt, Ca, rows)) return rc;
    if (nscale)
        if (int rc = r2g_check_ld(who, "lda", lda, Ca, rows)) return rc;
    KTF_REQUIRE(rows == 0 || (g && w && y && dx && gt), "%s: null g, w, y, dx or gt", who);
    const R2gSpan outs[] = {{"dx", dx, rows * lddx}, {"gt", gt, rows * ldgt}};
    const R2gSpan ins[] = {{"g", g, rows * ldg}, {"y", y, rows * ldy}, {"a", a, rows * lda}, {"w", w, Ca * 3 * wd}, {"nscale", nscale, Ca},
                           {"gt", gt, rows * ldgt}};
    if (int rc = r2g_no_overlap(who, outs, 2, ins, 5)) return rc;
    if (int rc = r2g_no_overlap(who, outs, 1, ins + 5, 1)) return rc;
    if (rows == 0) return KTF_OK;

    const int R = ktf_res2_grad_row_tile(wd, scale, dilation, gemm);
    const float* am = nscale ? a : y;
    Res2GradParams p = {g, lens, w, nscale, am, dx, gt, T, ldg, nscale ? lda : ldy, lddx, ldgt, scale, dilation, act == KTF_ACT_RELU, R,
                        R + 2 * (scale - 1) * dilation, nscale ? 0 : wd,
                        ((uintptr_t)g & 15) == 0, ((uintptr_t)am & 15) == 0, ((uintptr_t)dx & 15) == 0, ((uintptr_t)gt & 15) == 0, ((uintptr_t)w & 15) == 0};
    const dim3 grid((unsigned)ktf_cdiv(T, R), (unsigned)B);
    const int lds = r2g_lds_bytes(R, wd, scale, dilation);
    hipStream_t st = (hipStream_t)stream;
    r2g_launch(p, gemm, wd / 16, grid, lds, st);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_res2_grad_weights(const float* x, int64_t B, int64_t T, int32_t C, int64_t ldx, const int32_t* lens, int32_t scale,
                                     int32_t dilation, const float* nscale, const float* y, int64_t ldy, const float* a, int64_t lda,
                                     const float* gt, int64_t ldgt, int32_t act, int32_t gemm, float* dw, float* dbias, float* dnscale,
                                     float* dnshift, float* scratch, int64_t scratch_floats, void* stream) {
    const char* who = "ktf_res2_grad_weights";
    int32_t wd = 0;
    if (int rc = r2g_check_common(who, B, T, C, scale, dilation, act, gemm, nscale, a, &wd)) return rc;
    const int64_t rows = B * T, Ca = (int64_t)(scale - 1) * wd;
    if (int rc = r2g_check_ld(who, "ldx", ldx, C, rows)) return rc;
    if (int rc = r2g_check_ld(who, "ldy", ldy, C, rows)) return rc;
    if (int rc = r2g_check_ld(who, "ldgt", ldgt, Ca, rows)) return rc;
    if (nscale)
        if (int rc = r2g_check_ld(who, "lda", lda, Ca, rows)) return rc;
    KTF_REQUIRE(nscale || (!dnscale && !dnshift), "%s: dnscale / dnshift without nscale", who);
    KTF_REQUIRE(rows == 0 || (x && y && gt), "%s: null x, y or gt", who);
    const int nslots = rows == 0 ? 0 : r2g_slots(B, T, scale);
    const int64_t per = r2g_per(wd, scale), need = (int64_t)nslots * per;
    KTF_REQUIRE(scratch_floats >= need && (need == 0 || scratch), "%s: scratch %lld floats < %lld", who, (long long)scratch_floats, (long long)need);
    const R2gSpan outs[] = {{"dw", dw, Ca * 3 * wd}, {"dbias", dbias, Ca}, {"dnscale", dnscale, Ca}, {"dnshift", dnshift, Ca}, {"scratch", scratch, need}};
    const R2gSpan ins[] = {{"x", x, rows * ldx}, {"y", y, rows * ldy}, {"a", a, rows * lda}, {"gt", gt, rows * ldgt}, {"nscale", nscale, Ca}};
    if (int rc = r2g_no_overlap(who, outs, 5, ins, 5)) return rc;
    if (int rc = r2g_no_overlap(who, outs, 4, outs + 4, 1)) return rc;

    hipStream_t st = (hipStream_t)stream;
    if (nslots > 0) {
        const int64_t nct = (T + R2G_CHUNK - 1) / R2G_CHUNK, total = B * nct;          // < 2^31: B < 2^16, nct <= 2^25 ... checked below
        KTF_REQUIRE(total < (1ll << 31), "%s: B * ceil(T / 32) reaches 2^31", who);
        const float* am = nscale ? a : y;
        Res2GradWParams p = {x, y, am, gt, nscale, lens, scratch, T, ldx, ldy, nscale ? lda : ldy, ldgt, per, scale, dilation, act == KTF_ACT_RELU,
                             nscale ? 0 : wd, (int32_t)nct, (int32_t)((total + nslots - 1) / nslots), (int32_t)total,
                             ((uintptr_t)x & 15) == 0, ((uintptr_t)y & 15) == 0, ((uintptr_t)am & 15) == 0, ((uintptr_t)gt & 15) == 0};
        const dim3 grid((unsigned)nslots, (unsigned)(scale - 1), 3u);
        const int lds = 4 * wd * R2G_TP * 4;
        r2g_launch(p, gemm, wd / 16, grid, lds, st);
        KTF_CHECK_LAUNCH(who);
    }
    hipLaunchKernelGGL(res2_grad_reduce_kernel, dim3((unsigned)ktf_cdiv(per, 256)), dim3(256), 0, st, scratch, nslots, per, Ca * 3 * wd, wd, dw, dbias,
                       dnscale, dnshift);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
