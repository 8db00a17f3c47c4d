// The squeeze-excitation gate of an SE-Res2Block with the skip connection fused in: include/ktf_se.h states the arithmetic as numbered
// rules, INTEGRATION.md section 2t the use, DESIGN.md section 7 the traffic.
//
//   ktf_se_gate[_train]      se_squeeze_kernel<false>   one workgroup = one utterance x CW columns: mu = mean_t x (rule 2)
//                            se_excite_kernel<false>    one workgroup = 16 utterances x a block of C: h and the gate on fp64 MFMA (rule 3)
//                            se_scale_kernel            one workgroup = one utterance x a tile of rows: y = x s (+ r) (rule 4)
//   ktf_se_gate_backward     se_squeeze_kernel<true>    ds = sum_t g x
//                            se_excite_kernel<true>     dz2, dh and dmu / len: the forward's two products with the weights transposed
//                            se_param_grad_kernel       one wave = a 16 x 16 tile of dW2 | db2 or dW1 | db1 over all b ascending
//                            se_scale_grad_kernel       dx = g s + dmu / len, zero rows beyond the length
//
// The squeeze has the two thread mappings of attn_pool_kernel: CW = 256 columns as 16 row groups of 64 lanes (a float4 per lane), four
// canonical groups per thread, or CW = 64 columns as 64 row groups of 16 lanes, one group per thread -- four times the workgroups and
// a quarter of the serial chain when B C alone leaves compute units idle. Both end in ap_total (canon_sum.h): the same bits.
#include "common.h"
#include "canon_sum.h"
#include "f64_mfma.h"
#include "../../include/ktf_se.h"

// every operation is rounded on its own: no contraction into fma, in any kernel of this file
#pragma clang fp contract(off)

#define SE_SQ_THREADS 1024
#define SE_EX_THREADS 1024       // 16 waves: each takes output column tiles w, w + 16, ...
#define SE_EX_WAVES 16
#define SE_EX_KC 128             // channels of the first product's left operand staged in LDS at a time
#define SE_EX_T1 4               // column tiles of the first product per wave: H <= 1024 = 16 waves x 4 tiles x 16 columns
#define SE_SC_THREADS 256

typedef __attribute__((ext_vector_type(4))) float se_fv4;

__device__ __forceinline__ se_fv4 se_load4(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const se_fv4*>(p);
    return se_fv4{p[0], p[1], p[2], p[3]};
}
__device__ __forceinline__ void se_store4(float* p, se_fv4 v, bool vec) {
    if (vec) {
        *reinterpret_cast<se_fv4*>(p) = v;
    } else {
        p[0] = v[0], p[1] = v[1], p[2] = v[2], p[3] = v[3];
    }
}

// ------------------------------------------------------------------------------------ squeeze: mu (rule 2) or ds (rule 7)
template <bool PROD, int CW>
__global__ __launch_bounds__(SE_SQ_THREADS) void se_squeeze_kernel(const float* __restrict__ x, int64_t T, int C, int64_t ldx,
                                                                   const float* __restrict__ g, int64_t ldg,
                                                                   const int32_t* __restrict__ lens, int vec, double* __restrict__ out) {
    constexpr int LPR = CW / 4;                  // lanes per row group: a float4 of columns each
    constexpr int RG = SE_SQ_THREADS / LPR;      // row groups per workgroup: 16 or 64
    constexpr int NG = 64 / RG;                  // canonical groups per thread: 4 or 1
    __shared__ double red[RG][CW];
    const int b = blockIdx.y;
    const int len = ap_len(lens, b, T);
    const int lc = threadIdx.x % LPR, rg = threadIdx.x / LPR;
    const int c0 = blockIdx.x * CW + lc * 4;
    double s[NG][4];
#pragma unroll
    for (int q = 0; q < NG; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) s[q][i] = 0.;
    if (c0 < C) {                                // (C % 4 == 0: the lane's four columns exist together)
        const float* xb = x + (int64_t)b * T * ldx + c0;
        const float* gb = PROD ? g + (int64_t)b * T * ldg + c0 : nullptr;
#pragma unroll 2
        for (int t0 = rg; t0 < len; t0 += 64) {
#pragma unroll
            for (int q = 0; q < NG; ++q) {
                const int t = t0 + q * RG;
                if (t < len) {
                    const se_fv4 v = se_load4(xb + (int64_t)t * ldx, vec);
                    if (PROD) {
                        const se_fv4 w = se_load4(gb + (int64_t)t * ldg, vec);
#pragma unroll
                        for (int i = 0; i < 4; ++i) s[q][i] += (double)w[i] * (double)v[i];
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) s[q][i] += (double)v[i];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        red[rg][lc * 4 + i] = NG == 4 ? ((s[0][i] + s[1 % NG][i]) + s[2 % NG][i]) + s[3 % NG][i] : s[0][i];
    __syncthreads();
    if (threadIdx.x < CW) {
        const int c = blockIdx.x * CW + threadIdx.x;
        if (c < C) {
            const double S = ap_total<RG>(&red[0][threadIdx.x], CW);
            out[(int64_t)b * C + c] = PROD ? S : (len > 0 ? S / (double)len : 0.0);
        }
    }
}

// ------------------------------------------------------------------------------------ excite (rule 3) and its gradient (rule 7)
// Both are P (16 x C) -> Q = post(init + P M1) (16 x H, kept in LDS) -> R = init2 + Q M2 (16 x C) for a tile of 16 utterances:
//   forward   P = mu,                 M1 = W1,    init = b1, post = relu,        M2 = W2,    init2 = b2, out = sigmoid -> gate
//   GRAD      P = ds (s (1 - s)),     M1 = W2^T,  init = 0,  post = [hid > 0],   M2 = W1^T,  init2 = 0,  out = R / len -> dmu
// Lane l of a wave holds left[row l & 15][k = l >> 4] and right[k = l >> 4][col l & 15]; result register r is [row (l >> 4) + 4 r]
// [col l & 15] (f64_mfma.hip). P goes through LDS in chunks of SE_EX_KC channels (16 x 4096 fp64 would not fit), the weights come
// as fp32 from global / L2 and are widened in registers. blockIdx.y takes a block of the C output columns of the second product
// and computes all of Q for itself; block 0 writes the side outputs (hid | dz2, dh).
template <bool GRAD>
__global__ __launch_bounds__(SE_EX_THREADS) void se_excite_kernel(int B, int C, int H, int64_t T, const int32_t* __restrict__ lens,
                                                                  const double* __restrict__ P, const float* __restrict__ gate_in,
                                                                  const float* __restrict__ w1, const float* __restrict__ b1,
                                                                  const float* __restrict__ w2, const float* __restrict__ b2,
                                                                  const double* __restrict__ hid_in, double* __restrict__ side_p,
                                                                  double* __restrict__ side_q, float* __restrict__ gate_out,
                                                                  double* __restrict__ dmu_out) {
    extern __shared__ double se_lds[];
    __shared__ int slen[16];
    const int H4 = (H + 3) & ~3, HS = H4 + 1;            // Q row stride (odd: the 16 rows fall on different banks)
    double* qs = se_lds;                                 // [16][HS]
    double* ps = se_lds + 16 * HS;                       // [16][SE_EX_KC + 1]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const int b0 = blockIdx.x * 16;
    if (threadIdx.x < 16) slen[threadIdx.x] = b0 + threadIdx.x < B ? ap_len(lens, b0 + threadIdx.x, T) : 0;
    for (int i = threadIdx.x; i < 16 * HS; i += SE_EX_THREADS) qs[i] = 0.;
    const int nt1 = (H + 15) >> 4;

    f64x4 acc[SE_EX_T1];
#pragma unroll
    for (int i = 0; i < SE_EX_T1; ++i) {
        const int col = (wave + SE_EX_WAVES * i) * 16 + lc;
        const double v0 = (!GRAD && b1 && col < H) ? (double)b1[col] : 0.;
        acc[i] = f64x4{v0, v0, v0, v0};
    }
    for (int cb = 0; cb < C; cb += SE_EX_KC) {
        const int kc = C - cb < SE_EX_KC ? C - cb : SE_EX_KC;    // a multiple of 4
        __syncthreads();                                          // the last chunk has been read (first pass: slen, qs)
        for (int i = threadIdx.x; i < 16 * SE_EX_KC; i += SE_EX_THREADS) {
            const int row = i / SE_EX_KC, k = i % SE_EX_KC;
            const int b = b0 + row, c = cb + k;
            double v = 0.;
            if (b < B && k < kc) {
                v = P[(int64_t)b * C + c];
                if (GRAD) {
                    const double s = (double)gate_in[(int64_t)b * C + c];
                    v = v * (s * (1. - s));
                    if (blockIdx.y == 0) side_p[(int64_t)b * C + c] = v;       // dz2 for the parameter gradients
                }
            }
            ps[row * (SE_EX_KC + 1) + k] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < SE_EX_T1; ++i) {
            const int jt = wave + SE_EX_WAVES * i;
            if (jt < nt1) {                                       // (uniform over the wave)
                const int col = jt * 16 + lc;
                for (int k0 = 0; k0 < kc; k0 += 4) {
                    const int c = cb + k0 + lk;
                    const double a = ps[lc * (SE_EX_KC + 1) + k0 + lk];
                    double bv = 0.;
                    if (col < H) bv = GRAD ? (double)w2[(int64_t)col * C + c] : (double)w1[(int64_t)c * H + col];
                    acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[i], 0, 0, 0);
                }
            }
        }
    }
    // Q into LDS (rows of absent or empty utterances as +0, rule 5) and, from block 0, into its side output
#pragma unroll
    for (int i = 0; i < SE_EX_T1; ++i) {
        const int jt = wave + SE_EX_WAVES * i;
        const int col = jt * 16 + lc;
        if (jt < nt1 && col < H) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = lk + 4 * r, b = b0 + row;
                double v = acc[i][r];
                if (GRAD) v = (b < B && hid_in[(int64_t)b * H + col] > 0.) ? v : 0.;
                else v = v < 0. ? 0. : v;
                if (slen[row] == 0) v = 0.;
                qs[row * HS + col] = v;
                if (blockIdx.y == 0 && b < B && side_q) side_q[(int64_t)b * H + col] = v;
            }
        }
    }
    __syncthreads();
    // the second product: this block's column tiles of C, dealt to the waves
    const int nt2 = (C + 15) >> 4;
    const int per = (nt2 + (int)gridDim.y - 1) / (int)gridDim.y;
    const int ct0 = blockIdx.y * per, ct1 = ct0 + per < nt2 ? ct0 + per : nt2;
    for (int ct = ct0 + wave; ct < ct1; ct += SE_EX_WAVES) {
        const int col = ct * 16 + lc;
        const double v0 = (!GRAD && b2 && col < C) ? (double)b2[col] : 0.;
        f64x4 z = f64x4{v0, v0, v0, v0};
        for (int k0 = 0; k0 < H4; k0 += 4) {
            const int j = k0 + lk;
            const double a = qs[lc * HS + j];
            double bv = 0.;
            if (j < H && col < C) bv = GRAD ? (double)w1[(int64_t)col * H + j] : (double)w2[(int64_t)j * C + col];
            z = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, z, 0, 0, 0);
        }
        if (col < C) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = lk + 4 * r, b = b0 + row;
                if (b < B) {
                    const int len = slen[row];
                    if (GRAD) dmu_out[(int64_t)b * C + col] = len > 0 ? z[r] / (double)len : 0.;
                    else gate_out[(int64_t)b * C + col] = len > 0 ? (float)(1. / (1. + exp(-z[r]))) : 0.f;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------ parameter gradients (rule 7)
// Tiles [0, nA): dW2 (H x C) = hid^T dz2 with db2 as the row H of a left operand of ones; tiles [nA, nA + nB): dW1 (C x H) = mean^T dh
// with db1 as the row C. One wave owns a 16 x 16 tile over all b ascending, four per MFMA: no slots, no second reduction.
__global__ __launch_bounds__(256) void se_param_grad_kernel(int B, int C, int H, const double* __restrict__ mean,
                                                            const double* __restrict__ hid, const double* __restrict__ dz2,
                                                            const double* __restrict__ dh, float* __restrict__ dw1, float* __restrict__ db1,
                                                            float* __restrict__ dw2, float* __restrict__ db2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const int ncC = (C + 15) >> 4, ncH = (H + 15) >> 4;
    const int nA = ((H + 16) >> 4) * ncC, nB = ((C + 16) >> 4) * ncH;
    int tile = blockIdx.x * 4 + wave;
    if (tile >= nA + nB) return;
    const bool second = tile >= nA;
    if (second) tile -= nA;
    const int M = second ? C : H, N = second ? H : C;            // the product is (M + 1) x N
    const int nc = second ? ncH : ncC;
    const double* L = second ? mean : hid;                       // (B, M)
    const double* R = second ? dh : dz2;                         // (B, N)
    float* dw = second ? dw1 : dw2;
    float* db = second ? db1 : db2;
    if (!dw && !db) return;
    const int m = (tile / nc) * 16 + lc, n = (tile % nc) * 16 + lc;
    f64x4 acc = f64x4{0., 0., 0., 0.};
    for (int k0 = 0; k0 < B; k0 += 4) {
        const int b = k0 + lk;
        double a = 0., bv = 0.;
        if (b < B) {
            a = m < M ? L[(int64_t)b * M + m] : (m == M ? 1. : 0.);
            if (n < N) bv = R[(int64_t)b * N + n];
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc, 0, 0, 0);
    }
    if (n < N) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = (tile / nc) * 16 + lk + 4 * r;
            if (row < M) {
                if (dw) dw[(int64_t)row * N + n] = (float)acc[r];
            } else if (row == M) {
                if (db) db[n] = (float)acc[r];
            }
        }
    }
}

// ------------------------------------------------------------------------------------ scale (rule 4) and its gradient
// One workgroup = RT rows of one utterance. CT lanes (a power of two) lie along the float4 columns, 256 / CT rows are in flight
// at a time; a thread keeps the gate of its float4 column in registers and walks the rows, four loads ahead of the stores.
// r and y carry no __restrict__: y may be r itself, each element read before it is written by the same thread.
template <bool RES>
__global__ __launch_bounds__(SE_SC_THREADS) void se_scale_kernel(const float* __restrict__ x, int64_t T, int C, int64_t ldx, const float* r,
                                                                 int64_t ldr, const int32_t* __restrict__ lens,
                                                                 const float* __restrict__ gate, int CT, int RT, int vec, float* y,
                                                                 int64_t ldy) {
    const int b = blockIdx.y;
    const int len = ap_len(lens, b, T);
    const int64_t t0 = (int64_t)blockIdx.x * RT;
    const int64_t t1 = t0 + RT < len ? t0 + RT : len;
    if (t0 >= t1) return;
    const int ci = threadIdx.x & (CT - 1), rl = threadIdx.x / CT, RL = SE_SC_THREADS / CT;
    const int nc4 = C >> 2;
    for (int c4 = ci; c4 < nc4; c4 += CT) {
        const se_fv4 s = *reinterpret_cast<const se_fv4*>(gate + (int64_t)b * C + c4 * 4);
        const float* xb = x + (int64_t)b * T * ldx + c4 * 4;
        const float* rb = RES ? r + (int64_t)b * T * ldr + c4 * 4 : nullptr;
        float* yb = y + (int64_t)b * T * ldy + c4 * 4;
        for (int64_t t = t0 + rl; t < t1; t += 4 * RL) {
            se_fv4 v[4], q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t tu = t + (int64_t)u * RL;
                if (tu < t1) {
                    v[u] = se_load4(xb + tu * ldx, vec);
                    if (RES) q[u] = se_load4(rb + tu * ldr, vec);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t tu = t + (int64_t)u * RL;
                if (tu < t1) {
                    se_fv4 o = v[u] * s;
                    if (RES) o = o + q[u];
                    se_store4(yb + tu * ldy, o, vec);
                }
            }
        }
    }
}

__global__ __launch_bounds__(SE_SC_THREADS) void se_scale_grad_kernel(const float* __restrict__ g, int64_t T, int C, int64_t ldg,
                                                                      const int32_t* __restrict__ lens, const float* __restrict__ gate,
                                                                      const double* __restrict__ dmu, int CT, int RT, int vec,
                                                                      float* __restrict__ dx, int64_t lddx) {
    const int b = blockIdx.y;
    const int len = ap_len(lens, b, T);
    const int64_t t0 = (int64_t)blockIdx.x * RT;
    const int64_t t2 = t0 + RT < T ? t0 + RT : T;                // the tile's rows
    const int64_t t1 = t2 < len ? t2 : len;                      // ... of which [t0, t1) lie inside the length
    const int ci = threadIdx.x & (CT - 1), rl = threadIdx.x / CT, RL = SE_SC_THREADS / CT;
    const int nc4 = C >> 2;
    for (int c4 = ci; c4 < nc4; c4 += CT) {
        const float* gb = g + (int64_t)b * T * ldg + c4 * 4;
        float* db = dx + (int64_t)b * T * lddx + c4 * 4;
        if (t0 < t1) {
            const se_fv4 s = *reinterpret_cast<const se_fv4*>(gate + (int64_t)b * C + c4 * 4);
            double sd[4], dm[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sd[i] = (double)s[i];
                dm[i] = dmu[(int64_t)b * C + c4 * 4 + i];
            }
            for (int64_t t = t0 + rl; t < t1; t += 4 * RL) {
                se_fv4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t tu = t + (int64_t)u * RL;
                    if (tu < t1) v[u] = se_load4(gb + tu * ldg, vec);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t tu = t + (int64_t)u * RL;
                    if (tu < t1) {
                        se_fv4 o;
#pragma unroll
                        for (int i = 0; i < 4; ++i) o[i] = (float)((double)v[u][i] * sd[i] + dm[i]);
                        se_store4(db + tu * lddx, o, vec);
                    }
                }
            }
        }
        const int64_t z0 = t0 > t1 ? t0 : t1;                    // rows at and beyond the length: zero in [0, C)
        for (int64_t t = z0 + rl; t < t2; t += RL) se_store4(db + t * lddx, se_fv4{0.f, 0.f, 0.f, 0.f}, vec);
    }
}

// ------------------------------------------------------------------------------------ entry points
static bool se_overlap(const void* a, int64_t abytes, const void* b, int64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    const uintptr_t an = a0 + (uintptr_t)abytes < a0 ? UINTPTR_MAX : a0 + (uintptr_t)abytes;      // (saturating ends)
    const uintptr_t bn = b0 + (uintptr_t)bbytes < b0 ? UINTPTR_MAX : b0 + (uintptr_t)bbytes;
    return a0 < bn && b0 < an;
}

static int se_check_sizes(const char* who, int64_t B, int64_t T, int32_t C, int32_t H) {
    KTF_REQUIRE(B >= 0 && T >= 0, "%s: B and T must be >= 0", who);
    KTF_REQUIRE(B <= KTF_SE_MAX_BATCH && T <= KTF_SE_MAX_ROWS, "%s: B %lld above %d or T %lld above %d", who, (long long)B, KTF_SE_MAX_BATCH,
                (long long)T, KTF_SE_MAX_ROWS);
    KTF_REQUIRE(C >= 4 && C % 4 == 0 && C <= KTF_SE_MAX_DIM, "%s: C %d is not a multiple of 4 in [4, %d]", who, (int)C, KTF_SE_MAX_DIM);
    KTF_REQUIRE(H >= 1 && H <= KTF_SE_MAX_HIDDEN, "%s: H %d outside [1, %d]", who, (int)H, KTF_SE_MAX_HIDDEN);
    return KTF_OK;
}

static int se_check_ld(const char* who, const char* name, int64_t ld, int32_t C) {
    KTF_REQUIRE(ld >= C && ld % 4 == 0 && ld < (1ll << 31), "%s: %s %lld below C = %d, not a multiple of 4 or at 2^31", who, name, (long long)ld,
                (int)C);
    return KTF_OK;
}

// bytes from the first to behind the last element of (B, T, ld) rows of C columns, saturating (B T ld can pass 2^63 at the limits)
static int64_t se_span(int64_t B, int64_t T, int64_t ld, int32_t C) {
    int64_t n = 0;
    if (__builtin_mul_overflow(B * T - 1, ld, &n) || __builtin_add_overflow(n, (int64_t)C, &n) || __builtin_mul_overflow(n, (int64_t)4, &n)) return INT64_MAX;
    return n;
}

static void se_scale_shape(int64_t B, int64_t T, int32_t C, int* CT, int* RT) {
    int ct = 1;
    while (ct < C / 4 && ct < SE_SC_THREADS) ct <<= 1;
    *CT = ct;
    // rows per workgroup: fewer when the grid would leave compute units idle (the values do not depend on it)
    *RT = (int64_t)ktf_cdiv(T, 64) * B < 1024 ? 16 : 64;
    if (*RT < SE_SC_THREADS / ct) *RT = SE_SC_THREADS / ct;
}

static size_t se_excite_lds(int32_t H) { return (size_t)(16 * (((H + 3) & ~3) + 1) + 16 * (SE_EX_KC + 1)) * sizeof(double); }

// column blocks of the excite launch: few utterance tiles are spread over more workgroups, each recomputing Q
static int se_excite_blocks(int64_t B, int32_t C) {
    const int tiles = ktf_cdiv(B, 16), nt2 = ktf_cdiv(C, 16);
    int nb = tiles >= 64 ? 1 : ktf_cdiv(64, tiles);
    const int most = ktf_cdiv(nt2, SE_EX_WAVES);                  // at least one column tile per wave
    return nb > most ? most : nb;
}

static void se_launch_squeeze(bool prod, const float* x, int64_t B, int64_t T, int32_t C, int64_t ldx, const float* g, int64_t ldg,
                              const int32_t* lens, int vec, double* out, hipStream_t st) {
    // few workgroups: the 64-column mapping (4x the workgroups, the same bits)
    const bool wide = (int64_t)ktf_cdiv(C, 256) * B >= 256;
#define SE_SQ(P, CW) \
    hipLaunchKernelGGL((se_squeeze_kernel<P, CW>), dim3((unsigned)ktf_cdiv(C, CW), (unsigned)B), dim3(SE_SQ_THREADS), 0, st, x, T, (int)C, ldx, g, ldg, lens, vec, out)
    if (prod) {
        if (wide) SE_SQ(true, 256); else SE_SQ(true, 64);
    } else {
        if (wide) SE_SQ(false, 256); else SE_SQ(false, 64);
    }
#undef SE_SQ
}

static int se_forward(const char* who, bool train, const float* x, int64_t B, int64_t T, int32_t C, int64_t ldx, const float* r, int64_t ldr,
                      const int32_t* lens, const float* w1, const float* b1, const float* w2, const float* b2, int32_t H, float* y, int64_t ldy,
                      double* mean, double* hid, float* gate, void* stream) {
    int rc = se_check_sizes(who, B, T, C, H);
    if (rc != KTF_OK) return rc;
    if ((rc = se_check_ld(who, "ldx", ldx, C)) != KTF_OK || (rc = se_check_ld(who, "ldy", ldy, C)) != KTF_OK) return rc;
    if (r && (rc = se_check_ld(who, "ldr", ldr, C)) != KTF_OK) return rc;
    const int64_t rows = B * T;
    if (rows == 0) return KTF_OK;
    KTF_REQUIRE(x && y && w1 && w2 && gate && (!train || (mean && hid)), "%s: null argument", who);
    KTF_REQUIRE(((uintptr_t)gate & 255) == 0, "%s: gate not 256-byte aligned", who);
    KTF_REQUIRE(!train || ((((uintptr_t)mean | (uintptr_t)hid) & 7) == 0), "%s: mean or hid not 8-byte aligned", who);
    KTF_REQUIRE(!se_overlap(y, se_span(B, T, ldy, C), x, se_span(B, T, ldx, C)), "%s: y overlaps x", who);
    if (r && se_overlap(y, se_span(B, T, ldy, C), r, se_span(B, T, ldr, C)))
        KTF_REQUIRE(y == r && ldy == ldr, "%s: y overlaps r without being r itself", who);
    hipStream_t st = (hipStream_t)stream;
    if (!train) mean = (double*)(gate + ((B * C + 63) / 64) * 64);       // rule 6: the means behind the gate
    const int vec = ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)r) & 15) == 0);
    se_launch_squeeze(false, x, B, T, C, ldx, nullptr, 0, lens, vec, mean, st);
    const size_t lds = se_excite_lds(H);
    KTF_LDS_ONCE(se_excite_lds(KTF_SE_MAX_HIDDEN), se_excite_kernel<false>);
    hipLaunchKernelGGL((se_excite_kernel<false>), dim3((unsigned)ktf_cdiv(B, 16), (unsigned)se_excite_blocks(B, C)), dim3(SE_EX_THREADS), lds, st,
                       (int)B, (int)C, (int)H, T, lens, (const double*)mean, (const float*)nullptr, w1, b1, w2, b2, (const double*)nullptr,
                       (double*)nullptr, train ? hid : (double*)nullptr, gate, (double*)nullptr);
    int CT, RT;
    se_scale_shape(B, T, C, &CT, &RT);
    const dim3 grid((unsigned)ktf_cdiv(T, RT), (unsigned)B);
    if (r) hipLaunchKernelGGL((se_scale_kernel<true>), grid, dim3(SE_SC_THREADS), 0, st, x, T, (int)C, ldx, r, ldr, lens, (const float*)gate, CT, RT, vec, y, ldy);
    else hipLaunchKernelGGL((se_scale_kernel<false>), grid, dim3(SE_SC_THREADS), 0, st, x, T, (int)C, ldx, r, ldr, lens, (const float*)gate, CT, RT, vec, y, ldy);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_se_gate(const float* x, int64_t B, int64_t T, int32_t C, int64_t ldx, const float* r, int64_t ldr, const int32_t* lens,
                           const float* w1, const float* b1, const float* w2, const float* b2, int32_t H, float* y, int64_t ldy, float* gate,
                           void* stream) {
    return se_forward("ktf_se_gate", false, x, B, T, C, ldx, r, ldr, lens, w1, b1, w2, b2, H, y, ldy, nullptr, nullptr, gate, stream);
}

extern "C" int ktf_se_gate_train(const float* x, int64_t B, int64_t T, int32_t C, int64_t ldx, const float* r, int64_t ldr, const int32_t* lens,
                                 const float* w1, const float* b1, const float* w2, const float* b2, int32_t H, float* y, int64_t ldy,
                                 double* mean, double* hid, float* gate, void* stream) {
    return se_forward("ktf_se_gate_train", true, x, B, T, C, ldx, r, ldr, lens, w1, b1, w2, b2, H, y, ldy, mean, hid, gate, stream);
}

extern "C" int64_t ktf_se_gate_backward_workspace_bytes(int64_t B, int32_t C, int32_t H) {
    const int rc = se_check_sizes("ktf_se_gate_backward_workspace_bytes", B, 0, C, H);
    if (rc != KTF_OK) return rc;
    const int64_t rows = B > 0 ? B : 1;
    return 3 * al256(rows * C * 8) + al256(rows * H * 8);
}

extern "C" int ktf_se_gate_backward(const float* g, int64_t B, int64_t T, int32_t C, int64_t ldg, const float* x, int64_t ldx,
                                    const int32_t* lens, const float* w1, const float* w2, int32_t H, const double* mean, const double* hid,
                                    const float* gate, float* dx, int64_t lddx, float* dw1, float* db1, float* dw2, float* db2,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_se_gate_backward";
    int rc = se_check_sizes(who, B, T, C, H);
    if (rc != KTF_OK) return rc;
    if ((rc = se_check_ld(who, "ldg", ldg, C)) != KTF_OK || (rc = se_check_ld(who, "ldx", ldx, C)) != KTF_OK ||
        (rc = se_check_ld(who, "lddx", lddx, C)) != KTF_OK)
        return rc;
    KTF_REQUIRE(workspace, "%s: null workspace", who);
    rc = ktf_check_workspace(who, workspace, workspace_bytes, ktf_se_gate_backward_workspace_bytes(B, C, H));
    if (rc != KTF_OK) return rc;
    const int64_t rows = B * T;
    if (rows > 0) {
        KTF_REQUIRE(g && x && w1 && w2 && mean && hid && gate && dx, "%s: null argument", who);
        KTF_REQUIRE(((uintptr_t)gate & 15) == 0 && ((((uintptr_t)mean | (uintptr_t)hid) & 7) == 0), "%s: gate not 16-byte or mean / hid not 8-byte aligned",
                    who);
        const int64_t nd = se_span(B, T, lddx, C);
        KTF_REQUIRE(!se_overlap(dx, nd, g, se_span(B, T, ldg, C)) && !se_overlap(dx, nd, x, se_span(B, T, ldx, C)) &&
                        !se_overlap(dx, nd, gate, B * C * 4),
                    "%s: dx overlaps g, x or gate", who);
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t Bw = B > 0 ? B : 1;
    double* ds = (double*)workspace;
    double* dz2 = (double*)((char*)workspace + al256(Bw * C * 8));
    double* dmu = (double*)((char*)workspace + 2 * al256(Bw * C * 8));
    double* dh = (double*)((char*)workspace + 3 * al256(Bw * C * 8));
    if (rows > 0) {
        const int vec = ((((uintptr_t)g | (uintptr_t)x | (uintptr_t)dx) & 15) == 0);
        se_launch_squeeze(true, x, B, T, C, ldx, g, ldg, lens, vec, ds, st);
        const size_t lds = se_excite_lds(H);
        KTF_LDS_ONCE(se_excite_lds(KTF_SE_MAX_HIDDEN), se_excite_kernel<true>);
        hipLaunchKernelGGL((se_excite_kernel<true>), dim3((unsigned)ktf_cdiv(B, 16), (unsigned)se_excite_blocks(B, C)), dim3(SE_EX_THREADS), lds, st,
                           (int)B, (int)C, (int)H, T, lens, (const double*)ds, gate, w1, (const float*)nullptr, w2, (const float*)nullptr, hid, dz2, dh,
                           (float*)nullptr, dmu);
    }
    if (dw1 || db1 || dw2 || db2) {
        const int tiles = ((H + 16) >> 4) * ktf_cdiv(C, 16) + ((C + 16) >> 4) * ktf_cdiv(H, 16);
        hipLaunchKernelGGL(se_param_grad_kernel, dim3((unsigned)ktf_cdiv(tiles, 4)), dim3(256), 0, st, rows > 0 ? (int)B : 0, (int)C, (int)H, mean, hid,
                           (const double*)dz2, (const double*)dh, dw1, db1, dw2, db2);
    }
    if (rows > 0) {
        const int vec = ((((uintptr_t)g | (uintptr_t)x | (uintptr_t)dx) & 15) == 0);
        int CT, RT;
        se_scale_shape(B, T, C, &CT, &RT);
        hipLaunchKernelGGL(se_scale_grad_kernel, dim3((unsigned)ktf_cdiv(T, RT), (unsigned)B), dim3(SE_SC_THREADS), 0, st, g, T, (int)C, ldg, lens, gate,
                           (const double*)dmu, CT, RT, vec, dx, lddx);
    }
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
