// Attentive statistics pooling (Okabe et al. 2018; single-head, multi-head and channel-wise), forward and backward:
// include/ktf_attn.h states the arithmetic as numbered rules, INTEGRATION.md section 2r the use, DESIGN.md section 7 the traffic.
//
//   ktf_attn_pool            attn_norm_kernel   one workgroup = one utterance x CW heads: m = max_t e, then Z = sum_t exp(e - m)
//                            attn_pool_kernel   one workgroup = one utterance x CW columns: sum_t p x and sum_t p x^2, finalize
//   ktf_attn_pool_backward   attn_coef_kernel   one wave = one utterance x one head step: a_c, b_c and K_j = sum_c (a mu + b q)
//                            attn_grad_kernel   one wave = one utterance x one head step x a tile of rows: dx and de, one pass
//
// Sums over t (rule 8) follow stats_pool_kernel of pool_post.hip: row t -> group t mod 64 in ascending order, the groups combined as
// ((g + g+16) + g+32) + g+48 for g = 0..15 and then over g in ascending order, whichever of the two thread mappings runs. Sums over
// the channels of a head (rule 12) have one definition too: slot l of 64 adds the head's channels l, l + 64, ... in ascending order
// starting from +0, and the slots are added by a butterfly over the distances 32, 16, 8, 4, 2, 1. A head of at most 32 channels
// shares its wave with others: its slots beyond the channel count hold +0, so the first stages of the butterfly add +0 and are
// replaced by one `+ 0.0`, which gives the same bits.
#include "common.h"
#include "../../include/ktf_attn.h"

// An utterance without a row (rule 10): the finalize of stats_pool_kernel (pool_post.hip) on its sums s = q = 0 and n = 0, in that
// kernel's expression and contraction mode, so that the NaN of 0 / 0 comes out with the same sign bits in both columns.
__device__ __forceinline__ void ap_empty_row(double s, double q, double n, int include_std, float eps, float* mean_out, float* std_out) {
    const double mean = s / n;
    *mean_out = (float)mean;
    if (include_std) {
        const double var = q / n - mean * mean;
        *std_out = (float)sqrt((var < 0.0 ? 0.0 : var) + (double)eps);
    }
}

// every fp64 operation is rounded on its own: no contraction into fma, in any instantiation
#pragma clang fp contract(off)

#define AP_THREADS 1024

__device__ __forceinline__ double ap_keep_nan_relu(double v) { return v < 0.0 ? 0.0 : v; }    // NaN < 0 is false: NaN stays

// the canonical total of one column of red[RG][..][CW] (slot g of RG at r[g * stride])
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

// ------------------------------------------------------------------------------------ m and Z of every (utterance, head)
template <int CW>
__global__ __launch_bounds__(AP_THREADS) void attn_norm_kernel(const float* __restrict__ e, int64_t T, int H, int64_t lde,
                                                               const int32_t* __restrict__ lens, double* __restrict__ norm) {
    constexpr int RG = AP_THREADS / CW;          // row groups per workgroup: 16 or 64
    constexpr int NG = 64 / RG;                  // canonical groups per thread: 4 or 1
    __shared__ double red[RG][CW];
    __shared__ double mx[CW];
    const int b = blockIdx.y;
    const int len = ap_len(lens, b, T);
    const int lc = threadIdx.x % CW, rg = threadIdx.x / CW;
    const int j = blockIdx.x * CW + lc;
    const float* eb = e + (int64_t)b * T * lde + j;
    float m = -INFINITY;
    if (j < H)
        for (int t = rg; t < len; t += RG) m = fmaxf(m, eb[(int64_t)t * lde]);
    red[rg][lc] = (double)m;
    __syncthreads();
    if (threadIdx.x < CW) {
        double v = red[0][lc];
        for (int g = 1; g < RG; ++g) v = fmax(v, red[g][lc]);
        mx[lc] = v;
    }
    __syncthreads();
    const double md = mx[lc];
    double z[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) z[g] = 0.;
    if (j < H)
        for (int t0 = rg; t0 < len; t0 += 64) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int t = t0 + g * RG;
                if (t < len) z[g] += exp((double)eb[(int64_t)t * lde] - md);
            }
        }
    red[rg][lc] = NG == 4 ? ((z[0] + z[1 % NG]) + z[2 % NG]) + z[3 % NG] : z[0];
    __syncthreads();
    if (threadIdx.x < CW && j < H) {
        double* n = norm + ((int64_t)b * H + j) * 2;
        n[0] = md;
        n[1] = ap_total<RG>(&red[0][lc], CW);
    }
}

// ------------------------------------------------------------------------------------ the weighted sums and the outputs
template <int CW>
__global__ __launch_bounds__(AP_THREADS) void attn_pool_kernel(const float* __restrict__ x, int64_t T, int D, int64_t ldx,
                                                               const float* __restrict__ e, int H, int64_t lde,
                                                               const int32_t* __restrict__ lens, int include_std, float eps,
                                                               const double* __restrict__ norm, float* __restrict__ out, int64_t ldo,
                                                               double* __restrict__ stats) {
    constexpr int RG = AP_THREADS / CW;
    constexpr int NG = 64 / RG;
    __shared__ double red[RG][2][CW];
    const int b = blockIdx.y;
    const int len = ap_len(lens, b, T);
    const int lc = threadIdx.x % CW, rg = threadIdx.x / CW;
    const int c = blockIdx.x * CW + lc;
    const int j = c < D ? c / (D / H) : 0;
    const double* nj = norm + ((int64_t)b * H + j) * 2;
    double s[NG], q[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) s[g] = q[g] = 0.;
    if (c < D) {
        const double m = nj[0];
        const float* xb = x + (int64_t)b * T * ldx + c;
        const float* eb = e + (int64_t)b * T * lde + j;
#pragma unroll 2
        for (int t0 = rg; t0 < len; t0 += 64) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int t = t0 + g * RG;
                if (t < len) {
                    const double v = (double)xb[(int64_t)t * ldx];
                    const double p = exp((double)eb[(int64_t)t * lde] - m);
                    s[g] += p * v;
                    q[g] += p * (v * v);
                }
            }
        }
    }
    red[rg][0][lc] = NG == 4 ? ((s[0] + s[1 % NG]) + s[2 % NG]) + s[3 % NG] : s[0];
    red[rg][1][lc] = NG == 4 ? ((q[0] + q[1 % NG]) + q[2 % NG]) + q[3 % NG] : q[0];
    __syncthreads();
    if (threadIdx.x < CW && c < D) {
        const double Z = nj[1];
        const double S = ap_total<RG>(&red[0][0][lc], 2 * CW), Q = ap_total<RG>(&red[0][1][lc], 2 * CW);
        const double mu = S / Z, qq = Q / Z;
        if (len == 0) {
            ap_empty_row(S, Q, (double)len, include_std, eps, &out[(int64_t)b * ldo + c], &out[(int64_t)b * ldo + D + c]);
        } else {
            out[(int64_t)b * ldo + c] = (float)mu;
            if (include_std) out[(int64_t)b * ldo + D + c] = (float)sqrt(ap_keep_nan_relu(qq - mu * mu) + (double)eps);
        }
        if (stats) {
            stats[((int64_t)b * 2 + 0) * D + c] = mu;
            stats[((int64_t)b * 2 + 1) * D + c] = qq;
        }
    }
}

// ------------------------------------------------------------------------------------ backward
// Lanes of a wave on the heads of its step: a head of dh channels takes a segment of P2 = min(64, next power of two >= dh) lanes,
// 64 / P2 heads per step; lane l of a segment takes the head's channels l, l + P2, ... (more than one only when dh > 64).
struct ApLanes {
    int j, l, dh, P2;
    bool head;       // the lane's head exists
};
__device__ __forceinline__ ApLanes ap_lanes(int step, int D, int H, int P2) {
    ApLanes a;
    a.dh = D / H;
    a.P2 = P2;
    const int lane = threadIdx.x & 63;
    a.j = step * (64 / P2) + lane / P2;
    a.l = lane % P2;
    a.head = a.j < H;
    return a;
}
__device__ __forceinline__ double ap_head_sum(double v, int P2) {
    v = v + 0.0;
    for (int o = P2 >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a_c, b_c of rule 12 into coef (B, 2, D) and K_j = sum_{c in j} (a_c mu_c + b_c q_c) into K (B, H)
__global__ __launch_bounds__(64) void attn_coef_kernel(int D, int H, int P2, int include_std, float eps, const double* __restrict__ stats,
                                                       const float* __restrict__ gout, int64_t ldg, double* __restrict__ coef,
                                                       double* __restrict__ K) {
    const int b = blockIdx.y;
    const ApLanes L = ap_lanes(blockIdx.x, D, H, P2);
    const double* mu = stats + (int64_t)b * 2 * D;
    const double* qq = mu + D;
    const float* g = gout + (int64_t)b * ldg;
    double* ca = coef + (int64_t)b * 2 * D;
    double* cb = ca + D;
    double acc = 0.;
    if (L.head)
        for (int k = L.l; k < L.dh; k += P2) {
            const int c = L.j * L.dh + k;
            const double m = mu[c], q = qq[c];
            const double var = q - m * m;
            double a = (double)g[c], bb = 0.;
            if (include_std && var > 0.) {
                const double sg = sqrt(var + (double)eps);
                const double gs = (double)g[D + c];
                a = a - (gs * m) / sg;
                bb = gs / (2. * sg);
            }
            ca[c] = a;
            cb[c] = bb;
            acc += a * m + bb * q;
        }
    acc = ap_head_sum(acc, P2);
    if (L.head && L.l == 0) K[(int64_t)b * H + L.j] = acc;
}

// dx and de of rows [blockIdx.x * RT, + RT) of utterance blockIdx.z for the heads of step blockIdx.y; step 0 also zero-fills the
// pad columns of its rows
__global__ __launch_bounds__(64) void attn_grad_kernel(const float* __restrict__ x, int64_t T, int D, int64_t ldx, const float* __restrict__ e,
                                                       int H, int64_t lde, const int32_t* __restrict__ lens, int P2, int RT,
                                                       const double* __restrict__ norm, const double* __restrict__ coef,
                                                       const double* __restrict__ K, float* __restrict__ dx, int64_t ld_dx,
                                                       float* __restrict__ de, int64_t ld_de) {
    const int b = blockIdx.z;
    const int len = ap_len(lens, b, T);
    const ApLanes L = ap_lanes(blockIdx.y, D, H, P2);
    const bool small = L.dh <= 64;                 // one channel per lane: its coefficients stay in registers
    const double* ca = coef + (int64_t)b * 2 * D;
    const double* cb = ca + D;
    double m = 0., rz = 0., Kj = 0., a0 = 0., b0 = 0.;
    const int c0 = L.j * L.dh + L.l;
    const bool live = L.head && L.l < L.dh;        // the lane has a channel
    if (L.head && len > 0) {
        const double* nj = norm + ((int64_t)b * H + L.j) * 2;
        m = nj[0];
        rz = 1. / nj[1];
        Kj = K[(int64_t)b * H + L.j];
        if (small && live) { a0 = ca[c0]; b0 = cb[c0]; }
    }
    const float* xb = x + (int64_t)b * T * ldx;
    const float* eb = e + (int64_t)b * T * lde;
    float* dxb = dx + (int64_t)b * T * ld_dx;
    float* deb = de + (int64_t)b * T * ld_de;
    const int64_t t0 = (int64_t)blockIdx.x * RT;
    const int64_t t1 = t0 + RT < T ? t0 + RT : T;
    for (int64_t t = t0; t < t1; ++t) {
        if (t >= len) {                            // (uniform over the wave)
            if (L.head) {
                for (int k = L.l; k < L.dh; k += P2) dxb[t * ld_dx + L.j * L.dh + k] = 0.f;
                if (L.l == 0) deb[t * ld_de + L.j] = 0.f;
            }
        } else {
            double w = 0., acc = 0.;
            if (L.head) {
                w = exp((double)eb[t * lde + L.j] - m) * rz;
                for (int k = L.l; k < L.dh; k += P2) {
                    const int c = L.j * L.dh + k;
                    const double a = small ? a0 : ca[c], bb = small ? b0 : cb[c];
                    const double v = (double)xb[t * ldx + c];
                    dxb[t * ld_dx + c] = (float)(w * (a + (2. * bb) * v));
                    acc += a * v + bb * (v * v);
                }
            }
            acc = ap_head_sum(acc, P2);
            if (L.head && L.l == 0) deb[t * ld_de + L.j] = (float)(w * (acc - Kj));
        }
        if (blockIdx.y == 0) {
            const int lane = threadIdx.x & 63;
            for (int64_t c = D + lane; c < ld_dx; c += 64) dxb[t * ld_dx + c] = 0.f;
            for (int64_t c = H + lane; c < ld_de; c += 64) deb[t * ld_de + c] = 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------ entry points
static int ap_p2(int D, int H) {
    const int dh = D / H;
    int p = 1;
    while (p < dh && p < 64) p <<= 1;
    return p;
}

static int ap_check_common(const char* who, int64_t B, int64_t T, int32_t D, int64_t ldx, int32_t H, int64_t lde, float eps) {
    KTF_REQUIRE(B >= 0 && T >= 0, "%s: B and T must be >= 0", who);
    KTF_REQUIRE(D >= 1 && H >= 1 && H <= D && D % H == 0, "%s: 1 <= H <= D and D %% H == 0 are required (D %d, H %d)", who, (int)D, (int)H);
    KTF_REQUIRE(D <= KTF_ATTN_MAX_DIM, "%s: D %d above %d", who, (int)D, KTF_ATTN_MAX_DIM);
    KTF_REQUIRE(ldx >= D && lde >= H, "%s: ldx < D or lde < H", who);
    KTF_REQUIRE(eps >= 0.f && eps <= 3.4028234e38f, "%s: eps must be finite and >= 0", who);
    KTF_REQUIRE(B <= KTF_ATTN_MAX_BATCH, "%s: B %lld above %d", who, (long long)B, KTF_ATTN_MAX_BATCH);
    KTF_REQUIRE(T <= KTF_ATTN_MAX_ROWS, "%s: T %lld above %d", who, (long long)T, KTF_ATTN_MAX_ROWS);
    return KTF_OK;
}

extern "C" int ktf_attn_pool(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const float* e, int32_t H, int64_t lde,
                             const int32_t* lens, int32_t include_std, float eps, float* out, int64_t ld_out, double* norm, double* stats,
                             void* stream) {
    const char* who = "ktf_attn_pool";
    KTF_REQUIRE(out && norm && ((x && e) || T == 0), "%s: null argument", who);
    const int rc = ap_check_common(who, B, T, D, ldx, H, lde, eps);
    if (rc != KTF_OK) return rc;
    KTF_REQUIRE(ld_out >= (include_std ? 2 : 1) * (int64_t)D, "%s: ld_out too small", who);
    if (B == 0) return KTF_OK;
    hipStream_t st = (hipStream_t)stream;
    // few workgroups: the 16-column mapping (4x the workgroups, the same bits)
    if (H <= 16 || (int64_t)ktf_cdiv(H, 64) * B < 512)
        hipLaunchKernelGGL(attn_norm_kernel<16>, dim3((unsigned)ktf_cdiv(H, 16), (unsigned)B), dim3(AP_THREADS), 0, st, e, T, H, lde, lens, norm);
    else
        hipLaunchKernelGGL(attn_norm_kernel<64>, dim3((unsigned)ktf_cdiv(H, 64), (unsigned)B), dim3(AP_THREADS), 0, st, e, T, H, lde, lens, norm);
    if ((int64_t)ktf_cdiv(D, 64) * B < 512)
        hipLaunchKernelGGL(attn_pool_kernel<16>, dim3((unsigned)ktf_cdiv(D, 16), (unsigned)B), dim3(AP_THREADS), 0, st, x, T, D, ldx, e, H, lde,
                           lens, include_std, eps, norm, out, ld_out, stats);
    else
        hipLaunchKernelGGL(attn_pool_kernel<64>, dim3((unsigned)ktf_cdiv(D, 64), (unsigned)B), dim3(AP_THREADS), 0, st, x, T, D, ldx, e, H, lde,
                           lens, include_std, eps, norm, out, ld_out, stats);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int64_t ktf_attn_pool_backward_workspace_bytes(int64_t B, int32_t D, int32_t H) {
    KTF_REQUIRE(B >= 0 && B <= KTF_ATTN_MAX_BATCH && D >= 1 && D <= KTF_ATTN_MAX_DIM && H >= 1 && H <= D && D % H == 0,
                "ktf_attn_pool_backward_workspace_bytes: bad sizes");
    const int64_t rows = B > 0 ? B : 1;
    return al256(rows * 2 * D * 8) + al256(rows * H * 8);
}

extern "C" int ktf_attn_pool_backward(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const float* e, int32_t H, int64_t lde,
                                      const int32_t* lens, int32_t include_std, float eps, const double* norm, const double* stats,
                                      const float* gout, int64_t ld_gout, float* dx, int64_t ld_dx, float* de, int64_t ld_de,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_attn_pool_backward";
    KTF_REQUIRE(x && e && norm && stats && gout && dx && de && workspace, "%s: null argument", who);
    int rc = ap_check_common(who, B, T, D, ldx, H, lde, eps);
    if (rc != KTF_OK) return rc;
    KTF_REQUIRE(ld_gout >= (include_std ? 2 : 1) * (int64_t)D, "%s: ld_gout too small", who);
    KTF_REQUIRE(ld_dx >= D && ld_de >= H, "%s: ld_dx < D or ld_de < H", who);
    rc = ktf_check_workspace(who, workspace, workspace_bytes, ktf_attn_pool_backward_workspace_bytes(B, D, H));
    if (rc != KTF_OK) return rc;
    if (B == 0 || T == 0) return KTF_OK;
    hipStream_t st = (hipStream_t)stream;
    double* coef = (double*)workspace;
    double* K = (double*)((char*)workspace + al256(B * 2 * D * 8));
    const int P2 = ap_p2(D, H);
    const int steps = ktf_cdiv(H, 64 / P2);
    hipLaunchKernelGGL(attn_coef_kernel, dim3((unsigned)steps, (unsigned)B), dim3(64), 0, st, D, H, P2, include_std, eps, stats, gout, ld_gout,
                       coef, K);
    // rows per wave: fewer when the grid would leave compute units idle (the values do not depend on it)
    const int RT = (int64_t)ktf_cdiv(T, 16) * steps * B < 2048 ? 4 : 16;
    hipLaunchKernelGGL(attn_grad_kernel, dim3((unsigned)ktf_cdiv(T, RT), (unsigned)steps, (unsigned)B), dim3(64), 0, st, x, T, D, ldx, e, H, lde,
                       lens, P2, RT, norm, coef, K, dx, ld_dx, de, ld_de);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
