// Full-covariance UBM posteriors on preselected Gaussians (Kaldi's `fgmm-global-gselect-to-post`) and `add-deltas`.
//
// A (frame, slot) pair names a D x D matrix, so the pairs are turned round: bucketed by Gaussian, then every bucket is a GEMM.
//   gmm_bucket.hip     the counting sort of the pairs by Gaussian, with the unordered scatter (every pair's value is computed alone,
//                      so no bit depends on the order inside a bucket), and the cut of every bucket into items of FG_ROWS rows, so
//                      that a popular Gaussian is spread over workgroups.
//   fg_quad_kernel     one workgroup per item: inv_covars_g and means_invcovars_g in LDS; each wave gathers 32 rows of x at a time
//                      into LDS (transposed) and runs Y^T = inv_covars_g . X^T on v_mfma_f32_32x32x2_f32 (exact fp32, k ascending):
//                      the frame is on the lane, Y's dimensions in the accumulators, so the row dot sum_j x_j (mi_j - y_j / 2) is
//                      taken in registers in an order that depends on D alone; gconst added; written to ll[pair].
//   fg_softmax_kernel  one wave per frame: softmax over the listed slots (and, for ktf_fgmm_post_ll_f32, the frame's log-likelihood
//                      before pruning), prune below min_post, renormalise, sort.
//   adddeltas_kernel   one thread per output element, unfused multiply and add (fp contract off) in tap order.
#include "gmm_bucket.h"

namespace {

constexpr int FG_THREADS = 256;
constexpr int FG_WAVES = FG_THREADS / 64;
constexpr int FG_ROWS = 512;        // rows of a bucket per quadratic-form workgroup
constexpr int FG_XLD = 33;          // row stride of the transposed x tile (32 frames + 1: conflict-free transposed writes)

struct FgLayout {
    SecLayout sec;
    int64_t istart, ll, total;
};

FgLayout fg_layout(int64_t F, int64_t I, int64_t n) {
    FgLayout l;
    l.sec = sec_layout(F, I, n, false);
    int64_t at = l.sec.bytes;
    l.istart = at; at += al256((I + 1) * 4);
    l.ll = at;     at += al256(F * n * 4);
    l.total = at;
    return l;
}

inline int fg_dk(int D) { return (D + 1) & ~1; }
inline int fg_dp(int D) { return (D + 31) & ~31; }
inline size_t fg_quad_lds(int D) { return (size_t)4 * (fg_dk(D) * fg_dp(D) + fg_dp(D) + FG_WAVES * fg_dp(D) * FG_XLD); }

// NJ = Dp / 32 blocks of 32 output dimensions. S = inv_covars (I, D, D) row-major, symmetric (read as S[k][j]).
template <int NJ>
__global__ void __launch_bounds__(FG_THREADS) fg_quad_kernel(const float* __restrict__ x, int D, int64_t ldx, int n, const int* __restrict__ pairs,
                                                              const int* __restrict__ start, const int* __restrict__ istart, int I,
                                                              const float* __restrict__ mic, const float* __restrict__ S,
                                                              const float* __restrict__ gconst, float* __restrict__ ll) {
    constexpr int Dp = NJ * 32;
    extern __shared__ __attribute__((aligned(16))) float fg_lds[];
    const int Dk = (D + 1) & ~1;
    float* Ss = fg_lds;                          // (Dk, Dp): rows >= D and columns >= D zero
    float* ms = Ss + Dk * Dp;                    // (Dp): means_invcovars_g, zero beyond D
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
    float* Xs = ms + Dp + wv * Dp * FG_XLD;      // this wave's (Dp, 32) tile of x^T, row stride FG_XLD
    const BucketItem it = bucket_item(blockIdx.x, start, istart, I, FG_ROWS);
    if (it.g < 0) return;
    const int g = it.g, r0 = it.r0, r1 = it.r1;
    const float* Sg = S + (int64_t)g * D * D;
    for (int e = tid; e < Dk * Dp; e += FG_THREADS) {
        const int k = e / Dp, j = e - k * Dp;
        Ss[e] = (k < D && j < D) ? Sg[k * D + j] : 0.f;
    }
    for (int j = tid; j < Dp; j += FG_THREADS) ms[j] = j < D ? mic[(int64_t)g * D + j] : 0.f;
    const float gc = gconst[g];
    __syncthreads();
    for (int base = r0 + wv * 32; base < r1; base += FG_WAVES * 32) {
        const int pid = base + r < r1 ? pairs[base + r] : -1;
        const int t = pid >= 0 ? pid / n : -1;
        // gather: row rr of the tile = frame t of lane rr, one coalesced load per row, written transposed
        for (int d0 = 0; d0 < Dp; d0 += 64) {
            const int d = d0 + lane;
            float v[32];
#pragma unroll
            for (int rr = 0; rr < 32; ++rr) {
                const int tr = __builtin_amdgcn_readlane(t, rr);
                v[rr] = (tr >= 0 && d < D) ? x[(int64_t)tr * ldx + d] : 0.f;
            }
            if (d < Dp) {
#pragma unroll
                for (int rr = 0; rr < 32; ++rr) Xs[d * FG_XLD + rr] = v[rr];
            }
        }
        wave_lds_sync();
        f32x16 acc[NJ];
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[jb][q] = 0.f;
        for (int k = h; k < Dk; k += 2) {
            const float b = Xs[k * FG_XLD + r];
#pragma unroll
            for (int jb = 0; jb < NJ; ++jb) acc[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ss[k * Dp + jb * 32 + r], b, acc[jb], 0, 0, 0);
        }
        // lane (r, h) holds y_j of frame r for j = jb * 32 + 8 (q / 4) + 4 h + q % 4
        float part = 0.f;
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int j = jb * 32 + 8 * (q >> 2) + 4 * h + (q & 3);
                part = fmaf(Xs[j * FG_XLD + r], fmaf(-0.5f, acc[jb][q], ms[j]), part);
            }
        const float tot = part + __shfl_xor(part, 32, 64);
        if (h == 0 && pid >= 0) ll[pid] = gc + tot;
        wave_lds_sync();
    }
}

// (value, Gaussian, slot) a ranks before b: larger value, then the lower Gaussian, then the lower slot
__device__ __forceinline__ bool fg_before(float va, int ga, int sa, float vb, int gb, int sb) {
    return va > vb || (va == vb && (ga < gb || (ga == gb && sa < sb)));
}

__global__ void __launch_bounds__(FG_THREADS) fg_softmax_kernel(const int* __restrict__ gsel, const float* __restrict__ ll, int64_t F, int n, int I,
                                                                 float min_post, int* __restrict__ gauss, float* __restrict__ post,
                                                                 float* __restrict__ loglike) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * FG_WAVES + (threadIdx.x >> 6);
    if (t >= F) return;
    int g = -1;
    float l = -INFINITY;
    if (lane < n) {
        g = gsel[t * n + lane];
        if (g >= 0 && g < I) l = ll[t * n + lane];
        else g = -1;
    }
    float bv = l;
    int bg = g >= 0 ? g : 0x7fffffff, bs = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int og = __shfl_xor(bg, o, 64), os = __shfl_xor(bs, o, 64);
        if (fg_before(ov, og, os, bv, bg, bs)) {
            bv = ov;
            bg = og;
            bs = os;
        }
    }
    // a frame whose listed log-likelihoods are all -inf (zero-weight components) has no arg-max: it counts as an empty list
    const bool valid = g >= 0 && bv > -INFINITY;
    float p = valid ? expf(l - bv) : 0.f;
    const float tot = wave_sum(p);
    p = p / tot;                                 // no valid slot: 0 / 0, never kept (valid is false)
    if (loglike && lane == 0) loglike[t] = bv > -INFINITY ? bv + logf(tot) : 0.f;   // before pruning; an empty list: 0
    if (min_post != 0.f) {
        if (p < min_post) p = 0.f;
        const float s2 = wave_sum(valid ? p : 0.f);
        p = s2 == 0.f ? (lane == bs ? 1.f : 0.f) : p / s2;
    }
    const bool keep = valid && p != 0.f;
    const int cnt = __popcll(__ballot(keep));
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        const float pj = __shfl(p, j, 64);
        const int gj = __shfl(g, j, 64);
        const int kj = __shfl((int)keep, j, 64);
        rank += (kj && fg_before(pj, gj, j, p, g, lane)) ? 1 : 0;
    }
    if (keep) {
        gauss[t * n + rank] = g;
        post[t * n + rank] = p;
    }
    if (lane < n && lane >= cnt) {
        gauss[t * n + lane] = -1;
        post[t * n + lane] = 0.f;
    }
}

__global__ void __launch_bounds__(256) adddeltas_kernel(const float* __restrict__ x, int64_t T, int D, int64_t sb, int64_t st,
                                                         const int* __restrict__ lengths, const float* __restrict__ coeffs, int order, int window,
                                                         int64_t total, float* __restrict__ out) {
#pragma clang fp contract(off)          // one rounding per multiply and per add: __fmul_rn / __fadd_rn inline as contractable ops
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int C = D * (order + 1);
    const int c = (int)(e % C);
    const int64_t bt = e / C, b = bt / T, t = bt - b * T;
    int64_t len = lengths ? lengths[b] : T;
    len = len < 0 ? 0 : (len > T ? T : len);
    if (t >= len) {
        out[e] = 0.f;
        return;
    }
    const int i = c / D, d = c - i * D, ow = order * window, W = 2 * ow + 1;
    const float* xb = x + b * sb + d;
    float acc = 0.f;
    for (int j = -i * window; j <= i * window; ++j) {
        const float s = coeffs[i * W + ow + j];
        if (s == 0.f) continue;
        int64_t u = t + j;
        u = u < 0 ? 0 : (u > len - 1 ? len - 1 : u);
        const float prod = s * xb[u * st];
        acc = acc + prod;
    }
    out[e] = acc;
}

template <int NJ>
void fg_launch_quad(int items, size_t lds, hipStream_t st, const float* x, int D, int64_t ldx, int n, const int* pairs, const int* start,
                    const int* istart, int I, const float* mic, const float* S, const float* gconst, float* ll) {
    KTF_LDS_ONCE(fg_quad_lds(NJ * 32), fg_quad_kernel<NJ>);
    hipLaunchKernelGGL(fg_quad_kernel<NJ>, dim3(items), dim3(FG_THREADS), lds, st, x, D, ldx, n, pairs, start, istart, I, mic, S, gconst, ll);
}

}  // namespace

extern "C" int64_t ktf_fgmm_workspace_bytes(int64_t F, int32_t I, int32_t D, int32_t n) {
    const int rc = bucket_check_shape("ktf_fgmm_workspace_bytes", F, I, D, n);
    if (rc != KTF_OK) return rc;
    return fg_layout(F, I, n).total;
}

static int fg_post(const char* who, const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* gselect, int32_t n,
                   const float* means_invcovars, const float* inv_covars, const float* gconst, int32_t I, float min_post, int32_t* gauss,
                   float* post, float* loglike, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = bucket_check_shape(who, F, I, D, n);
    if (rc != KTF_OK) return rc;
    KTF_REQUIRE(ldx >= D, "%s: ldx %lld < D %d", who, (long long)ldx, (int)D);
    KTF_REQUIRE(min_post >= 0.f && min_post < 1.f, "%s: min_post %g outside [0, 1)", who, (double)min_post);
    if (F == 0) return KTF_OK;
    KTF_REQUIRE(x && gselect && means_invcovars && inv_covars && gconst && gauss && post && workspace, "%s: null argument", who);
    const FgLayout l = fg_layout(F, I, n);
    if (ktf_check_workspace(who, workspace, workspace_bytes, l.total) != KTF_OK) return KTF_EINVAL;
    char* ws = (char*)workspace;
    const int* start = (const int*)(ws + l.sec.start);
    const int* pairs = (const int*)(ws + l.sec.pairs);
    int* istart = (int*)(ws + l.istart);
    float* ll = (float*)(ws + l.ll);
    hipStream_t st = (hipStream_t)stream;
    const int64_t P = F * n;
    if ((rc = sec_bucket(who, gselect, P, (int)I, l.sec, ws, st)) != KTF_OK) return rc;
    if ((rc = bucket_items(who, start, (int)I, FG_ROWS, istart, nullptr, st)) != KTF_OK) return rc;
    const int items = (int)((P + FG_ROWS - 1) / FG_ROWS) + I;       // an upper bound of istart[I]; the rest exit at once
    const size_t lds = fg_quad_lds(D);
    switch (fg_dp(D) / 32) {
        case 1: fg_launch_quad<1>(items, lds, st, x, D, ldx, n, pairs, start, istart, I, means_invcovars, inv_covars, gconst, ll); break;
        case 2: fg_launch_quad<2>(items, lds, st, x, D, ldx, n, pairs, start, istart, I, means_invcovars, inv_covars, gconst, ll); break;
        case 3: fg_launch_quad<3>(items, lds, st, x, D, ldx, n, pairs, start, istart, I, means_invcovars, inv_covars, gconst, ll); break;
        default: fg_launch_quad<4>(items, lds, st, x, D, ldx, n, pairs, start, istart, I, means_invcovars, inv_covars, gconst, ll); break;
    }
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(fg_softmax_kernel, dim3((unsigned)((F + FG_WAVES - 1) / FG_WAVES)), dim3(FG_THREADS), 0, st, gselect, (const float*)ll, F,
                       (int)n, (int)I, min_post, gauss, post, loglike);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_add_deltas_f32(const float* x, int64_t B, int64_t T, int32_t D, int64_t stride_b, int64_t stride_t, const int32_t* lengths,
                                  const float* coeffs, int32_t order, int32_t window, float* out, void* stream) {
    const char* who = "ktf_add_deltas_f32";
    KTF_REQUIRE(order >= 0 && window >= 1 && (int64_t)order * window <= KTF_ADD_DELTAS_MAX_CONTEXT,
                "%s: order %d, window %d: need order >= 0, window >= 1, order * window <= %d", who, (int)order, (int)window,
                KTF_ADD_DELTAS_MAX_CONTEXT);
    KTF_REQUIRE(D >= 1 && D <= 65536, "%s: feature dim %d outside 1 .. 65536", who, (int)D);
    KTF_REQUIRE(B >= 0 && T >= 0, "%s: negative shape (%lld, %lld)", who, (long long)B, (long long)T);
    KTF_REQUIRE(stride_t >= D && stride_b >= 0, "%s: strides (%lld, %lld) for D %d", who, (long long)stride_b, (long long)stride_t, (int)D);
    const int64_t rows = B * T;
    KTF_REQUIRE(B == 0 || T == 0 || rows / T == B, "%s: B * T overflows", who);
    KTF_REQUIRE(rows <= ((int64_t)1 << 38) / ((int64_t)D * (order + 1)), "%s: output of %lld rows too large", who, (long long)rows);
    if (rows == 0) return KTF_OK;
    KTF_REQUIRE(x && coeffs && out, "%s: null argument", who);
    const int64_t total = rows * D * (order + 1);
    hipLaunchKernelGGL(adddeltas_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, T, (int)D, stride_b, stride_t,
                       lengths, coeffs, (int)order, (int)window, total, out);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_fgmm_post_f32(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* gselect, int32_t n,
                                 const float* means_invcovars, const float* inv_covars, const float* gconst, int32_t I, float min_post,
                                 int32_t* gauss, float* post, void* workspace, size_t workspace_bytes, void* stream) {
    return fg_post("ktf_fgmm_post_f32", x, F, D, ldx, gselect, n, means_invcovars, inv_covars, gconst, I, min_post, gauss, post, nullptr,
                   workspace, workspace_bytes, stream);
}

extern "C" int ktf_fgmm_post_ll_f32(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* gselect, int32_t n,
                                    const float* means_invcovars, const float* inv_covars, const float* gconst, int32_t I, float min_post,
                                    int32_t* gauss, float* post, float* loglike, void* workspace, size_t workspace_bytes, void* stream) {
    return fg_post("ktf_fgmm_post_ll_f32", x, F, D, ldx, gselect, n, means_invcovars, inv_covars, gconst, I, min_post, gauss, post, loglike,
                   workspace, workspace_bytes, stream);
}
