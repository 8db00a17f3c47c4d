// VBx: the VB-HMM of Landini / Diez / Burget over window x-vectors in the PLDA-transformed space (within-class covariance I,
// between-class covariance diag(phi)), batched over the recordings of one call. Windows of all recordings lie end to end: recording
// r owns rows [offsets[r], offsets[r + 1]) of x / rho / gamma / lls. The forward-backward and the bound are vb_fb.hip's.
//
//   vbx_prepare_kernel   one wave per window: rho = x sqrt(phi), G = -(sum x^2 + D log 2 pi) / 2 (lane-strided, then a butterfly).
//   vbx_acc_kernel       gamma^T [rho | 1] on v_mfma_f64_16x16x4_f64: one workgroup per chunk of VBX_UROWS windows of a recording
//                        (chunks count from the recording's first window), one wave per 16 columns; speakers padded to 16, the
//                        column D carries N_k. A chunk's 16 x (D + 1) block goes to the workspace.
//   vbx_finish_kernel    one workgroup per recording adds the chunks' blocks in chunk order, then invL, alpha and, 16 lanes per
//                        speaker (lane j takes d = j, j + 16, ...; then a butterfly), c and kl.
//   vbx_lls_kernel       one wave per 16 packed windows x 16 speakers, the contraction over D four per MFMA in ascending d. A tile
//                        that spans recordings runs once per recording with the other rows zeroed: an element's bits depend on
//                        its own row and its recording's alpha alone.
#include "vb_common.h"
#include "f64_mfma.h"

namespace {

constexpr int UROWS = KTF_VBX_UPDATE_ROWS;
constexpr int UWAVES = 4;           // waves (16-column tiles) per workgroup of vbx_acc_kernel

__device__ __forceinline__ double group16_sum(double v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(256) vbx_prepare_kernel(const double* __restrict__ x, int64_t TB, int D, const double* __restrict__ phi,
                                                          double* __restrict__ rho, double* __restrict__ G) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= TB) return;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = x[t * D + d];
        rho[t * D + d] = v * sqrt(phi[d]);
        s = fma(v, v, s);
    }
    s = wave_sum_d(s);
    if (lane == 0) G[t] = -0.5 * (s + (double)D * 1.8378770664093454835606594728112);      // log 2 pi
}

// cstart[r] = the chunks of the recordings before r (one thread: N is small next to the windows)
__global__ void vbx_cstart_kernel(const int* __restrict__ off, int N, int* __restrict__ cstart) {
    if (blockIdx.x || threadIdx.x) return;
    int run = 0;
    for (int r = 0; r < N; ++r) {
        cstart[r] = run;
        const int T = off[r + 1] - off[r];
        run += T > 0 ? (T + UROWS - 1) / UROWS : 0;
    }
    cstart[N] = run;
}

// part[w][k][col] (16 x ldp per chunk w): sum over the chunk's windows t, ascending and four per MFMA, of gamma_tk [rho_t | 1]_col
__global__ void __launch_bounds__(64 * UWAVES) vbx_acc_kernel(const double* __restrict__ gamma, const double* __restrict__ rho, int64_t TB,
                                                              int D, int K, const int* __restrict__ off, const int* __restrict__ cstart,
                                                              int N, int ldp, double* __restrict__ part) {
    const int w = blockIdx.x, lane = threadIdx.x & 63;
    const int col0 = (blockIdx.y * UWAVES + (threadIdx.x >> 6)) * 16;
    if (col0 > D) return;
    const int r = vb_owner(cstart, N, w);
    if (r < 0) return;
    const int64_t base = off[r];
    const int64_t T = (int64_t)off[r + 1] - base;
    if (base < 0 || base + T > TB) return;       // an inconsistent table reads nothing out of range
    const int64_t r0 = (int64_t)(w - cstart[r]) * UROWS;
    const int rows = (int)(T - r0 < UROWS ? T - r0 : UROWS);
    const int lc = lane & 15, lk = lane >> 4, col = col0 + lc;
    const double* g = gamma + (base + r0) * K;
    const double* p = rho + (base + r0) * D;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < rows; k0 += 16) {      // four MFMAs' operands in flight; a step past the chunk's end adds 0 * 0
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = k0 + 4 * u + lk;
            const bool in = t < rows;
            a[u] = (in && lc < K) ? g[(int64_t)t * K + lc] : 0.0;
            b[u] = in ? (col < D ? p[(int64_t)t * D + col] : (col == D ? 1.0 : 0.0)) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
    double* o = part + (int64_t)w * FBK * ldp;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[(int64_t)(lk + 4 * i) * ldp + col] = acc[i];
}

__global__ void __launch_bounds__(256) vbx_finish_kernel(const double* __restrict__ part, const int* __restrict__ cstart, int64_t maxch, int ldp,
                                                         int D, int K, const double* __restrict__ phi, double fafb,
                                                         double* __restrict__ alpha, double* __restrict__ invL, double* __restrict__ c,
                                                         double* __restrict__ kl) {
    const int r = blockIdx.x, k = threadIdx.x >> 4, j = threadIdx.x & 15;
    const int w0 = cstart[r];
    const int nch = (w0 >= 0 && cstart[r + 1] >= w0 && cstart[r + 1] <= maxch) ? cstart[r + 1] - w0 : 0;
    const bool on = k < K;
    if (nch == 0) {                              // no windows: alpha and invL stay as they are
        if (on && j == 0) c[(int64_t)r * K + k] = kl[(int64_t)r * K + k] = 0.0;
        return;
    }
    const double* p = part + ((int64_t)w0 * FBK + k) * ldp;
    const int64_t cs = (int64_t)FBK * ldp;
    double Nk = 0.0;
    for (int ch = 0; ch < nch; ++ch) Nk += p[ch * cs + D];
    double cacc = 0.0, kacc = 0.0;
    if (on)
        for (int d = j; d < D; d += 16) {
            double s = 0.0;
            for (int ch = 0; ch < nch; ++ch) s += p[ch * cs + d];
            const double ph = phi[d];
            const double il = 1.0 / (1.0 + fafb * Nk * ph);
            const double a = fafb * il * s;
            alpha[((int64_t)r * K + k) * D + d] = a;
            invL[((int64_t)r * K + k) * D + d] = il;
            cacc += (il + a * a) * ph;
            kacc += log(il) - il - a * a + 1.0;
        }
    cacc = group16_sum(cacc);
    kacc = group16_sum(kacc);
    if (on && j == 0) {
        c[(int64_t)r * K + k] = 0.5 * cacc;
        kl[(int64_t)r * K + k] = 0.5 * kacc;
    }
}

__global__ void __launch_bounds__(256) vbx_lls_kernel(const double* __restrict__ rho, const double* __restrict__ G, int64_t TB, int D, int K,
                                                      const int* __restrict__ off, int N, const double* __restrict__ alpha,
                                                      const double* __restrict__ c, double Fa, double* __restrict__ lls) {
    const int lane = threadIdx.x & 63, lc = lane & 15, lk = lane >> 4;
    const int64_t t0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    if (t0 >= TB) return;
    const int64_t tend = t0 + 16 < TB ? t0 + 16 : TB;
    int64_t t = t0;
    while (t < tend) {
        const int r = vb_owner(off, N, t);
        if (r < 0) {                             // rows in front of the first recording belong to nobody
            if (t >= off[0]) break;
            t = off[0];
            continue;
        }
        const int64_t e = off[r + 1] < tend ? off[r + 1] : tend;
        const int64_t row = t0 + lc;             // this lane's row of the A operand
        const bool mine = row >= t && row < e;
        const double* pa = rho + row * D;
        const double* pb = alpha + ((int64_t)r * K + (lc < K ? lc : 0)) * D;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int d0 = 0; d0 < D; d0 += 16) {     // four MFMAs' operands in flight; a step past D adds 0 * 0
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int d = d0 + 4 * u + lk;
                a[u] = (mine && d < D) ? pa[d] : 0.0;
                b[u] = (lc < K && d < D) ? pb[d] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
        }
        if (lc < K) {
            const double ck = c[(int64_t)r * K + lc];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t ro = t0 + lk + 4 * i;
                if (ro >= t && ro < e) lls[ro * K + lc] = Fa * (acc[i] - ck + G[ro]);
            }
        }
        t = e;
    }
}

int vbx_check(const char* who, int64_t TB, int32_t D, int32_t N, int32_t K) {
    KTF_REQUIRE(TB >= 0 && TB < ((int64_t)1 << 31), "%s: window count %lld out of range", who, (long long)TB);
    KTF_REQUIRE(D >= 1 && D <= KTF_VBX_MAX_DIM, "%s: dim %d outside 1 .. %d", who, (int)D, KTF_VBX_MAX_DIM);
    KTF_REQUIRE(N >= 1 && N <= 65535, "%s: %d recordings outside 1 .. 65535", who, (int)N);
    KTF_REQUIRE(K >= 1 && K <= KTF_VB_MAX_SPEAKERS, "%s: %d speakers outside 1 .. %d", who, (int)K, KTF_VB_MAX_SPEAKERS);
    return KTF_OK;
}

struct UpLayout {
    int64_t cstart, part, total, maxch;
    int ldp;
};

UpLayout up_layout(int64_t TB, int64_t N, int64_t D) {
    UpLayout l;
    l.maxch = TB / UROWS + N;                    // every recording adds at most one partial chunk
    l.ldp = (int)((D + 1 + 15) / 16 * 16);
    int64_t at = 0;
    l.cstart = at; at += al256((N + 1) * 4);
    l.part = at;   at += al256(l.maxch * FBK * l.ldp * 8);
    l.total = at;
    return l;
}

}  // namespace

extern "C" int ktf_vbx_prepare(const double* x, int64_t TB, int32_t D, const double* phi, double* rho, double* G, void* stream) {
    const char* who = "ktf_vbx_prepare";
    int rc = vbx_check(who, TB, D, 1, 1);
    if (rc != KTF_OK) return rc;
    KTF_REQUIRE(phi && (TB == 0 || (x && rho && G)), "%s: null argument", who);
    if (TB == 0) return KTF_OK;
    hipLaunchKernelGGL(vbx_prepare_kernel, dim3((unsigned)((TB + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, TB, (int)D, phi, rho, G);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int64_t ktf_vbx_update_workspace_bytes(int64_t TB, int32_t N, int32_t D) {
    const char* who = "ktf_vbx_update_workspace_bytes";
    int rc = vbx_check(who, TB, D, N, 1);
    if (rc != KTF_OK) return rc;
    return up_layout(TB, N, D).total;
}

extern "C" int ktf_vbx_speaker_update(const double* gamma, const double* rho, int64_t TB, int32_t D, int32_t K, const int32_t* offsets, int32_t N,
                                      const double* phi, double fa_over_fb, double* alpha, double* invL, double* c, double* kl,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "ktf_vbx_speaker_update";
    int rc = vbx_check(who, TB, D, N, K);
    if (rc != KTF_OK) return rc;
    KTF_REQUIRE(fa_over_fb > 0.0 && fa_over_fb < INFINITY, "%s: Fa / Fb %g not positive and finite", who, fa_over_fb);
    KTF_REQUIRE(offsets && phi && alpha && invL && c && kl && workspace, "%s: null argument", who);
    KTF_REQUIRE(TB == 0 || (gamma && rho), "%s: null gamma / rho", who);
    const UpLayout l = up_layout(TB, N, D);
    if (ktf_check_workspace(who, workspace, workspace_bytes, l.total) != KTF_OK) return KTF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int* cstart = (int*)(ws + l.cstart);
    double* part = (double*)(ws + l.part);
    hipLaunchKernelGGL(vbx_cstart_kernel, dim3(1), dim3(64), 0, st, offsets, (int)N, cstart);
    KTF_CHECK_LAUNCH(who);
    if (TB > 0) {
        hipLaunchKernelGGL(vbx_acc_kernel, dim3((unsigned)l.maxch, ktf_cdiv(l.ldp / 16, UWAVES)), dim3(64 * UWAVES), 0, st, gamma, rho, TB, (int)D,
                           (int)K, offsets, (const int*)cstart, (int)N, l.ldp, part);
        KTF_CHECK_LAUNCH(who);
    }
    hipLaunchKernelGGL(vbx_finish_kernel, dim3(N), dim3(256), 0, st, (const double*)part, (const int*)cstart, l.maxch, l.ldp, (int)D, (int)K, phi,
                       fa_over_fb, alpha, invL, c, kl);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_vbx_loglike(const double* rho, const double* G, int64_t TB, int32_t D, int32_t K, const int32_t* offsets, int32_t N,
                               const double* alpha, const double* c, double Fa, double* lls, void* stream) {
    const char* who = "ktf_vbx_loglike";
    int rc = vbx_check(who, TB, D, N, K);
    if (rc != KTF_OK) return rc;
    KTF_REQUIRE(Fa > 0.0 && Fa < INFINITY, "%s: Fa %g not positive and finite", who, Fa);
    KTF_REQUIRE(offsets && alpha && c, "%s: null argument", who);
    KTF_REQUIRE(TB == 0 || (rho && G && lls), "%s: null rho / G / lls", who);
    if (TB == 0) return KTF_OK;
    hipLaunchKernelGGL(vbx_lls_kernel, dim3((unsigned)((TB + 63) / 64)), dim3(256), 0, (hipStream_t)stream, rho, G, TB, (int)D, (int)K, offsets,
                       (int)N, alpha, c, Fa, lls);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
