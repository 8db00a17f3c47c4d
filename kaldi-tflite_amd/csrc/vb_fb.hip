// VB-HMM resegmentation (vb_common.h): forward-backward over a recording's blocks, and the bound.
//
//   fb_*              forward-backward as a chunked scan, KTF_VB_FB_CHUNK blocks per chunk. fb_matrix_kernel: one wave per
//                     chunk, lane j carries column j of the chunk's K x K transfer matrix through the chunk's steps (a step is
//                     diagonal plus rank one: O(K)), renormalised every step with a running log-scale. fb_carry_kernel: one wave
//                     per recording takes the forward vector through the chunks' matrices and the backward vector through their
//                     transposes. fb_post_kernel: one wave per chunk recomputes its alpha and beta in LDS and writes q and the
//                     chunk's share of the sp sums; fb_sp_kernel adds the shares in chunk order.
#include "vb_common.h"
#include "ivector_stages.h"

namespace {

struct FbLayout {
    int64_t cstart, M, sc, ain, bout, spc, total;
    int64_t maxch;
};

FbLayout fb_layout(int64_t TB, int64_t N) {
    FbLayout l;
    l.maxch = TB / FBC + N;                      // every recording adds at most one partial chunk
    int64_t at = 0;
    l.cstart = at; at += al256((N + 1) * 4);
    l.M = at;      at += al256(l.maxch * FBK * FBK * 8);
    l.sc = at;     at += al256(l.maxch * FBK * 8);
    l.ain = at;    at += al256(l.maxch * FBK * 8);
    l.bout = at;   at += al256(l.maxch * FBK * 8);
    l.spc = at;    at += al256(l.maxch * FBK * 8);
    l.total = at;
    return l;
}

// cstart[r] = the chunks of the recordings before r (one thread: N is small next to the frames)
__global__ void fb_cstart_kernel(const int* __restrict__ boff, int N, int* __restrict__ cstart) {
    if (blockIdx.x || threadIdx.x) return;
    int run = 0;
    for (int r = 0; r < N; ++r) {
        cstart[r] = run;
        const int tb = boff[r + 1] - boff[r];
        run += tb > 0 ? (tb + FBC - 1) / FBC : 0;
    }
    cstart[N] = run;
}

struct FbChunk {
    int r, k, b0, b1;               // recording, chunk within it, its blocks [b0, b1) within the recording
    int64_t base;                   // the recording's first block
};

__device__ __forceinline__ FbChunk fb_chunk(int w, const int* __restrict__ boff, const int* __restrict__ cstart, int N, int64_t TB) {
    FbChunk c;
    c.r = vb_owner(cstart, N, w);
    c.k = c.b0 = c.b1 = 0;
    c.base = 0;
    if (c.r < 0) return c;
    c.k = w - cstart[c.r];
    c.base = boff[c.r];
    int64_t tb = (int64_t)boff[c.r + 1] - c.base;
    if (c.base < 0 || c.base + tb > TB) {        // an inconsistent table reads nothing out of range
        c.r = -1;
        return c;
    }
    c.b0 = c.k * FBC;
    c.b1 = c.b0 + FBC < tb ? c.b0 + FBC : (int)tb;
    return c;
}

// e[b][i] = exp(lls - the row's max) and mxs[b] = that max for the chunk's blocks, 64 lanes over the blocks
__device__ __forceinline__ void fb_load_e(double (*e)[FBK], double* mxs, const double* __restrict__ lls, const FbChunk& c, int K, int lane) {
    for (int b = c.b0 + lane; b < c.b1; b += 64) {
        const double* row = lls + (c.base + b) * K;
        double mx = row[0];
        for (int i = 1; i < K; ++i) mx = fmax(mx, row[i]);
        for (int i = 0; i < K; ++i) e[b - c.b0][i] = exp(row[i] - mx);
        mxs[b - c.b0] = mx;
    }
}

// one step of the scaled forward recursion on v (K entries): v_i <- e_i (lp v_i + (1 - lp) sp_i sum v); -> (sum before, sum after)
__device__ __forceinline__ void fb_step(double (&v)[FBK], const double* __restrict__ e, const double (&sp)[FBK], int K, double lp, double* s_in,
                                        double* s_out) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < FBK; ++i)
        if (i < K) s += v[i];
    const double t = (1.0 - lp) * s;
    double s2 = 0.0;
#pragma unroll
    for (int i = 0; i < FBK; ++i)
        if (i < K) {
            v[i] = e[i] * (lp * v[i] + t * sp[i]);
            s2 += v[i];
        }
    *s_in = s;
    *s_out = s2;
}

// the sum of lanes 0 .. K - 1 in lane order, the same bits in every lane (all 64 lanes call)
__device__ __forceinline__ double fb_lanes_sum(double v, int K) {
    double s = 0.0;
    for (int j = 0; j < K; ++j) s += __shfl(v, j, 64);
    return s;
}
__device__ __forceinline__ double fb_lanes_max(double v, int K) {
    double m = -INFINITY;
    for (int j = 0; j < K; ++j) m = fmax(m, __shfl(v, j, 64));
    return m;
}

// Mws[w][j][i] = column j of the product of the chunk's steps (blocks max(b0, 1) .. b1 - 1), scaled to sum 1; sc[w][j] = its log-scale
__global__ void __launch_bounds__(64) fb_matrix_kernel(const double* __restrict__ lls, const int* __restrict__ boff, const int* __restrict__ cstart,
                                                       int N, int64_t TB, int K, const double* __restrict__ sp_in, double lp,
                                                       double* __restrict__ Mws, double* __restrict__ sc) {
    __shared__ double e[FBC][FBK];
    __shared__ double mxs[FBC];
    const int w = blockIdx.x, lane = threadIdx.x;
    const FbChunk c = fb_chunk(w, boff, cstart, N, TB);
    if (c.r < 0) return;
    fb_load_e(e, mxs, lls, c, K, lane);
    __syncthreads();
    if (lane >= K) return;
    double v[FBK], sp[FBK];
#pragma unroll
    for (int i = 0; i < FBK; ++i) {
        v[i] = i == lane ? 1.0 : 0.0;
        sp[i] = i < K ? sp_in[(int64_t)c.r * K + i] : 0.0;
    }
    double ls = 0.0;
    for (int b = c.b0 > 1 ? c.b0 : 1; b < c.b1; ++b) {
        double s, s2;
        fb_step(v, e[b - c.b0], sp, K, lp, &s, &s2);
        const double inv = s2 > 0.0 ? 1.0 / s2 : 0.0;
#pragma unroll
        for (int i = 0; i < FBK; ++i) v[i] *= inv;
        ls += (s2 > 0.0 ? log(s2) : -INFINITY) + mxs[b - c.b0];
    }
    double* m = Mws + ((int64_t)w * FBK + lane) * FBK;
#pragma unroll
    for (int i = 0; i < FBK; ++i) m[i] = v[i];
    sc[(int64_t)w * FBK + lane] = ls;
}

// one wave per recording, lane i = speaker i: ain[w] = the scaled alpha entering chunk w (for a recording's first chunk: alpha of
// block 0), bout[w] = the scaled beta of chunk w's last block, tll = log p(blocks)
__global__ void __launch_bounds__(64) fb_carry_kernel(const double* __restrict__ lls, const int* __restrict__ boff, const int* __restrict__ cstart,
                                                      int N, int64_t TB, int64_t maxch, int K, const double* __restrict__ sp_in,
                                                      const double* __restrict__ Mws, const double* __restrict__ sc, double* __restrict__ ain,
                                                      double* __restrict__ bout, double* __restrict__ tll) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const bool on = lane < K;
    const int64_t base = boff[r];
    const int64_t tb = (int64_t)boff[r + 1] - base;
    const int w0 = cstart[r], nch = cstart[r + 1] - w0;
    if (tb <= 0 || base < 0 || base + tb > TB || w0 + nch > maxch) {      // an inconsistent table touches nothing
        if (lane == 0) tll[r] = 0.0;
        return;
    }
    const double* row0 = lls + base * K;
    const double mx0 = fb_lanes_max(on ? row0[lane] : -INFINITY, K);
    double a = on ? sp_in[(int64_t)r * K + lane] * exp(row0[lane] - mx0) : 0.0;
    double s = fb_lanes_sum(a, K);
    a = s > 0.0 ? a / s : 0.0;
    double la = log(s) + mx0;
    for (int k = 0; k < nch; ++k) {
        const int64_t w = w0 + k;
        if (on) ain[w * FBK + lane] = a;
        const double sj = on ? sc[w * FBK + lane] : -INFINITY;
        const double smax = fb_lanes_max(sj, K);
        const double wt = (on && sj > -INFINITY) ? exp(sj - smax) * a : 0.0;
        double o = 0.0;
        for (int j = 0; j < K; ++j) {
            const double wj = __shfl(wt, j, 64);
            if (on) o = fma(Mws[(w * FBK + j) * FBK + lane], wj, o);
        }
        s = fb_lanes_sum(o, K);
        a = s > 0.0 ? o / s : 0.0;
        la += smax + log(s);
    }
    if (lane == 0) tll[r] = la;
    double bt = on ? 1.0 : 0.0;
    for (int k = nch - 1; k >= 0; --k) {
        const int64_t w = w0 + k;
        if (on) bout[w * FBK + lane] = bt;
        if (k == 0) break;
        double dot = 0.0;                        // lane j: column j of the chunk's matrix against beta
        for (int i = 0; i < K; ++i) {
            const double bi = __shfl(bt, i, 64);
            if (on) dot = fma(Mws[(w * FBK + lane) * FBK + i], bi, dot);
        }
        const double sj = on ? sc[w * FBK + lane] : -INFINITY;
        const double smax = fb_lanes_max(sj, K);
        const double o = (on && sj > -INFINITY) ? exp(sj - smax) * dot : 0.0;
        s = fb_lanes_sum(o, K);
        bt = s > 0.0 ? o / s : 0.0;
    }
}

// one wave per chunk: alpha forwards from ain and beta backwards from bout, both in LDS; then q and the chunk's share of the sp sums
__global__ void __launch_bounds__(64) fb_post_kernel(const double* __restrict__ lls, const int* __restrict__ boff, const int* __restrict__ cstart,
                                                     int N, int64_t TB, int K, const double* __restrict__ sp_in, double lp,
                                                     const double* __restrict__ ain, const double* __restrict__ bout, double* __restrict__ q,
                                                     double* __restrict__ spc) {
    __shared__ double e[FBC][FBK];               // exp(lls - max); after the backward walk e . beta
    __shared__ double ah[FBC][FBK];              // scaled alpha; after the backward walk alpha . beta
    __shared__ double cb[FBC];                   // (1 - lp) sum(alpha_{b-1}) / the step's normaliser; mxs while e is built
    __shared__ double tot[FBC];
    const int w = blockIdx.x, lane = threadIdx.x;
    const FbChunk c = fb_chunk(w, boff, cstart, N, TB);
    if (c.r < 0) return;
    fb_load_e(e, cb, lls, c, K, lane);
    __syncthreads();
    double v[FBK], sp[FBK];
#pragma unroll
    for (int i = 0; i < FBK; ++i) {
        v[i] = i < K ? ain[(int64_t)w * FBK + i] : 0.0;
        sp[i] = i < K ? sp_in[(int64_t)c.r * K + i] : 0.0;
    }
    const int nb = c.b1 - c.b0;
    const int s0 = c.b0 > 1 ? c.b0 : 1;
    // every lane walks the same recursion; lane 0 keeps the rows
    if (c.b0 == 0 && lane == 0) {
#pragma unroll
        for (int i = 0; i < FBK; ++i) ah[0][i] = v[i];
        cb[0] = 0.0;
    }
    for (int b = s0; b < c.b1; ++b) {
        double s, s2;
        fb_step(v, e[b - c.b0], sp, K, lp, &s, &s2);
        const double inv = s2 > 0.0 ? 1.0 / s2 : 0.0;
#pragma unroll
        for (int i = 0; i < FBK; ++i) v[i] *= inv;
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < FBK; ++i) ah[b - c.b0][i] = v[i];
            cb[b - c.b0] = (1.0 - lp) * s * inv;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < FBK; ++i) v[i] = i < K ? bout[(int64_t)w * FBK + i] : 0.0;
    for (int b = c.b1 - 1; b >= c.b0; --b) {
        double eb[FBK];
        double dot = 0.0, at = 0.0;
#pragma unroll
        for (int i = 0; i < FBK; ++i) {
            eb[i] = i < K ? e[b - c.b0][i] * v[i] : 0.0;
            dot = fma(sp[i], eb[i], dot);
            at += i < K ? ah[b - c.b0][i] * v[i] : 0.0;
        }
        __syncthreads();                         // every lane has read row b before lane 0 overwrites it
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < FBK; ++i) {
                ah[b - c.b0][i] *= v[i];
                e[b - c.b0][i] = eb[i];
            }
            tot[b - c.b0] = at;
        }
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < FBK; ++i) {
            v[i] = i < K ? lp * eb[i] + (1.0 - lp) * dot : 0.0;
            s += v[i];
        }
        const double inv = s > 0.0 ? 1.0 / s : 0.0;
#pragma unroll
        for (int i = 0; i < FBK; ++i) v[i] *= inv;
    }
    __syncthreads();
    for (int idx = lane; idx < nb * K; idx += 64) {
        const int b = idx / K, j = idx - b * K;
        q[(c.base + c.b0 + b) * K + j] = ah[b][j] / tot[b];
    }
    if (lane < K) {
        const double spj = sp_in[(int64_t)c.r * K + lane];
        double acc = c.b0 == 0 ? ah[0][lane] / tot[0] : 0.0;
        for (int b = s0; b < c.b1; ++b) acc += cb[b - c.b0] * spj * e[b - c.b0][lane] / tot[b - c.b0];
        spc[(int64_t)w * FBK + lane] = acc;
    }
}

// sp_out (N, K) = the chunks' shares added in chunk order, normalised; a recording without blocks keeps its sp
__global__ void __launch_bounds__(64) fb_sp_kernel(const int* __restrict__ cstart, int64_t maxch, int K, const double* __restrict__ sp_in,
                                                   const double* __restrict__ spc, double* __restrict__ sp_out) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const bool on = lane < K;
    const int w0 = cstart[r], nch = w0 + (cstart[r + 1] - w0) <= maxch ? cstart[r + 1] - w0 : 0;
    double acc = 0.0;
    if (on)
        for (int k = 0; k < nch; ++k) acc += spc[(int64_t)(w0 + k) * FBK + lane];
    const double s = fb_lanes_sum(on ? acc : 0.0, K);
    if (on) sp_out[(int64_t)r * K + lane] = (nch > 0 && s > 0.0) ? acc / s : sp_in[(int64_t)r * K + lane];
}

// the sum / max over the 16 lanes of a speaker group by a butterfly: the same bits in every lane (lanes beyond K hold 0 / -inf)
__device__ __forceinline__ double fb_group_sum(double v) {
#pragma unroll
    for (int o = FBK / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double fb_group_max(double v) {
#pragma unroll
    for (int o = FBK / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// The serial form, for tools/bench_vb.py to time the chunked scan against (not on the product's path): one wave per recording,
// lane i = speaker i, walks all the recording's blocks forwards and then backwards. alpha (TB, FBK) and cb (TB) in the workspace
// hold the scaled forward vectors and (1 - lp) sum(alpha_{b-1}) / the step's normaliser; no LDS staging.
__global__ void __launch_bounds__(64) fb_serial_kernel(const double* __restrict__ lls, const int* __restrict__ boff, int64_t TB, int K,
                                                       const double* __restrict__ sp_in, double lp, double* __restrict__ alpha,
                                                       double* __restrict__ cbw, double* __restrict__ q, double* __restrict__ sp_out,
                                                       double* __restrict__ tll) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const bool on = lane < K;
    const int64_t base = boff[r];
    const int64_t tb = (int64_t)boff[r + 1] - base;
    const double spi = on ? sp_in[(int64_t)r * K + lane] : 0.0;
    if (tb <= 0 || base < 0 || base + tb > TB) {                           // no blocks (or an inconsistent table): sp stays
        if (lane == 0) tll[r] = 0.0;
        if (on) sp_out[(int64_t)r * K + lane] = spi;
        return;
    }
    double l = on ? lls[base * K + lane] : -INFINITY;
    double mx = fb_group_max(l);
    double a = on ? spi * exp(l - mx) : 0.0;
    double s = fb_group_sum(a);
    a = s > 0.0 ? a / s : 0.0;
    double la = log(s) + mx;
    if (lane < FBK) alpha[base * FBK + lane] = a;
    if (lane == 0) cbw[base] = 0.0;
    for (int64_t b = 1; b < tb; ++b) {
        l = on ? lls[(base + b) * K + lane] : -INFINITY;
        mx = fb_group_max(l);
        s = fb_group_sum(a);
        const double v = on ? exp(l - mx) * (lp * a + (1.0 - lp) * s * spi) : 0.0;
        const double s2 = fb_group_sum(v);
        const double inv = s2 > 0.0 ? 1.0 / s2 : 0.0;
        a = v * inv;
        la += (s2 > 0.0 ? log(s2) : -INFINITY) + mx;
        if (lane < FBK) alpha[(base + b) * FBK + lane] = a;
        if (lane == 0) cbw[base + b] = (1.0 - lp) * s * inv;
    }
    if (lane == 0) tll[r] = la;
    __syncthreads();                             // lane 0's cbw are read by every lane below
    double bt = on ? 1.0 : 0.0, acc = 0.0;
    for (int64_t b = tb - 1; b >= 0; --b) {
        l = on ? lls[(base + b) * K + lane] : -INFINITY;
        mx = fb_group_max(l);
        const double eb = on ? exp(l - mx) * bt : 0.0;
        const double ab = on ? alpha[(base + b) * FBK + lane] * bt : 0.0;
        const double at = fb_group_sum(ab);
        const double qv = ab / at;
        if (on) q[(base + b) * K + lane] = qv;
        acc += b == 0 ? qv : cbw[base + b] * spi * eb / at;
        const double dot = fb_group_sum(spi * eb);
        const double o = on ? lp * eb + (1.0 - lp) * dot : 0.0;
        s = fb_group_sum(o);
        bt = s > 0.0 ? o / s : 0.0;
    }
    s = fb_group_sum(on ? acc : 0.0);
    if (on) sp_out[(int64_t)r * K + lane] = s > 0.0 ? acc / s : spi;
}

// ---------------------------------------------------------------- the bound
// gsum[r] = sum_t G_t over recording r's frames in fp64: thread-strided from the recording's first frame, then a fixed tree, so the
// bits depend on the recording's values alone, not on where it lies in the packed vector
__global__ void __launch_bounds__(256) vb_gsum_kernel(const float* __restrict__ loglike, const int* __restrict__ off, int64_t F,
                                                      double* __restrict__ gsum) {
    __shared__ double part[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    int64_t t0, t1;
    utt_rows(off, r, F, &t0, &t1);
    double v = 0.0;
    for (int64_t t = t0 + tid; t < t1; t += 256) v += (double)loglike[t];
    part[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) part[tid] += part[tid + s];
        __syncthreads();
    }
    if (tid == 0) gsum[r] = part[0];
}

// bound[r] = stat_scale gsum[r] + tll[r] + sum_s kl[r K + s], s ascending
__global__ void vb_bound_kernel(const double* __restrict__ gsum, const double* __restrict__ tll, const double* __restrict__ kl, int N, int K,
                                double stat_scale, double* __restrict__ bound) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += kl[(int64_t)r * K + k];
    bound[r] = stat_scale * gsum[r] + tll[r] + s;
}

}  // namespace

extern "C" int64_t ktf_vb_fb_workspace_bytes(int64_t TB, int32_t N) {
    const char* who = "ktf_vb_fb_workspace_bytes";
    KTF_REQUIRE(TB >= 0 && TB < ((int64_t)1 << 31), "%s: block count %lld out of range", who, (long long)TB);
    KTF_REQUIRE(N >= 1 && N <= 65535, "%s: %d recordings outside 1 .. 65535", who, (int)N);
    return fb_layout(TB, N).total;
}

extern "C" int ktf_vb_forward_backward(const double* lls, const int32_t* boffsets, int32_t N, int64_t TB, int32_t K, const double* sp,
                                       double loop_prob, double* q, double* sp_out, double* tll, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    const char* who = "ktf_vb_forward_backward";
    const int64_t need = ktf_vb_fb_workspace_bytes(TB, N);
    if (need < 0) return (int)need;
    KTF_REQUIRE(K >= 1 && K <= KTF_VB_MAX_SPEAKERS, "%s: %d speakers outside 1 .. %d", who, (int)K, KTF_VB_MAX_SPEAKERS);
    KTF_REQUIRE(loop_prob >= 0.0 && loop_prob <= 1.0, "%s: loop_prob %g outside [0, 1]", who, loop_prob);
    KTF_REQUIRE(boffsets && sp && sp_out && tll && workspace, "%s: null argument", who);
    KTF_REQUIRE(TB == 0 || (lls && q), "%s: null lls / q", who);
    if (ktf_check_workspace(who, workspace, workspace_bytes, need) != KTF_OK) return KTF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const FbLayout l = fb_layout(TB, N);
    int* cstart = (int*)(ws + l.cstart);
    double* Mws = (double*)(ws + l.M);
    double* sc = (double*)(ws + l.sc);
    double* ain = (double*)(ws + l.ain);
    double* bout = (double*)(ws + l.bout);
    double* spc = (double*)(ws + l.spc);
    hipLaunchKernelGGL(fb_cstart_kernel, dim3(1), dim3(64), 0, st, boffsets, (int)N, cstart);
    KTF_CHECK_LAUNCH(who);
    const unsigned nch = (unsigned)l.maxch;
    hipLaunchKernelGGL(fb_matrix_kernel, dim3(nch), dim3(64), 0, st, lls, boffsets, (const int*)cstart, (int)N, TB, (int)K, sp, loop_prob, Mws, sc);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(fb_carry_kernel, dim3(N), dim3(64), 0, st, lls, boffsets, (const int*)cstart, (int)N, TB, l.maxch, (int)K, sp,
                       (const double*)Mws, (const double*)sc, ain, bout, tll);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(fb_post_kernel, dim3(nch), dim3(64), 0, st, lls, boffsets, (const int*)cstart, (int)N, TB, (int)K, sp, loop_prob,
                       (const double*)ain, (const double*)bout, q, spc);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(fb_sp_kernel, dim3(N), dim3(64), 0, st, (const int*)cstart, l.maxch, (int)K, sp, (const double*)spc, sp_out);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int64_t ktf_vb_fb_serial_workspace_bytes(int64_t TB, int32_t N) {
    const char* who = "ktf_vb_fb_serial_workspace_bytes";
    KTF_REQUIRE(TB >= 0 && TB < ((int64_t)1 << 31), "%s: block count %lld out of range", who, (long long)TB);
    KTF_REQUIRE(N >= 1 && N <= 65535, "%s: %d recordings outside 1 .. 65535", who, (int)N);
    return al256((TB > 0 ? TB : 1) * FBK * 8) + al256((TB > 0 ? TB : 1) * 8);
}

extern "C" int ktf_vb_forward_backward_serial(const double* lls, const int32_t* boffsets, int32_t N, int64_t TB, int32_t K, const double* sp,
                                              double loop_prob, double* q, double* sp_out, double* tll, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    const char* who = "ktf_vb_forward_backward_serial";
    const int64_t need = ktf_vb_fb_serial_workspace_bytes(TB, N);
    if (need < 0) return (int)need;
    KTF_REQUIRE(K >= 1 && K <= KTF_VB_MAX_SPEAKERS, "%s: %d speakers outside 1 .. %d", who, (int)K, KTF_VB_MAX_SPEAKERS);
    KTF_REQUIRE(loop_prob >= 0.0 && loop_prob <= 1.0, "%s: loop_prob %g outside [0, 1]", who, loop_prob);
    KTF_REQUIRE(boffsets && sp && sp_out && tll && workspace, "%s: null argument", who);
    KTF_REQUIRE(TB == 0 || (lls && q), "%s: null lls / q", who);
    if (ktf_check_workspace(who, workspace, workspace_bytes, need) != KTF_OK) return KTF_EINVAL;
    char* ws = (char*)workspace;
    double* alpha = (double*)ws;
    double* cbw = (double*)(ws + al256((TB > 0 ? TB : 1) * FBK * 8));
    hipLaunchKernelGGL(fb_serial_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, lls, boffsets, TB, (int)K, sp, loop_prob, alpha, cbw, q, sp_out,
                       tll);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_vb_loglike_sums(const float* loglike, const int32_t* offsets, int32_t N, int64_t F, double* gsum, void* stream) {
    const char* who = "ktf_vb_loglike_sums";
    KTF_REQUIRE(F >= 0 && F < ((int64_t)1 << 31), "%s: frame count %lld out of range", who, (long long)F);
    KTF_REQUIRE(N >= 1 && N <= 65535, "%s: %d recordings outside 1 .. 65535", who, (int)N);
    KTF_REQUIRE(offsets && gsum && (F == 0 || loglike), "%s: null argument", who);
    hipLaunchKernelGGL(vb_gsum_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, loglike, offsets, F, gsum);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_vb_bound(const double* gsum, const double* tll, const double* kl, int32_t N, int32_t K, double stat_scale, double* bound,
                            void* stream) {
    const char* who = "ktf_vb_bound";
    KTF_REQUIRE(N >= 1 && N <= 65535, "%s: %d recordings outside 1 .. 65535", who, (int)N);
    KTF_REQUIRE(K >= 1 && K <= KTF_VB_MAX_SPEAKERS, "%s: %d speakers outside 1 .. %d", who, (int)K, KTF_VB_MAX_SPEAKERS);
    KTF_REQUIRE(gsum && tll && kl && bound, "%s: null argument", who);
    hipLaunchKernelGGL(vb_bound_kernel, dim3(ktf_cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, gsum, tll, kl, (int)N, (int)K, stat_scale, bound);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
