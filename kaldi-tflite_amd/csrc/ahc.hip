// Agglomerative clustering of dense PLDA scores: Kaldi's `agglomerative-cluster` (AgglomerativeClusterer, single pass), the
// stage of x-vector diarization that follows `ivector-plda-scoring-dense`, batched over the recordings of one call.
//
// Per recording r (n rows, costs C = -scores or scores, strict upper triangle only):
//   ahc_meta_kernel     the per-recording table (offsets, min_clusters, max cluster size) from lengths_dev
//   ahc_expand_kernel   Sigma = the full symmetric n x n cost matrix (diagonal 0, never read) in the workspace    (wide)
//   ahc_best_kernel     every row's best eligible partner among the singletons, one wave per row                   (wide)
//   ahc_merge_kernel    one workgroup per recording: merge the eligible pair with the smallest (avg, lo_id, hi_id)
//                       until none is left or min_clusters is reached, then label the rows
// The merge loop keeps a cached best (avg, partner) per slot. A merge of slots a and b (a: the smaller id, it keeps the
// cluster under the new id) changes only the pairs (k, a): every other row either compares its best against the new pair or,
// when its best partner was a or b, rescans its row of Sigma. Sizes only grow, so a cached best that is eligible stays so.
// Per-slot state (best avg, best partner, size, id, union-find parent, rescan list, id bitmap and its prefix counts) lives in
// LDS up to KTF_AHC_LDS_SLOTS slots and in the workspace above that. All arithmetic is in the block's dtype, divisions
// correctly rounded (no fast-math), so the labels are bit-exact against a restatement of Kaldi's algorithm.
#include "common.h"

namespace {

constexpr int AHC_THREADS = 256;           // the merge kernel: one wave per SIMD, a barrier per phase is the cost
constexpr int AHC_WAVES = AHC_THREADS / 64;
constexpr int AHC_META = 8;                // int64 per recording
enum { A_N = 0, A_OFF = 1, A_ROW = 2, A_ST = 3, A_MINC = 4, A_MAXSZ = 5 };
constexpr int AHC_TILE = 32;               // the expand kernel's square tile
constexpr unsigned NO_PAIR = 0xFFFFFFFFu;  // key of "no eligible pair": above every (lo_id << 16 | hi_id), ids <= 2n - 1 < 65535

__host__ __device__ inline int64_t al16(int64_t b) { return (b + 15) & ~(int64_t)15; }
__host__ __device__ inline int64_t bit_words(int64_t n) { return (2 * n) / 32 + 1; }  // one bit per cluster id 0 .. 2n - 1
__host__ __device__ inline int64_t state_bytes(int64_t n, int esz) {
    return al16(n * esz) + 5 * al16(n * 4) + 2 * al16(bit_words(n) * 4);
}

template <typename R>
struct State {
    R* val;          // cached best avg of the slot (valid when bj >= 0)
    int* bj;         // its partner slot, -1: none eligible
    int* size;       // cluster size, 0: retired
    int* id;         // cluster id (1 .. 2n - 1)
    int* par;        // union-find parent slot (a retired slot points at the slot it merged into)
    int* stale;      // the rows to rescan in this step
    unsigned* bits;  // final cluster ids
    int* pref;       // set bits below each word of `bits`
};

template <typename R>
__device__ inline State<R> state_at(unsigned char* b, int64_t n) {
    State<R> s;
    s.val = (R*)b; b += al16(n * sizeof(R));
    s.bj = (int*)b; b += al16(n * 4);
    s.size = (int*)b; b += al16(n * 4);
    s.id = (int*)b; b += al16(n * 4);
    s.par = (int*)b; b += al16(n * 4);
    s.stale = (int*)b; b += al16(n * 4);
    s.bits = (unsigned*)b; b += al16(bit_words(n) * 4);
    s.pref = (int*)b;
    return s;
}

__device__ inline unsigned pair_key(int i, int j) {
    return i < j ? ((unsigned)i << 16) | (unsigned)j : ((unsigned)j << 16) | (unsigned)i;
}

// (v1, k1) < (v2, k2) lexicographically; NaN never enters (only eligible pairs, avg <= threshold, are candidates)
template <typename R>
__device__ inline bool key_less(R v1, unsigned k1, R v2, unsigned k2) {
    return v1 < v2 || (v1 == v2 && k1 < k2);
}

// the wave's smallest (v, key) and its slot, in every lane
template <typename R>
__device__ inline void wave_argmin(R& v, unsigned& k, int& s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const R ov = __shfl_xor(v, o, 64);
        const unsigned ok = __shfl_xor(k, o, 64);
        const int os = __shfl_xor(s, o, 64);
        if (key_less(ov, ok, v, k)) v = ov, k = ok, s = os;
    }
}

template <typename R>
__device__ inline R inf_of() { return __builtin_huge_val(); }
template <>
__device__ inline float inf_of<float>() { return __builtin_huge_valf(); }

// ----------------------------------------------------------------------------- table
struct Layout {
    size_t meta, sig, st, total;           // byte offsets into the workspace
    int64_t S, max_n, lds_n;               // rows, the largest n, the largest n whose state fits in LDS (0: none)
};

__host__ __device__ inline void fill_meta(const int32_t* lengths, int32_t R_, int esz, const int32_t* minc, float frac,
                                          int64_t* meta, Layout* lay) {
    int64_t S = 0, sc = 0, st = 0, mn = 0, ln = 0;
    for (int32_t r = 0; r < R_; ++r) {
        const int64_t n = lengths[r];
        if (meta) {
            int64_t* m = meta + (int64_t)r * AHC_META;
            m[A_N] = n; m[A_OFF] = sc; m[A_ROW] = S; m[A_ST] = st;
            m[A_MINC] = minc ? minc[r] : 1;
            m[A_MAXSZ] = (int64_t)ceilf((float)n * frac);   // Kaldi: ceil(num_points * max_cluster_fraction) in BaseFloat
            m[6] = m[7] = 0;
        }
        S += n;
        sc += n * n;
        st += al16(state_bytes(n, esz));
        mn = n > mn ? n : mn;
        ln = (n <= KTF_AHC_LDS_SLOTS && n > ln) ? n : ln;
    }
    if (lay) {
        auto al = [](int64_t b) { return (size_t)((b + 255) & ~(int64_t)255); };
        lay->S = S; lay->max_n = mn; lay->lds_n = ln;
        lay->meta = 0;
        lay->sig = al((int64_t)R_ * AHC_META * 8);
        lay->st = lay->sig + al(sc * esz);
        lay->total = lay->st + al(st);
    }
}

__global__ void ahc_meta_kernel(const int32_t* __restrict__ lengths, int32_t R_, int esz, const int32_t* __restrict__ minc, float frac,
                                int64_t* __restrict__ meta) {
    if (threadIdx.x == 0) fill_meta(lengths, R_, esz, minc, frac, meta, nullptr);
}

// ----------------------------------------------------------------------------- init (wide)
// Sigma[i][j] = sign * scores[min(i,j)][max(i,j)], Sigma[i][i] = 0: tile (I, J) of the output reads tile (min, max) of the scores
// (coalesced) and writes it as it is or transposed.
template <typename R>
__global__ __launch_bounds__(256) void ahc_expand_kernel(const R* __restrict__ scores, const int64_t* __restrict__ meta, R sign,
                                                         R* __restrict__ sig) {
    __shared__ R t[AHC_TILE][AHC_TILE + 1];
    const int64_t* m = meta + (int64_t)blockIdx.z * AHC_META;
    const int n = (int)m[A_N];
    const int I = blockIdx.y, J = blockIdx.x;
    if (I * AHC_TILE >= n || J * AHC_TILE >= n) return;
    const R* s = scores + m[A_OFF];
    R* g = sig + m[A_OFF];
    const int lo = I < J ? I : J, hi = I < J ? J : I;
    const int tx = threadIdx.x & (AHC_TILE - 1), ty0 = threadIdx.x / AHC_TILE;
    for (int ty = ty0; ty < AHC_TILE; ty += 256 / AHC_TILE) {
        const int r = lo * AHC_TILE + ty, c = hi * AHC_TILE + tx;
        t[ty][tx] = (r < n && c < n) ? s[(int64_t)r * n + c] : R(0);
    }
    __syncthreads();
    for (int ty = ty0; ty < AHC_TILE; ty += 256 / AHC_TILE) {
        const int i = I * AHC_TILE + ty, j = J * AHC_TILE + tx;
        if (i >= n || j >= n) continue;
        // (i, j) with i < j is scores[i][j]; I <= J holds it at t[ty][tx], I > J never has i < j
        // (i, j) with i > j is scores[j][i]; I >= J holds it at t[tx][ty]
        const R v = i < j ? t[ty][tx] : i > j ? t[tx][ty] : R(0);
        g[(int64_t)i * n + j] = i == j ? R(0) : sign * v;
    }
}

// the best eligible partner of every row among the singletons (avg = cost / 1): one wave per row
template <typename R>
__global__ __launch_bounds__(256) void ahc_best_kernel(const int64_t* __restrict__ meta, const R* __restrict__ sig,
                                                       unsigned char* __restrict__ gst, R thr) {
    const int64_t* m = meta + (int64_t)blockIdx.y * AHC_META;
    const int n = (int)m[A_N];
    const int i = blockIdx.x * AHC_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const bool fits = m[A_MAXSZ] >= 2;
    const R* row = sig + m[A_OFF] + (int64_t)i * n;
    R bv = inf_of<R>();
    unsigned bk = NO_PAIR;
    int bs = -1;
    for (int j = lane; j < n && fits; j += 64) {
        const R avg = row[j] / R(1);
        const unsigned k = pair_key(i + 1, j + 1);
        if (j != i && avg <= thr && key_less(avg, k, bv, bk)) bv = avg, bk = k, bs = j;
    }
    wave_argmin(bv, bk, bs);
    if (lane == 0) {
        State<R> s = state_at<R>(gst + m[A_ST], n);
        s.val[i] = bv;
        s.bj[i] = bs;
    }
}

// ----------------------------------------------------------------------------- merge (one workgroup per recording)
template <typename R>
__global__ __launch_bounds__(AHC_THREADS) void ahc_merge_kernel(const int64_t* __restrict__ meta, R* __restrict__ sig,
                                                                unsigned char* __restrict__ gst, R thr, int lds_n,
                                                                int32_t* __restrict__ labels, int32_t* __restrict__ counts) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ R red_v[AHC_WAVES];
    __shared__ unsigned red_k[AHC_WAVES];
    __shared__ int red_s[AHC_WAVES];
    __shared__ int bc_a, bc_b, bc_size, bc_stop, n_stale, flag;
    __shared__ int part[AHC_THREADS];

    const int64_t* m = meta + (int64_t)blockIdx.x * AHC_META;
    const int n = (int)m[A_N], minc = (int)m[A_MINC], maxsz = (int)m[A_MAXSZ];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    R* S = sig + m[A_OFF];
    State<R> g = state_at<R>(gst + m[A_ST], n);
    const bool in_lds = n <= lds_n;
    State<R> s = in_lds ? state_at<R>(lds, n) : g;
    for (int k = tid; k < n; k += AHC_THREADS) {
        if (in_lds) s.val[k] = g.val[k], s.bj[k] = g.bj[k];
        s.size[k] = 1;
        s.id[k] = k + 1;
        s.par[k] = k;
    }
    if (tid == 0) n_stale = 0;
    __syncthreads();

    int active = n, next_id = n + 1;
    while (active > minc) {
        // 1. the smallest cached key over all slots
        R bv = inf_of<R>();
        unsigned bk = NO_PAIR;
        int bs = -1;
        for (int k = tid; k < n; k += AHC_THREADS) {
            const int j = s.bj[k];
            if (s.size[k] > 0 && j >= 0) {
                const R v = s.val[k];
                const unsigned key = pair_key(s.id[k], s.id[j]);
                if (key_less(v, key, bv, bk)) bv = v, bk = key, bs = k;
            }
        }
        wave_argmin(bv, bk, bs);
        if (lane == 0) red_v[wave] = bv, red_k[wave] = bk, red_s[wave] = bs;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < AHC_WAVES; ++w)
                if (key_less(red_v[w], red_k[w], bv, bk)) bv = red_v[w], bk = red_k[w], bs = red_s[w];
            bc_stop = bs < 0;
            if (bs >= 0) {
                const int p = bs, q = s.bj[bs];
                const int a = s.id[p] < s.id[q] ? p : q, b = p + q - a;
                const int sz = s.size[a] + s.size[b];
                bc_a = a, bc_b = b, bc_size = sz;
                s.size[a] = sz;
                s.size[b] = 0;
                s.id[a] = next_id;
                s.par[b] = a;
            }
        }
        __syncthreads();
        if (bc_stop) break;
        const int a = bc_a, b = bc_b, sz = bc_size;
        // 2. Sigma(k, new) = Sigma(k, a) + Sigma(k, b); every row either takes the new pair into its cached best or is rescanned
        R av = inf_of<R>();
        unsigned ak = NO_PAIR;
        int as = -1;
        for (int k = tid; k < n; k += AHC_THREADS) {
            const int szk = s.size[k];
            if (szk == 0 || k == a) continue;
            const R c = S[(int64_t)a * n + k] + S[(int64_t)b * n + k];
            S[(int64_t)a * n + k] = c;
            S[(int64_t)k * n + a] = c;
            const R avg = c / R(szk * sz);
            const bool ok = avg <= thr && szk + sz <= maxsz;
            const unsigned key = ((unsigned)s.id[k] << 16) | (unsigned)next_id;
            if (ok && key_less(avg, key, av, ak)) av = avg, ak = key, as = k;
            const int j = s.bj[k];
            if (j == a || j == b) {
                s.stale[atomicAdd(&n_stale, 1)] = k;
            } else if (ok && (j < 0 || key_less(avg, key, s.val[k], pair_key(s.id[k], s.id[j])))) {
                s.val[k] = avg;
                s.bj[k] = a;
            }
        }
        wave_argmin(av, ak, as);
        if (lane == 0) red_v[wave] = av, red_k[wave] = ak, red_s[wave] = as;
        __syncthreads();
        // 3. the new cluster's best (thread 0) and the rescans (one wave per stale row)
        if (tid == 0) {
            for (int w = 1; w < AHC_WAVES; ++w)
                if (key_less(red_v[w], red_k[w], av, ak)) av = red_v[w], ak = red_k[w], as = red_s[w];
            s.val[a] = av;
            s.bj[a] = as;
        }
        const int ns = n_stale;
        for (int t = wave; t < ns; t += AHC_WAVES) {
            const int k = s.stale[t], szk = s.size[k], idk = s.id[k];
            const R* row = S + (int64_t)k * n;
            R v = inf_of<R>();
            unsigned kk = NO_PAIR;
            int js = -1;
            for (int j = lane; j < n; j += 64) {
                const int szj = s.size[j];
                if (szj == 0 || j == k) continue;
                const R avg = row[j] / R(szk * szj);
                const unsigned key = pair_key(idk, s.id[j]);
                if (avg <= thr && szk + szj <= maxsz && key_less(avg, key, v, kk)) v = avg, kk = key, js = j;
            }
            wave_argmin(v, kk, js);
            if (lane == 0) s.val[k] = v, s.bj[k] = js;
        }
        __syncthreads();
        if (tid == 0) n_stale = 0;
        --active;
        ++next_id;
    }

    // 4. labels: rank of each final id among the final ids, then every row takes its root's label
    const int W = (int)bit_words(n);
    for (int w = tid; w < W; w += AHC_THREADS) s.bits[w] = 0;
    __syncthreads();
    for (int k = tid; k < n; k += AHC_THREADS)
        if (s.size[k] > 0) atomicOr(&s.bits[s.id[k] >> 5], 1u << (s.id[k] & 31));
    __syncthreads();
    const int chunk = (W + AHC_THREADS - 1) / AHC_THREADS, w0 = tid * chunk, w1 = w0 + chunk < W ? w0 + chunk : W;
    int c = 0;
    for (int w = w0; w < w1; ++w) c += __popc(s.bits[w]);
    part[tid] = c;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < AHC_THREADS; ++t) {
            const int v = part[t];
            part[t] = run;
            run += v;
        }
        counts[blockIdx.x] = run;
    }
    __syncthreads();
    c = part[tid];
    for (int w = w0; w < w1; ++w) {
        s.pref[w] = c;
        c += __popc(s.bits[w]);
    }
    // pointer jumping: every slot's parent becomes its root (an active slot)
    for (;;) {
        if (tid == 0) flag = 0;
        __syncthreads();
        bool moved = false;
        for (int k = tid; k < n; k += AHC_THREADS) {
            const int p = s.par[k], pp = s.par[p];
            if (pp != p) s.par[k] = pp, moved = true;
        }
        if (moved) flag = 1;
        __syncthreads();
        const int more = flag;
        __syncthreads();
        if (!more) break;
    }
    int32_t* out = labels + m[A_ROW];
    for (int k = tid; k < n; k += AHC_THREADS) {
        const int id = s.id[s.par[k]], w = id >> 5;
        out[k] = s.pref[w] + __popc(s.bits[w] & ((1u << (id & 31)) - 1u)) + 1;
    }
}

// ----------------------------------------------------------------------------- host side
// Checks lengths (a HOST array) and sizes the workspace.
static int ahc_layout(const char* who, const int32_t* lengths, int32_t R_, int esz, Layout* lay) {
    KTF_REQUIRE(lengths, "%s: null lengths", who);
    KTF_REQUIRE(R_ >= 1 && R_ < 65536, "%s: R = %d recordings, need 1 .. 65535", who, (int)R_);
    for (int32_t r = 0; r < R_; ++r)
        KTF_REQUIRE(lengths[r] >= 1 && lengths[r] <= KTF_AHC_MAX_N, "%s: lengths[%d] = %d outside 1..%d", who, (int)r, (int)lengths[r],
                    KTF_AHC_MAX_N);
    fill_meta(lengths, R_, esz, nullptr, 1.0f, nullptr, lay);
    return KTF_OK;
}

template <typename R>
static int ahc_launch(const char* who, const R* scores, const int32_t* lengths, const int32_t* lengths_dev, int32_t R_,
                      int32_t read_costs, double threshold, const int32_t* min_clusters_dev, double max_spk_fraction,
                      int32_t* labels, int32_t* num_clusters, void* workspace, size_t workspace_bytes, void* stream) {
    KTF_REQUIRE(scores && lengths_dev && labels && num_clusters && workspace, "%s: null argument", who);
    KTF_REQUIRE(max_spk_fraction > 0 && max_spk_fraction <= 1, "%s: max_spk_fraction %g outside (0, 1]", who, max_spk_fraction);
    Layout lay;
    int rc = ahc_layout(who, lengths, R_, (int)sizeof(R), &lay);
    if (rc != KTF_OK) return rc;
    KTF_REQUIRE(workspace_bytes >= lay.total, "%s: workspace of %zu bytes, need %zu", who, workspace_bytes, lay.total);

    hipStream_t st = (hipStream_t)stream;
    unsigned char* w = (unsigned char*)workspace;
    int64_t* meta = (int64_t*)(w + lay.meta);
    R* sig = (R*)(w + lay.sig);
    unsigned char* gst = w + lay.st;
    const R thr = (R)threshold;                       // Kaldi's threshold is a BaseFloat: fp32 blocks compare against fp32
    hipLaunchKernelGGL(ahc_meta_kernel, dim3(1), dim3(64), 0, st, lengths_dev, R_, (int)sizeof(R), min_clusters_dev,
                       (float)max_spk_fraction, meta);
    KTF_CHECK_LAUNCH(who);
    const unsigned tn = (unsigned)ktf_cdiv(lay.max_n, AHC_TILE);
    hipLaunchKernelGGL(ahc_expand_kernel<R>, dim3(tn, tn, (unsigned)R_), dim3(256), 0, st, scores, meta,
                       read_costs ? R(1) : R(-1), sig);
    KTF_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(ahc_best_kernel<R>, dim3((unsigned)ktf_cdiv(lay.max_n, AHC_WAVES), (unsigned)R_), dim3(256), 0, st, meta,
                       sig, gst, thr);
    KTF_CHECK_LAUNCH(who);
    const size_t lds = lay.lds_n ? (size_t)state_bytes(lay.lds_n, (int)sizeof(R)) : 0;
    KTF_LDS_ONCE((int)state_bytes(KTF_AHC_LDS_SLOTS, (int)sizeof(R)), ahc_merge_kernel<R>);
    hipLaunchKernelGGL(ahc_merge_kernel<R>, dim3((unsigned)R_), dim3(AHC_THREADS), lds, st, meta, sig, gst, thr, (int)lay.lds_n,
                       labels, num_clusters);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

}  // namespace

extern "C" int64_t ktf_ahc_workspace_bytes(const int32_t* lengths, int32_t R, int32_t dtype_bytes) {
    const char* who = "ktf_ahc_workspace_bytes";
    KTF_REQUIRE(dtype_bytes == 4 || dtype_bytes == 8, "%s: dtype_bytes %d, need 4 or 8", who, (int)dtype_bytes);
    Layout lay;
    const int rc = ahc_layout(who, lengths, R, dtype_bytes, &lay);
    return rc == KTF_OK ? (int64_t)lay.total : (int64_t)rc;
}

extern "C" int ktf_ahc_f64(const double* scores, const int32_t* lengths, const int32_t* lengths_dev, int32_t R, int32_t read_costs,
                           double threshold, const int32_t* min_clusters_dev, double max_spk_fraction, int32_t* labels,
                           int32_t* num_clusters, void* workspace, size_t workspace_bytes, void* stream) {
    return ahc_launch<double>("ktf_ahc_f64", scores, lengths, lengths_dev, R, read_costs, threshold, min_clusters_dev, max_spk_fraction,
                              labels, num_clusters, workspace, workspace_bytes, stream);
}
extern "C" int ktf_ahc_f32(const float* scores, const int32_t* lengths, const int32_t* lengths_dev, int32_t R, int32_t read_costs,
                           double threshold, const int32_t* min_clusters_dev, double max_spk_fraction, int32_t* labels,
                           int32_t* num_clusters, void* workspace, size_t workspace_bytes, void* stream) {
    return ahc_launch<float>("ktf_ahc_f32", scores, lengths, lengths_dev, R, read_costs, threshold, min_clusters_dev, max_spk_fraction,
                             labels, num_clusters, workspace, workspace_bytes, stream);
}
