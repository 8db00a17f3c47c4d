// Sample-rate conversion (include/ktf_resample.h): the windowed-sinc polyphase plan on the host, and one kernel that resamples a
// ragged batch.
//
// A workgroup owns KTF_RS_TILE consecutive outputs [s0, s0 + TILE) of one row. It loads the input span those outputs need, coalesced
// and once, into LDS as fp32 (zero outside [0, n): the load address is clamped into the row, nothing past n is read; RS_LOADS loads
// per thread are in flight at a time), and the weight table too when it fits beside it. Output s = u ou + i reads
// x[first[i] + u iu + j], j < taps[i]. A thread takes a task (phase i, units u0 + g + r G for r < RS_R, G = the tile's units / RS_R
// rounded up): its RS_R outputs share every weight, so a step of the tap loop is one weight read and RS_R sample reads from LDS for
// RS_R fp64 fused multiply-adds (5 bytes per FMA with RS_R = 4, against 8 for one output per thread); RS_J taps are read ahead of
// their use. Lanes of a wave run over g first: they read samples iu apart and the same weight (a broadcast); table rows in LDS are an
// odd number of floats apart for the lanes that differ in i. With an even iu, lanes iu apart share banks in a 4-byte read, and every
// base of a thread has one parity: the samples are then read as 8-byte aligned pairs (after one single tap when that parity is odd).
// The products of two fp32 values are exact in fp64, so the fused multiply-add is rule 4's "exact product, added in ascending j";
// the sum is rounded to fp32 once, staged in LDS and stored coalesced with the zeros from m to T_out. No atomics; a row's bits
// depend on its own samples and the plan only. Outputs of a task that fall outside the tile read a zero tail behind the span.
#include <math.h>

#include "common.h"
#include "../../include/ktf_resample.h"

namespace {

constexpr int RS_TILE = KTF_RS_TILE;
constexpr int RS_THREADS = 256;
constexpr int RS_R = 4;                         // outputs of one phase per task
constexpr int RS_J = 4;                         // taps per step of the tap loop
constexpr int RS_LOADS = 8;                     // global loads a thread issues before it waits for the first
constexpr int RS_LDS_FLOATS = 16384;            // 64 KiB of LDS per workgroup at most
static_assert(RS_J % 2 == 0, "the tap loop reads pairs");
static_assert(RS_TILE % RS_THREADS == 0, "the store loop covers the tile");
static_assert(KTF_RS_MAX_SPAN + KTF_RS_MAX_TAPS + 2 + RS_TILE <= RS_LDS_FLOATS, "span, its zero tail and the staged outputs fit LDS");

struct RsUnits {
    int32_t g, iu, ou;
    double ww;
};

int check_rates(const char* who, int32_t fi, int32_t fo, double cutoff, int32_t zeros, RsUnits* un) {
    KTF_REQUIRE(fi > 0 && fo > 0, "%s: rates %d -> %d must be positive", who, (int)fi, (int)fo);
    KTF_REQUIRE(fi != fo, "%s: equal rates (%d): nothing to resample", who, (int)fi);
    KTF_REQUIRE(zeros >= 1, "%s: zeros = %d, must be at least 1", who, (int)zeros);
    const double half = 0.5 * (double)(fi < fo ? fi : fo);
    KTF_REQUIRE(cutoff > 0.0 && cutoff <= half, "%s: cutoff %g out of range (0 < cutoff <= %g)", who, cutoff, half);
    int32_t a = fi, b = fo;
    while (b) { const int32_t r = a % b; a = b; b = r; }
    un->g = a;
    un->iu = fi / a;
    un->ou = fo / a;
    un->ww = (double)zeros / (2.0 * cutoff);
    return KTF_OK;
}

// rule 2's window of phase i
inline void phase_window(const RsUnits& un, int32_t fi, int32_t fo, int32_t i, double* t, int64_t* lo, int64_t* hi) {
    *t = (double)i / (double)fo;
    *lo = (int64_t)ceil((*t - un.ww) * (double)fi);
    *hi = (int64_t)floor((*t + un.ww) * (double)fi);
}

// the most units a tile's outputs reach past its first one
inline int64_t tile_unit_reach(int32_t ou) { return ((int64_t)RS_TILE - 1 + ou - 1) / ou; }

int plan_sizes(const char* who, int32_t fi, int32_t fo, double cutoff, int32_t zeros, RsUnits* un, int32_t* max_taps) {
    const int rc = check_rates(who, fi, fo, cutoff, zeros, un);
    if (rc != KTF_OK) return rc;
    int64_t widest = 0, fmin = INT64_MAX, emax = INT64_MIN;
    for (int32_t i = 0; i < un->ou; ++i) {
        double t;
        int64_t lo, hi;
        phase_window(*un, fi, fo, i, &t, &lo, &hi);
        const int64_t nt = hi - lo + 1;
        KTF_REQUIRE(nt >= 1 && nt <= KTF_RS_MAX_TAPS, "%s: %d -> %d: phase %d has %lld taps (1 .. %d)", who, (int)fi, (int)fo, (int)i,
                    (long long)nt, KTF_RS_MAX_TAPS);
        widest = nt > widest ? nt : widest;
        fmin = lo < fmin ? lo : fmin;
        emax = hi + 1 > emax ? hi + 1 : emax;
    }
    KTF_REQUIRE((int64_t)un->ou * widest <= KTF_RS_MAX_TABLE_FLOATS, "%s: %d -> %d: a table of %d x %lld weights, above %d", who, (int)fi,
                (int)fo, (int)un->ou, (long long)widest, KTF_RS_MAX_TABLE_FLOATS);
    const int64_t span = tile_unit_reach(un->ou) * un->iu + (emax - fmin);
    KTF_REQUIRE(span <= KTF_RS_MAX_SPAN, "%s: %d -> %d: a tile of %d outputs spans %lld input samples, above %d", who, (int)fi, (int)fo,
                RS_TILE, (long long)span, KTF_RS_MAX_SPAN);
    *max_taps = (int32_t)widest;
    return KTF_OK;
}

template <bool I16>
__device__ __forceinline__ float rs_sample(const void* row, int64_t k) {
    if constexpr (I16) return (float)reinterpret_cast<const short*>(row)[k];
    else return reinterpret_cast<const float*>(row)[k];
}

// tap j of the thread's RS_R outputs
__device__ __forceinline__ void rs_tap(double (&acc)[RS_R], float w, const float* xs, const int (&base)[RS_R], int j) {
    const double wv = (double)w;
#pragma unroll
    for (int r = 0; r < RS_R; ++r) acc[r] = fma(wv, (double)xs[base[r] + j], acc[r]);
}

// taps j, j + RS_J, ... while RS_J of them are left: every LDS read of a step is issued before its use. PAIRS: base[r] + j is even
// for every r, and the samples are read as 8-byte pairs. -> the first tap not done
template <bool PAIRS>
__device__ __forceinline__ int rs_taps(double (&acc)[RS_R], const float* wr, const float* xs, const int (&base)[RS_R], int j, int nt) {
    for (; j + RS_J <= nt; j += RS_J) {
        float wq[RS_J], xq[RS_R][RS_J];
#pragma unroll
        for (int q = 0; q < RS_J; ++q) wq[q] = wr[j + q];
#pragma unroll
        for (int r = 0; r < RS_R; ++r)
#pragma unroll
            for (int q = 0; q < RS_J; q += 2) {
                if constexpr (PAIRS) {
                    const float2 v = *reinterpret_cast<const float2*>(__builtin_assume_aligned(xs + base[r] + j + q, 8));
                    xq[r][q] = v.x;
                    xq[r][q + 1] = v.y;
                } else {
                    xq[r][q] = xs[base[r] + j + q];
                    xq[r][q + 1] = xs[base[r] + j + q + 1];
                }
            }
#pragma unroll
        for (int q = 0; q < RS_J; ++q) {
            const double wv = (double)wq[q];
#pragma unroll
            for (int r = 0; r < RS_R; ++r) acc[r] = fma(wv, (double)xq[r][q], acc[r]);
        }
    }
    return j;
}

struct RsArgs {
    const void* x;
    int64_t ldx;
    const int32_t* n;
    const int32_t* first;
    const int32_t* taps;
    const float* w;
    void* out;
    int64_t ldo, T_out;
    int32_t iu, ou, ldw, max_taps;
    int32_t fmin, emax;         // the lowest first[i], the highest first[i] + taps[i]
    int32_t ordered;            // first[] and first[] + taps[] ascend with i and wrap by at most iu: the tile's span is exact
    int32_t span_floats;        // floats of LDS for the span and its zero tail
};

// workgroup (tile, b). WLDS: the table is copied into LDS (rows of max_taps | 1 floats).
template <bool XI16, bool OI16, bool WLDS>
__global__ __launch_bounds__(RS_THREADS) void rs_kernel(const RsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    float* xs = rs_lds;                             // the span, then max_taps + 2 zeros
    float* os = rs_lds + a.span_floats;             // the tile's outputs
    float* wl = os + RS_TILE;                       // the table (WLDS)
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t s0 = (int64_t)blockIdx.x * RS_TILE;
    const int64_t n = a.n[b];
    const int64_t m = n == 0 ? 0 : (n * a.ou + a.iu - 1) / a.iu;
    if (s0 < m) {                                   // (workgroup-uniform)
        const int64_t s_end = (s0 + RS_TILE < m ? s0 + RS_TILE : m) - 1;
        const int64_t u_first = s0 / a.ou, u_last = s_end / a.ou;
        int64_t lo, hi;
        if (a.ordered) {
            const int i0 = (int)(s0 - u_first * a.ou), i1 = (int)(s_end - u_last * a.ou);
            lo = a.first[i0] + u_first * a.iu;
            hi = a.first[i1] + a.taps[i1] + u_last * a.iu;
            if (u_last > u_first) {
                const int64_t lo2 = a.first[0] + (u_first + 1) * a.iu;
                const int64_t hi2 = a.first[a.ou - 1] + a.taps[a.ou - 1] + (u_last - 1) * a.iu;
                lo = lo2 < lo ? lo2 : lo;
                hi = hi2 > hi ? hi2 : hi;
            }
        } else {
            lo = a.fmin + u_first * a.iu;
            hi = a.emax + u_last * a.iu;
        }
        const int span = (int)(hi - lo);            // <= span_floats - max_taps - 2 (the host's bound)
        const void* row = XI16 ? (const void*)(reinterpret_cast<const short*>(a.x) + (int64_t)b * a.ldx)
                               : (const void*)(reinterpret_cast<const float*>(a.x) + (int64_t)b * a.ldx);
        // RS_LOADS loads per thread in flight: the address is clamped into [0, n) (n >= 1 here), the value dropped outside
        for (int at = tid; at < span + a.max_taps + 2; at += RS_THREADS * RS_LOADS) {
            float v[RS_LOADS];
#pragma unroll
            for (int q = 0; q < RS_LOADS; ++q) {
                const int64_t k = lo + at + q * RS_THREADS;
                v[q] = rs_sample<XI16>(row, k < 0 ? 0 : (k < n ? k : n - 1));
            }
#pragma unroll
            for (int q = 0; q < RS_LOADS; ++q) {
                const int idx = at + q * RS_THREADS;
                const int64_t k = lo + idx;
                if (idx < span + a.max_taps + 2) xs[idx] = (idx < span && k >= 0 && k < n) ? v[q] : 0.0f;
            }
        }
        const int ldl = a.max_taps | 1;
        if constexpr (WLDS) {
            const int di = RS_THREADS / a.max_taps, dj = RS_THREADS - di * a.max_taps;
            int i = tid / a.max_taps, j = tid - i * a.max_taps;
            while (i < a.ou) {                                      // (i, j) steps RS_THREADS elements of the table at a time
                wl[i * ldl + j] = a.w[(int64_t)i * a.ldw + j];
                i += di;
                j += dj;
                if (j >= a.max_taps) { j -= a.max_taps; ++i; }
            }
        }
        __syncthreads();
        const int units = (int)(u_last - u_first) + 1;
        const int G = (units + RS_R - 1) / RS_R;
        const bool pairs = (a.iu & 1) == 0;
        const int tasks = a.ou * G;
        for (int task = tid; task < tasks; task += RS_THREADS) {
            const int i = task / G, g = task - i * G;
            const int nt = a.taps[i];
            const int64_t f = a.first[i];
            // with an even iu every live base of the thread has the parity of first[i] - lo: pairs of samples are read 8-byte aligned
            const int odd = (int)((f - lo) & 1);
            int base[RS_R], slot[RS_R];
#pragma unroll
            for (int r = 0; r < RS_R; ++r) {
                const int64_t u = u_first + g + (int64_t)r * G;
                const int64_t s = u * a.ou + i;
                const bool live = s >= s0 && s <= s_end;
                slot[r] = live ? (int)(s - s0) : -1;
                base[r] = live ? (int)(f + u * a.iu - lo) : span + ((span ^ odd) & 1);      // (a dead output reads the zero tail)
            }
            double acc[RS_R];
#pragma unroll
            for (int r = 0; r < RS_R; ++r) acc[r] = 0.0;
            const float* wr = WLDS ? wl + i * ldl : a.w + (int64_t)i * a.ldw;
            int j = 0;
            if (pairs) {
                if (odd) {
                    rs_tap(acc, wr[0], xs, base, 0);
                    j = 1;
                }
                j = rs_taps<true>(acc, wr, xs, base, j, nt);
            } else {
                j = rs_taps<false>(acc, wr, xs, base, j, nt);
            }
            for (; j < nt; ++j) rs_tap(acc, wr[j], xs, base, j);
#pragma unroll
            for (int r = 0; r < RS_R; ++r)
                if (slot[r] >= 0) os[slot[r]] = (float)acc[r];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < RS_TILE / RS_THREADS; ++q) {
        const int c = tid + RS_THREADS * q;
        const int64_t s = s0 + c;
        if (s >= a.T_out) continue;
        const float v = s < m ? os[c] : 0.0f;
        if constexpr (OI16) {
            const float r = fminf(fmaxf(rintf(v), -32768.0f), 32767.0f);
            reinterpret_cast<short*>(a.out)[(int64_t)b * a.ldo + s] = (short)(int)r;
        } else {
            reinterpret_cast<float*>(a.out)[(int64_t)b * a.ldo + s] = v;
        }
    }
}

template <bool XI16, bool OI16>
void rs_launch(bool wlds, dim3 grid, size_t lds, hipStream_t st, const RsArgs& a) {
    if (wlds) hipLaunchKernelGGL((rs_kernel<XI16, OI16, true>), grid, dim3(RS_THREADS), lds, st, a);
    else hipLaunchKernelGGL((rs_kernel<XI16, OI16, false>), grid, dim3(RS_THREADS), lds, st, a);
}

}  // namespace

extern "C" int32_t ktf_rs_tile(void) { return RS_TILE; }

extern "C" int ktf_rs_plan_sizes(int32_t fi, int32_t fo, double cutoff, int32_t zeros, int32_t* ou, int32_t* iu, int32_t* max_taps) {
    const char* who = "ktf_rs_plan_sizes";
    KTF_REQUIRE(ou && iu && max_taps, "%s: null argument", who);
    RsUnits un;
    int32_t widest = 0;
    const int rc = plan_sizes(who, fi, fo, cutoff, zeros, &un, &widest);
    if (rc != KTF_OK) return rc;
    *ou = un.ou;
    *iu = un.iu;
    *max_taps = widest;
    return KTF_OK;
}

extern "C" int ktf_rs_plan(int32_t fi, int32_t fo, double cutoff, int32_t zeros, int32_t* first, int32_t* taps, float* w, int32_t ldw) {
    const char* who = "ktf_rs_plan";
    RsUnits un;
    int32_t widest = 0;
    const int rc = plan_sizes(who, fi, fo, cutoff, zeros, &un, &widest);
    if (rc != KTF_OK) return rc;
    KTF_REQUIRE(first && taps && w, "%s: null argument", who);
    KTF_REQUIRE(ldw >= widest, "%s: ldw = %d below the widest phase (%d taps)", who, (int)ldw, (int)widest);
    const double two_pi_cutoff = 2.0 * M_PI * cutoff;
    for (int32_t i = 0; i < un.ou; ++i) {
        double t;
        int64_t lo, hi;
        phase_window(un, fi, fo, i, &t, &lo, &hi);
        first[i] = (int32_t)lo;
        taps[i] = (int32_t)(hi - lo + 1);
        float* row = w + (int64_t)i * ldw;
        for (int32_t j = 0; j < ldw; ++j) {
            if (j >= taps[i]) { row[j] = 0.0f; continue; }
            const double d = (double)(lo + j) / (double)fi - t;
            const double win = fabs(d) < un.ww ? 0.5 * (1.0 + cos(two_pi_cutoff / (double)zeros * d)) : 0.0;
            const double f = d != 0.0 ? sin(two_pi_cutoff * d) / (M_PI * d) : 2.0 * cutoff;
            row[j] = (float)(f * win / (double)fi);
        }
    }
    return KTF_OK;
}

extern "C" int64_t ktf_rs_num_out(int64_t n, int32_t fi, int32_t fo) {
    const char* who = "ktf_rs_num_out";
    KTF_REQUIRE(fi > 0 && fo > 0, "%s: rates %d -> %d must be positive", who, (int)fi, (int)fo);
    KTF_REQUIRE(n >= 0 && n <= KTF_RS_MAX_SAMPLES, "%s: n = %lld samples (0 .. 2^30)", who, (long long)n);
    if (n == 0) return 0;
    int32_t a = fi, b = fo;
    while (b) { const int32_t r = a % b; a = b; b = r; }
    const int64_t per_in = fo / a, per_out = fi / a;            // tick / fi, tick / fo
    const int64_t span = n * per_in;
    int64_t last = span / per_out;
    if (last * per_out == span) --last;
    return last + 1;
}

extern "C" int ktf_rs_resample(const void* x, int32_t x_i16, int64_t ldx, const int32_t* n, const int32_t* n_dev, int32_t B, int32_t iu,
                               int32_t ou, const int32_t* first, const int32_t* taps, const int32_t* first_dev, const int32_t* taps_dev,
                               const float* w_dev, int32_t ldw, void* out, int32_t out_i16, int64_t ldo, int64_t T_out, void* stream) {
    const char* who = "ktf_rs_resample";
    KTF_REQUIRE(B >= 0 && ldx >= 0 && ldo >= 0 && T_out >= 0, "%s: negative size (B = %d, ldx = %lld, ldo = %lld, T_out = %lld)", who, (int)B,
                (long long)ldx, (long long)ldo, (long long)T_out);
    KTF_REQUIRE(iu >= 1 && ou >= 1 && iu != ou, "%s: units %d -> %d (positive, not equal)", who, (int)iu, (int)ou);
    KTF_REQUIRE(first && taps, "%s: null argument", who);
    int32_t widest = 0, fmin = INT32_MAX, emax = INT32_MIN;
    bool ordered = true;
    for (int32_t i = 0; i < ou; ++i) {
        KTF_REQUIRE(taps[i] >= 1 && taps[i] <= KTF_RS_MAX_TAPS, "%s: phase %d has %d taps (1 .. %d)", who, (int)i, (int)taps[i], KTF_RS_MAX_TAPS);
        KTF_REQUIRE(first[i] > -(1 << 24) && first[i] < (1 << 24), "%s: phase %d starts at %d", who, (int)i, (int)first[i]);
        widest = taps[i] > widest ? taps[i] : widest;
        fmin = first[i] < fmin ? first[i] : fmin;
        emax = first[i] + taps[i] > emax ? first[i] + taps[i] : emax;
        if (i > 0 && (first[i] < first[i - 1] || first[i] + taps[i] < first[i - 1] + taps[i - 1])) ordered = false;
    }
    if (first[ou - 1] > first[0] + iu || first[ou - 1] + taps[ou - 1] > first[0] + taps[0] + iu) ordered = false;
    KTF_REQUIRE(ldw >= widest, "%s: ldw = %d below the widest phase (%d taps)", who, (int)ldw, (int)widest);
    KTF_REQUIRE((int64_t)ou * widest <= KTF_RS_MAX_TABLE_FLOATS, "%s: a table of %d x %d weights, above %d", who, (int)ou, (int)widest,
                KTF_RS_MAX_TABLE_FLOATS);
    const int64_t span = tile_unit_reach(ou) * iu + ((int64_t)emax - fmin);
    KTF_REQUIRE(span <= KTF_RS_MAX_SPAN, "%s: a tile of %d outputs spans %lld input samples, above %d", who, RS_TILE, (long long)span,
                KTF_RS_MAX_SPAN);
    KTF_REQUIRE(B == 0 || n, "%s: null argument", who);
    int64_t max_n = 0, max_m = 0;
    for (int32_t b = 0; b < B; ++b) {
        KTF_REQUIRE(n[b] >= 0 && n[b] <= KTF_RS_MAX_SAMPLES, "%s: negative size or too long (row %d has n = %d; 0 .. 2^30)", who, (int)b,
                    (int)n[b]);
        const int64_t m = n[b] == 0 ? 0 : ((int64_t)n[b] * ou + iu - 1) / iu;
        KTF_REQUIRE(m <= KTF_RS_MAX_SAMPLES, "%s: row %d would have %lld output samples, above 2^30", who, (int)b, (long long)m);
        max_n = n[b] > max_n ? n[b] : max_n;
        max_m = m > max_m ? m : max_m;
    }
    KTF_REQUIRE(ldx >= max_n, "%s: row stride %lld below the longest row (%lld)", who, (long long)ldx, (long long)max_n);
    KTF_REQUIRE(T_out >= max_m && ldo >= T_out, "%s: T_out = %lld, ldo = %lld: need ldo >= T_out >= %lld (the longest output row)", who,
                (long long)T_out, (long long)ldo, (long long)max_m);
    if (B == 0 || T_out == 0) return KTF_OK;
    KTF_REQUIRE(B < 65536, "%s: B = %d rows, at most 65535 per call (chunk them)", who, (int)B);
    KTF_REQUIRE(n_dev && first_dev && taps_dev && w_dev && out && (x || max_n == 0), "%s: null argument", who);
    RsArgs a;
    a.x = x; a.ldx = ldx; a.n = n_dev; a.first = first_dev; a.taps = taps_dev; a.w = w_dev; a.out = out; a.ldo = ldo; a.T_out = T_out;
    a.iu = iu; a.ou = ou; a.ldw = ldw; a.max_taps = widest; a.fmin = fmin; a.emax = emax; a.ordered = ordered ? 1 : 0;
    a.span_floats = (int32_t)span + widest + 2;
    const int64_t table = (int64_t)ou * (widest | 1);
    const bool wlds = a.span_floats + RS_TILE + table <= RS_LDS_FLOATS;
    const size_t lds = (size_t)(a.span_floats + RS_TILE + (wlds ? table : 0)) * sizeof(float);
    const dim3 grid((unsigned)ktf_cdiv(T_out, RS_TILE), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (x_i16 && out_i16) rs_launch<true, true>(wlds, grid, lds, st, a);
    else if (x_i16) rs_launch<true, false>(wlds, grid, lds, st, a);
    else if (out_i16) rs_launch<false, true>(wlds, grid, lds, st, a);
    else rs_launch<false, false>(wlds, grid, lds, st, a);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}
