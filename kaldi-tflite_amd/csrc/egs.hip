// Training examples (include/ktf_egs.h, whose rule numbers the comments use).
//   ktf_egs_draw      egs_draw_kernel: a thread per batch row
//   ktf_egs_gather    egs_chunk_kernel<DRAW = false>: a workgroup per (batch row, slice of its chunk), the plan read from utt / offset
//   ktf_egs_sample    egs_chunk_kernel<DRAW = true>: the same workgroups derive the row's draw themselves, in wave-uniform code
//   ktf_egs_philox    the generator on the host
// One access pattern for every alignment (rule 9): a lane reads one element of the bank and writes one float, consecutive lanes on
// consecutive elements of the (T, ldo) chunk. No arithmetic on values: fp32 is copied, fp16 is widened.
#include <hip/hip_fp16.h>

#include "common.h"
#include "../../include/ktf_egs.h"

namespace {

constexpr int EGS_THREADS = KTF_EGS_THREADS;
constexpr int EGS_SLICE_ELEMS = EGS_THREADS * 8;      // elements of a chunk a workgroup takes before a row is cut into more slices

// Philox4x32-10 (Salmon et al., SC'11), the one function host and device run
__host__ __device__ inline void egs_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

__host__ __device__ inline int egs_idx(uint32_t r, int n) { return (int)(((uint64_t)r * (uint32_t)n) >> 32); }

struct EgsDrawParams {
    KtfEgsIndex ix;
    int S, U, n_spk, T;
    uint32_t seed_lo, seed_hi, step_lo, step_hi;
    int64_t b0, b_stride;
};

struct EgsBankParams {
    const void* bank;
    int64_t rows, ldb;
    const int64_t* row0;
    const int32_t* len;
    int U, D, T;
    int64_t ldo;
};

struct EgsPlan {
    int utt, offset, label;
};

// rules 1 - 7 for global row b; every index entry is checked before it addresses anything
__device__ __forceinline__ EgsPlan egs_draw_row(const EgsDrawParams& p, uint32_t b) {
    const EgsPlan none = {-1, 0, -1};
    uint32_t r[4];
    egs_philox(b, p.step_lo, p.step_hi, 0u, p.seed_lo, p.seed_hi, r);
    const int s = p.ix.spk_order[egs_idx(r[0], p.n_spk)];              // n_spk <= S: inside spk_order
    if (s < 0 || s >= p.S) return none;
    const int first = p.ix.spk_off[s], n = p.ix.spk_off[s + 1] - first;
    if (first < 0 || n < 0 || (int64_t)first + n > p.U) return none;
    const int32_t* __restrict__ ul = p.ix.spk_utt_len + first;
    int lo = 0, hi = n;                                                // ul descending: m = the count of entries >= T
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ul[mid] >= p.T) lo = mid + 1;
        else hi = mid;
    }
    if (lo == 0) return none;
    const int k = egs_idx(r[1], lo);
    const int u = p.ix.spk_utts[first + k], L = ul[k];
    if (u < 0 || u >= p.U || L < p.T) return none;
    return {u, egs_idx(r[2], L - p.T + 1), s};
}

// rule 7 for a plan row: the first bank row of the chunk, or -1 for a chunk of zeros
__device__ __forceinline__ int64_t egs_chunk_row(const EgsBankParams& p, int u, int off) {
    if (u < 0 || u >= p.U || off < 0) return -1;
    const int64_t first = p.row0[u], n = p.len[u];
    if ((int64_t)off + p.T > n || first < 0 || first > p.rows || n > p.rows - first) return -1;
    return first + off;
}

__global__ __launch_bounds__(EGS_THREADS) void egs_draw_kernel(EgsDrawParams p, int B, int32_t* __restrict__ utt, int32_t* __restrict__ offset,
                                                              int32_t* __restrict__ label) {
    const int64_t i = (int64_t)blockIdx.x * EGS_THREADS + threadIdx.x;
    if (i >= B) return;
    const EgsPlan d = egs_draw_row(p, (uint32_t)(p.b0 + i * p.b_stride));
    utt[i] = d.utt;
    offset[i] = d.offset;
    label[i] = d.label;
}

// grid (B, slices). Workgroup (i, y) writes the elements y * 256 + tid, + slices * 256, ... of batch row i's (T, ldo) chunk.
template <typename E, bool DRAW>
__global__ __launch_bounds__(EGS_THREADS) void egs_chunk_kernel(EgsDrawParams dp, EgsBankParams p, const int32_t* plan_utt,
                                                               const int32_t* plan_offset, int32_t* __restrict__ utt,
                                                               int32_t* __restrict__ offset, int32_t* __restrict__ label,
                                                               float* __restrict__ out) {
    const int64_t i = blockIdx.x;
    EgsPlan d;
    if (DRAW) {
        d = egs_draw_row(dp, (uint32_t)(dp.b0 + i * dp.b_stride));     // the same in every lane: scalar code
        if (blockIdx.y == 0 && threadIdx.x == 0) {
            utt[i] = d.utt;
            offset[i] = d.offset;
            label[i] = d.label;
        }
    } else {
        d.utt = plan_utt[i];
        d.offset = plan_offset[i];
    }
    const int64_t row = egs_chunk_row(p, d.utt, d.offset);
    const int64_t total = (int64_t)p.T * p.ldo, step = (int64_t)gridDim.y * EGS_THREADS;
    const int64_t step_t = step / p.ldo, step_d = step % p.ldo;
    int64_t e = (int64_t)blockIdx.y * EGS_THREADS + threadIdx.x;
    int64_t t = e / p.ldo, c = e % p.ldo;
    float* __restrict__ o = out + i * total;
    if (row < 0) {
        for (; e < total; e += step) o[e] = 0.0f;
        return;
    }
    const E* __restrict__ src = reinterpret_cast<const E*>(p.bank) + row * p.ldb;
#pragma unroll 4
    for (; e < total; e += step) {
        o[e] = c < p.D ? (float)src[t * p.ldb + c] : 0.0f;
        t += step_t;
        c += step_d;
        if (c >= p.ldo) {
            c -= p.ldo;
            ++t;
        }
    }
}

int egs_draw_check(const char* who, const KtfEgsIndex* index, int64_t S, int64_t U, int64_t n_spk, uint64_t seed, uint64_t step, int64_t T,
                   int64_t b0, int64_t b_stride, int64_t B, const int32_t* utt, const int32_t* offset, const int32_t* label,
                   EgsDrawParams* p) {
    KTF_REQUIRE(index && index->spk_order && index->spk_off && index->spk_utts && index->spk_utt_len && utt && offset && label,
                "%s: null argument", who);
    KTF_REQUIRE(B >= 0, "%s: negative size", who);
    KTF_REQUIRE(T >= 1, "%s: T %lld below 1", who, (long long)T);
    KTF_REQUIRE(S >= 1 && U >= 1, "%s: S %lld or U %lld below 1", who, (long long)S, (long long)U);
    KTF_REQUIRE(B < (1ll << 31) && T < (1ll << 31) && S < (1ll << 31) && U < (1ll << 31), "%s: B, T, S or U reaches 2^31", who);
    KTF_REQUIRE(n_spk >= 1 && n_spk <= S, "%s: n_spk %lld outside [1, S = %lld]", who, (long long)n_spk, (long long)S);
    KTF_REQUIRE(b_stride >= 1 && b0 >= 0, "%s: b_stride %lld below 1 or b0 %lld below 0", who, (long long)b_stride, (long long)b0);
    KTF_REQUIRE(b0 < (1ll << 31) && b_stride < (1ll << 31) && (B == 0 || b0 + (B - 1) * b_stride < (1ll << 31)),
                "%s: the last global row reaches 2^31", who);
    p->ix = *index;
    p->S = (int)S;
    p->U = (int)U;
    p->n_spk = (int)n_spk;
    p->T = (int)T;
    p->seed_lo = (uint32_t)seed;
    p->seed_hi = (uint32_t)(seed >> 32);
    p->step_lo = (uint32_t)step;
    p->step_hi = (uint32_t)(step >> 32);
    p->b0 = b0;
    p->b_stride = b_stride;
    return KTF_OK;
}

int egs_bank_check(const char* who, const void* bank, int32_t bank_dtype, int64_t rows, int64_t ldb, int64_t D, const int64_t* row0,
                   const int32_t* len, int64_t U, int64_t T, int64_t B, const float* out, int64_t ldo, EgsBankParams* p) {
    KTF_REQUIRE(bank && row0 && len && out, "%s: null argument", who);
    KTF_REQUIRE(B >= 0 && rows >= 0, "%s: negative size", who);
    KTF_REQUIRE(D >= 1, "%s: D %lld below 1", who, (long long)D);
    KTF_REQUIRE(T >= 1, "%s: T %lld below 1", who, (long long)T);
    KTF_REQUIRE(U >= 1, "%s: U %lld below 1", who, (long long)U);
    KTF_REQUIRE(bank_dtype == KTF_F32 || bank_dtype == KTF_F16, "%s: unknown bank dtype %d", who, (int)bank_dtype);
    KTF_REQUIRE(B < (1ll << 31) && T < (1ll << 31) && D < (1ll << 31) && U < (1ll << 31) && ldb < (1ll << 31) && ldo < (1ll << 31),
                "%s: B, T, D, U or a leading dimension reaches 2^31", who);
    KTF_REQUIRE(B * T < (1ll << 31), "%s: B * T reaches 2^31", who);
    KTF_REQUIRE(ldb >= D && ldo >= D, "%s: leading dimension below D %lld", who, (long long)D);
    KTF_REQUIRE(rows < (1ll << 62) / ldb, "%s: the bank reaches 2^62 elements", who);
    const uintptr_t a0 = (uintptr_t)bank, a1 = a0 + (uintptr_t)(rows * ldb) * (bank_dtype == KTF_F16 ? 2 : 4);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)(B * T * ldo) * 4;
    KTF_REQUIRE(!(a0 < a1 && o0 < o1 && a0 < o1 && o0 < a1), "%s: out overlaps the bank", who);
    p->bank = bank;
    p->rows = rows;
    p->ldb = ldb;
    p->row0 = row0;
    p->len = len;
    p->U = (int)U;
    p->D = (int)D;
    p->T = (int)T;
    p->ldo = ldo;
    return KTF_OK;
}

template <bool DRAW>
int egs_launch_chunks(const char* who, const EgsDrawParams& dp, const EgsBankParams& p, int32_t bank_dtype, int64_t B, const int32_t* plan_utt,
                      const int32_t* plan_offset, int32_t* utt, int32_t* offset, int32_t* label, float* out, void* stream) {
    const int64_t total = (int64_t)p.T * p.ldo;
    int64_t slices = (total + EGS_SLICE_ELEMS - 1) / EGS_SLICE_ELEMS;
    if (slices > KTF_EGS_MAX_SLICES) slices = KTF_EGS_MAX_SLICES;
    const dim3 grid((unsigned)B, (unsigned)slices), block(EGS_THREADS);
    if (bank_dtype == KTF_F16)
        hipLaunchKernelGGL((egs_chunk_kernel<__half, DRAW>), grid, block, 0, (hipStream_t)stream, dp, p, plan_utt, plan_offset, utt, offset,
                           label, out);
    else
        hipLaunchKernelGGL((egs_chunk_kernel<float, DRAW>), grid, block, 0, (hipStream_t)stream, dp, p, plan_utt, plan_offset, utt, offset,
                           label, out);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------ entry points
extern "C" int ktf_egs_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
    KTF_REQUIRE(ctr && key && out, "ktf_egs_philox: null argument");
    egs_philox(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out);
    return KTF_OK;
}

extern "C" int ktf_egs_draw(const KtfEgsIndex* index, int64_t S, int64_t U, int64_t n_spk, uint64_t seed, uint64_t step, int64_t T,
                            int64_t b0, int64_t b_stride, int64_t B, int32_t* utt, int32_t* offset, int32_t* label, void* stream) {
    const char* who = "ktf_egs_draw";
    EgsDrawParams p = {};
    if (int rc = egs_draw_check(who, index, S, U, n_spk, seed, step, T, b0, b_stride, B, utt, offset, label, &p)) return rc;
    if (B == 0) return KTF_OK;
    hipLaunchKernelGGL(egs_draw_kernel, dim3((unsigned)ktf_cdiv(B, EGS_THREADS)), dim3(EGS_THREADS), 0, (hipStream_t)stream, p, (int)B, utt,
                       offset, label);
    KTF_CHECK_LAUNCH(who);
    return KTF_OK;
}

extern "C" int ktf_egs_gather(const void* bank, int32_t bank_dtype, int64_t rows, int64_t ldb, int64_t D, const int64_t* row0,
                              const int32_t* len, int64_t U, const int32_t* utt, const int32_t* offset, int64_t T, int64_t B, float* out,
                              int64_t ldo, void* stream) {
    const char* who = "ktf_egs_gather";
    KTF_REQUIRE(utt && offset, "%s: null argument", who);
    EgsBankParams p = {};
    if (int rc = egs_bank_check(who, bank, bank_dtype, rows, ldb, D, row0, len, U, T, B, out, ldo, &p)) return rc;
    if (B == 0) return KTF_OK;
    return egs_launch_chunks<false>(who, EgsDrawParams{}, p, bank_dtype, B, utt, offset, nullptr, nullptr, nullptr, out, stream);
}

extern "C" int ktf_egs_sample(const KtfEgsIndex* index, int64_t S, int64_t U, int64_t n_spk, uint64_t seed, uint64_t step, int64_t T,
                              int64_t b0, int64_t b_stride, int64_t B, const void* bank, int32_t bank_dtype, int64_t rows, int64_t ldb,
                              int64_t D, const int64_t* row0, const int32_t* len, float* out, int64_t ldo, int32_t* utt, int32_t* offset,
                              int32_t* label, void* stream) {
    const char* who = "ktf_egs_sample";
    EgsDrawParams dp = {};
    EgsBankParams p = {};
    if (int rc = egs_draw_check(who, index, S, U, n_spk, seed, step, T, b0, b_stride, B, utt, offset, label, &dp)) return rc;
    if (int rc = egs_bank_check(who, bank, bank_dtype, rows, ldb, D, row0, len, U, T, B, out, ldo, &p)) return rc;
    if (B == 0) return KTF_OK;
    return egs_launch_chunks<true>(who, dp, p, bank_dtype, B, nullptr, nullptr, utt, offset, label, out, stream);
}
