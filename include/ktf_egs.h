/*
 * ktf_egs.h -- training examples ("egs") on the GPU: random fixed-length chunks of a bank of feature rows, drawn per batch row by a
 * counter-based generator and gathered into a dense fp32 batch, the stage of Kaldi's sid/nnet3/xvector recipe (get_egs.sh,
 * allocate_egs.py) between the front-end and the training step. Entry points of libktf_hip.so next to those of ktf_hip.h, whose
 * conventions and error codes hold here too (kernels: csrc/egs.hip). There is no
 * floating-point arithmetic: every output is an integer or a copied (fp32) / exactly converted (fp16 -> fp32) element.
 *
 * The bank. A flat row-major matrix (rows, ldb) of fp32 (KTF_F32) or fp16 (KTF_F16) on the device, ldb >= D. Utterance u of U owns
 * the rows [row0[u], row0[u] + len[u]); row0 is int64, len is int32, both on the device. Speaker labels are 0 .. S - 1.
 *
 * The index (KtfEgsIndex: four int32 arrays on the device, built on the host and uploaded once per view of the bank).
 *   spk_order[S]     the speakers sorted by the length of their longest utterance, descending; ties: the lower speaker first.
 *   spk_off[S + 1]   speaker s owns the entries [spk_off[s], spk_off[s + 1]) of the next two arrays; spk_off[0] = 0, spk_off[S] = U.
 *   spk_utts[U]      each speaker's utterances sorted by length, descending; ties: the lower utterance index first.
 *   spk_utt_len[U]   spk_utt_len[k] = len[spk_utts[k]].
 *
 * The generator. Philox4x32-10 with the published constants (multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9,
 * 0xBB67AE85); ktf_egs_philox runs the very function the kernels run, on the host. A bounded draw from a 32-bit word r is
 * idx(r, n) = ((uint64_t)r * n) >> 32, 0 <= n < 2^31. Its bias is at most n * 2^-32: below 3e-5 for any n a bank holds per utterance
 * (n < 2^17 rows is 22 minutes of 10 ms frames), and below 0.5 at the limit.
 *
 * Rules, for global batch row b at (seed, step, T); n_spk = the number of speakers whose longest utterance has at least T rows (the
 * first n_spk entries of spk_order), which the caller counts on its host copy of the index:
 *   1. (r0, r1, r2, _) = philox(ctr = (b, step_lo, step_hi, 0), key = (seed_lo, seed_hi)); _lo / _hi: the low / high 32 bits.
 *   2. s = spk_order[idx(r0, n_spk)].
 *   3. m = the number of utterances of s with len >= T, by binary search in spk_utt_len[spk_off[s] .. spk_off[s + 1]).
 *   4. u = spk_utts[spk_off[s] + idx(r1, m)].
 *   5. offset = idx(r2, spk_utt_len[spk_off[s] + idx(r1, m)] - T + 1).
 *   6. label = s.
 *      A batch row is a function of (seed, step, b) alone: not of B, b0, b_stride or of any other row. (Kaldi's allocator walks a
 *      shuffled list of speakers; these are independent draws with the same marginal.)
 *   7. Never a fault. A draw that cannot be completed -- m = 0 (n_spk too large), an index entry out of range (s outside [0, S), a
 *      speaker's span outside [0, U], u outside [0, U)), a length below T -- gives utt = -1, offset = 0, label = -1. A plan row with
 *      utt outside [0, U), offset < 0, offset + T > len[utt], or row0[utt] < 0 or row0[utt] + len[utt] > rows, gives an all-zero
 *      chunk. No such row reads the bank, and no row reads outside its (rows, ldb) extent. label = -1 is an ignored row of
 *      ktf_loss_margin_softmax_*.
 *   8. Gather. out is fp32 (B, T, ldo), ldo >= D: out[i, t, d] = (float)bank[(row0[utt[i]] + offset[i] + t) * ldb + d] for d < D;
 *      columns [D, ldo) are written as zero; columns [D, ldb) of the bank are never read (NaN allowed, as in rows no utterance owns).
 *   9. Alignment. There is one path: a lane reads one element of the bank (four or two bytes) and writes one float, consecutive
 *      lanes on consecutive elements of the row-major (T, ldo) chunk, so a wave writes 256 contiguous bytes per instruction and, for
 *      a compact bank (ldb = D = ldo), reads one contiguous run. Nothing depends on the alignment of bank, row0, out, ldb or ldo
 *      beyond that of an element.
 *  10. ktf_egs_sample = ktf_egs_draw then ktf_egs_gather of what it drew, in one launch, bit for bit. A workgroup owns a slice of
 *      one batch row; it derives the row's draw once, in wave-uniform code. No atomics, no LDS, no scratch. The same call twice
 *      gives the same bits.
 *  11. Refused (KTF_EINVAL, before any launch, no GPU needed): a null index or index array, utt, offset, label, bank, row0, len or
 *      out (each where the call takes it); D < 1, T < 1, B < 0, S < 1, U < 1, rows < 0; n_spk < 1 or n_spk > S; b_stride < 1,
 *      b0 < 0, or a last global row b0 + (B - 1) * b_stride at or beyond 2^31; ldb < D, ldo < D; a bank dtype other than KTF_F32 /
 *      KTF_F16; B, T, D, ldb, ldo, S or U at or beyond 2^31; B * T at or beyond 2^31; out overlapping the bank. B = 0 launches
 *      nothing. Elements are addressed in 64 bits.
 */
#ifndef KTF_EGS_H_
#define KTF_EGS_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_F16 2                 /* bank dtype: IEEE binary16 (next to KTF_F32 of ktf_hip.h) */
#define KTF_EGS_THREADS 256       /* threads of a workgroup */
#define KTF_EGS_MAX_SLICES 32     /* workgroups a batch row is cut into, at most */

typedef struct {
    const int32_t* spk_order;     /* [S] */
    const int32_t* spk_off;       /* [S + 1] */
    const int32_t* spk_utts;      /* [U] */
    const int32_t* spk_utt_len;   /* [U] */
} KtfEgsIndex;

/* Philox4x32-10 on the host: out = philox(ctr, key). KTF_EINVAL for a null pointer. Needs no GPU. */
int ktf_egs_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out);

/* Rules 1 - 7 for the global rows b0 + i * b_stride, i < B: utt, offset, label are B int32 each. */
int ktf_egs_draw(const KtfEgsIndex* index, int64_t S, int64_t U, int64_t n_spk, uint64_t seed, uint64_t step, int64_t T, int64_t b0,
                 int64_t b_stride, int64_t B, int32_t* utt, int32_t* offset, int32_t* label, void* stream);

/* Rules 7 - 9 for an explicit plan (utt, offset: B int32 each, read only). */
int ktf_egs_gather(const void* bank, int32_t bank_dtype, int64_t rows, int64_t ldb, int64_t D, const int64_t* row0, const int32_t* len,
                   int64_t U, const int32_t* utt, const int32_t* offset, int64_t T, int64_t B, float* out, int64_t ldo, void* stream);

/* Rule 10: the call a training step makes. */
int ktf_egs_sample(const KtfEgsIndex* index, int64_t S, int64_t U, int64_t n_spk, uint64_t seed, uint64_t step, int64_t T, int64_t b0,
                   int64_t b_stride, int64_t B, const void* bank, int32_t bank_dtype, int64_t rows, int64_t ldb, int64_t D,
                   const int64_t* row0, const int32_t* len, float* out, int64_t ldo, int32_t* utt, int32_t* offset, int32_t* label,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
