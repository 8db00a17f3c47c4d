/*
 * ktf_augment.h -- waveform augmentation on the GPU: RIR reverberation and noise mixing at a controlled SNR (INTEGRATION.md §2m;
 * entry points of libktf_hip.so next to those of ktf_hip.h, whose conventions and error codes hold here too).
 *
 * Semantics per utterance b: a signal x of n samples, at most one RIR h of L taps, a list of additives; sample rate fs.
 *   1. p_before = mean(x^2).
 *   2. with an RIR: k = the lowest index of max(h) (signed), s0 = max(0, k - round(0.001 fs)), s1 = min(L, k + round(0.05 fs)),
 *      p_sig = mean((x * h[s0:s1])^2) over the full linear convolution (never stored), y = x * h of n + L - 1 samples.
 *      Without: y = x, p_sig = p_before, k = 0, L = 1. (round: to nearest, ties to even. n = 0: y is empty, every power is 0.)
 *   3. each additive (noise, snr_db, start o >= 0, duration d or 0): the noise nu has m samples, d' = d or m, e[t] = nu[t mod m],
 *      p_nu = mean(e^2) over t < d', g = sqrt(10^(-snr_db / 10) p_sig / p_nu) (0 when p_nu = 0), y[o + t] += g e[t] for
 *      t < min(d', len(y) - o); in list order, on the unshifted y.
 *   4. p_after = mean(y^2); volume > 0: y *= volume; else normalize_output and p_after > 0: y *= sqrt(p_before / p_after).
 *   5. out = y[k : k + n] (shift_output) or all n + L - 1 samples; int16: round to nearest even, saturated.
 * Powers and g are fp64 sums of fp32 samples in a fixed order (no floating-point atomics); the convolution, the adds and the scale
 * are fp32. A row's output bits depend on that row's inputs alone: not on the batch, not on the run.
 *
 * The convolution is uniformly partitioned overlap-save: partitions of P = ktf_aug_partition() samples, each a 2P-point real FFT
 * run as a P-point complex one by one workgroup; spectra are P complex fp32 (bin 0 holds the real bins 0 and P).
 *
 * HOST arrays are named so; `*_dev` is the same array on the device (argument checks and sizes come from the host copy, kernels
 * read the device copy). Nothing is copied to or from the host. Every check runs before any launch and needs no GPU.
 */
#ifndef KTF_AUGMENT_H_
#define KTF_AUGMENT_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_AUG_PARTITION 1024
#define KTF_AUG_META 8          /* int32 per RIR: k, s0, s1, L, first full partition, first early partition, 0, 0 */
#define KTF_AUG_STATS 4         /* doubles per row: p_before, p_sig, p_after, the scale applied */
#define KTF_AUG_MAX_SAMPLES (1 << 30)
#define KTF_AUG_DIRECT_TAPS 64  /* a filter (h, or h[s0:s1]) of at most this many taps is applied in the time domain */

/* P. */
int32_t ktf_aug_partition(void);

/* The twiddle tables every transform reads: ktf_aug_tables_floats() floats, filled once per device. */
int64_t ktf_aug_tables_floats(void);
int ktf_aug_tables(float* tables, void* stream);

/* A bank of R >= 0 RIRs, one after another in h (fp32): offsets is a HOST array of R + 1 ascending sample offsets (offsets[0] = 0,
 * every RIR has at least one tap). ktf_aug_rir_spectra_floats: the floats of `spectra` (negative KTF_* code on bad arguments).
 * ktf_aug_rir_prepare fills meta (R x KTF_AUG_META int32) and the partition spectra of every h and h[s0:s1]. */
int64_t ktf_aug_rir_spectra_floats(const int32_t* offsets, int32_t R, int32_t fs);
int ktf_aug_rir_prepare(const float* h, const int32_t* offsets, const int32_t* offsets_dev, int32_t R, int32_t fs,
                        const float* tables, int32_t* meta, float* spectra, void* stream);

/* Bytes of the workspace ktf_aug_convolve and ktf_aug_mix share for B rows: n (HOST, B lengths), rir_ids (HOST, B ids in
 * -1 .. R - 1), rir_lengths (HOST, R tap counts), num_additives in all. Negative KTF_* code on bad arguments. */
int64_t ktf_aug_workspace_bytes(const int32_t* n, const int32_t* rir_ids, int32_t B, const int32_t* rir_lengths, int32_t R,
                                int32_t fs, int64_t num_additives);

/* Steps 1 and 2. x: B rows of ldx elements, fp32 or (x_i16) int16; h, offsets_dev, meta, spectra: the bank as
 * ktf_aug_rir_prepare took and left it (NULL when no row has an RIR). Leaves the unshifted y in the workspace and p_before, p_sig in
 * stats (B x KTF_AUG_STATS doubles). */
int ktf_aug_convolve(const void* x, int32_t x_i16, int64_t ldx, const int32_t* n, const int32_t* n_dev, const int32_t* rir_ids,
                     const int32_t* rir_ids_dev, int32_t B, const int32_t* rir_lengths, int32_t R, int32_t fs, const float* h,
                     const int32_t* offsets_dev, const int32_t* meta, const float* spectra, const float* tables, int64_t num_additives,
                     double* stats, void* workspace, size_t workspace_bytes, void* stream);

/* One additive of a row's list. */
typedef struct KtfAugAdditive {
    int32_t noise;      /* index into the noise bank */
    float snr_db;
    int32_t start;      /* o, in samples of y */
    int32_t duration;   /* d in samples, 0: the noise's own length */
} KtfAugAdditive;

/* Steps 3 to 5 on the y ktf_aug_convolve left (same n, rir_ids, rir_lengths, fs, workspace). add_offsets: HOST CSR of B + 1
 * offsets into adds (HOST, add_offsets[B] additives); noise: the bank's samples (fp32), noise_offsets HOST int64 M + 1 (every noise
 * has at least one sample). out: B rows of ldo elements, fp32 or (out_i16) int16; columns up to T_out are written (zeros past a
 * row's own length: n with shift_output, n + L - 1 without). stats gets p_after and the scale. */
int ktf_aug_mix(const int32_t* n, const int32_t* n_dev, const int32_t* rir_ids, const int32_t* rir_ids_dev, int32_t B,
                const int32_t* rir_lengths, int32_t R, int32_t fs, const int32_t* meta, const int32_t* add_offsets,
                const int32_t* add_offsets_dev, const KtfAugAdditive* adds, const KtfAugAdditive* adds_dev, const float* noise,
                const int64_t* noise_offsets, const int64_t* noise_offsets_dev, int32_t M, int32_t shift_output,
                int32_t normalize_output, double volume, void* out, int32_t out_i16, int64_t ldo, int64_t T_out, double* stats,
                void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
