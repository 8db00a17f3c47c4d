/*
 * ktf_resample.h -- sample-rate conversion and speed perturbation on the GPU: a windowed-sinc polyphase resampler with the rules of
 * Kaldi's LinearResample / ResampleWaveform in its whole-signal (flush = true) mode, on a ragged batch (entry
 * points of libktf_hip.so next to those of ktf_hip.h and ktf_augment.h, whose conventions and error codes hold here too).
 *
 * The rules are the project's own, modelled on Kaldi's; where they and Kaldi differ, these govern. All arithmetic of rules 1 to 4 is
 * IEEE fp64 in the operation order written. fi, fo: positive integers, fi != fo. zeros: an integer >= 1 (Kaldi's default 6).
 * cutoff: 0 < cutoff <= min(fi, fo) / 2 (Kaldi's default 0.99 * 0.5 * min(fi, fo)).
 *   1. Units. g = gcd(fi, fo), iu = fi / g, ou = fo / g: the input and output samples per repeating unit, so there are ou phases.
 *      ww = zeros / (2 cutoff).
 *   2. Phase i < ou. t = i / fo, lo = ceil((t - ww) fi), hi = floor((t + ww) fi); first[i] = lo (it may be negative),
 *      taps[i] = hi - lo + 1. For input index k = lo + j: d = k / fi - t,
 *        win = 0.5 (1 + cos(((2 pi cutoff) / zeros) d)) if |d| < ww, else 0,
 *        f = sin((2 pi cutoff) d) / (pi d) if d != 0, else 2 cutoff,
 *        w[i][j] = f win / fi, then rounded to fp32.
 *      (A tap on the window's edge has weight 0 up to rounding: one tap more or fewer from the ceil / floor cannot matter.)
 *   3. Length of n input samples. m = 0 if n = 0; otherwise tick = lcm(fi, fo), span = n (tick / fi), last = span // (tick / fo),
 *      last -= 1 if last (tick / fo) == span, m = last + 1. (tick / fi = ou and tick / fo = iu: m = ceil(n ou / iu).)
 *   4. Output sample s < m. u, i = divmod(s, ou), k0 = first[i] + u iu, y[s] = sum_j w[i][j] x[k0 + j] with x = 0 outside [0, n):
 *      each product of an fp32 weight and an fp32 sample formed exactly in fp64, added in ascending j in fp64, rounded to fp32 once.
 *   5. int16 input is read as int16 and converted exactly; int16 output rounds the fp32 result to nearest even and saturates. No
 *      atomics. A row's output bits depend on that row's samples, fi, fo, cutoff and zeros only: not on the batch, ldx, the tiling,
 *      the run, or on what lies past n in the row.
 *   6. Refused (KTF_EINVAL, before any launch, no GPU needed): non-positive rates; fi == fo; cutoff out of range; zeros < 1; a table
 *      (ou x max taps) above KTF_RS_MAX_TABLE_FLOATS or taps above KTF_RS_MAX_TAPS; a decimation so steep that the input span of one
 *      tile exceeds KTF_RS_MAX_SPAN samples; more than KTF_RS_MAX_SAMPLES samples in a row, in or out. (Python also refuses
 *      non-integer rates and multi-channel input; there equal rates return the input unfiltered -- Kaldi would low-pass it.)
 *   7. Not implemented: the streaming mode (flush = false, carried remainders), ArbitraryResample, multi-channel.
 *
 * The plan (first, taps, w) is pure host code; the caller uploads it once. HOST arrays are named so; `*_dev` is the same array on the
 * device (checks and sizes come from the host copy, kernels read the device copy). Every check runs before any launch.
 */
#ifndef KTF_RESAMPLE_H_
#define KTF_RESAMPLE_H_

#include "ktf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_RS_TILE 1024                    /* consecutive outputs of one row per workgroup */
#define KTF_RS_MAX_TAPS 256                 /* 48000 -> 8000 has 73, 44100 -> 16000 has 34 */
#define KTF_RS_MAX_TABLE_FLOATS (1 << 16)   /* ou x max taps; 44100 -> 16000 has 160 x 34 = 5440 */
#define KTF_RS_MAX_SPAN 12288               /* input samples under one tile: about KTF_RS_TILE fi / fo + taps (48000 -> 8000: 6211) */
#define KTF_RS_MAX_SAMPLES (1 << 30)

/* The tile's output count. */
int32_t ktf_rs_tile(void);

/* Rule 1 and the widest phase of rule 2: *ou, *iu, *max_taps. KTF_OK, or a negative KTF_* code (rule 6). */
int ktf_rs_plan_sizes(int32_t fi, int32_t fo, double cutoff, int32_t zeros, int32_t* ou, int32_t* iu, int32_t* max_taps);

/* Rule 2 into HOST arrays: first (ou int32), taps (ou int32), w (ou rows of ldw >= max taps fp32, zero past a row's taps). */
int ktf_rs_plan(int32_t fi, int32_t fo, double cutoff, int32_t zeros, int32_t* first, int32_t* taps, float* w, int32_t ldw);

/* Rule 3: m for n input samples (a negative KTF_* code on bad arguments). */
int64_t ktf_rs_num_out(int64_t n, int32_t fi, int32_t fo);

/* Rules 4 and 5 on B rows. x: B rows of ldx elements, fp32 or (x_i16) int16; n: HOST, B lengths (n[b] <= ldx; nothing past n[b] is
 * read). The plan as ktf_rs_plan left it: iu, ou, first / taps (HOST), first_dev / taps_dev / w_dev (rows of ldw floats). out: B rows
 * of ldo elements, fp32 or (out_i16) int16; columns up to T_out are written, zeros from a row's m on (T_out >= every row's m). */
int ktf_rs_resample(const void* x, int32_t x_i16, int64_t ldx, const int32_t* n, const int32_t* n_dev, int32_t B, int32_t iu, int32_t ou,
                    const int32_t* first, const int32_t* taps, const int32_t* first_dev, const int32_t* taps_dev, const float* w_dev,
                    int32_t ldw, void* out, int32_t out_i16, int64_t ldo, int64_t T_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
