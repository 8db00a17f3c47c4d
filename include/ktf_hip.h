/*
 * ktf_hip.h — C-ABI of libktf_hip.so: the MI355X (gfx950) kernels behind the
 * wav -> x-vector hot path of shahruk10/kaldi-tflite.
 *
 * The reference has no FFI of its own: its operator API is the Keras layer protocol
 * and every layer's `call` is a chain of TensorFlow ops. Each entry point below
 * replaces the TF op chain of one (or a fused run of) reference layer call(s); the
 * reference location it replaces is cited per function (paths relative to
 * kaldi_tflite/lib/ in the reference tree). The Python host side
 * (kaldi-tflite_amd/kaldi_tflite_amd) mirrors the reference's ktf.layers / ktf.models
 * surface and binds these symbols with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - plain C symbols, plain pointers and sizes, no C++/torch types;
 *  - every pointer is a DEVICE pointer unless stated; the caller owns every buffer
 *    (including workspaces); the library allocates nothing and keeps no state except a
 *    thread-local error string;
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *    default stream) and is safe to capture into a hipGraph;
 *  - return value: 0 = KTF_OK, negative = error (ktf_last_error() has the text);
 *  - fp32 tensors are row-major; "ld*" arguments are row strides in ELEMENTS;
 *  - ragged batches: activations are kept utterance-strided (B, T_max, D) with a device
 *    int32 `lens[B]` giving the number of valid rows of each utterance (NULL = all T).
 */
#ifndef KTF_HIP_H_
#define KTF_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KTF_OK 0
#define KTF_EINVAL (-1)     /* bad argument */
#define KTF_ELAUNCH (-2)    /* HIP launch/runtime error */
#define KTF_EUNSUPPORTED (-3)

/* element types of activation / weight buffers */
#define KTF_F32 0
#define KTF_BF16 1
/* (2 was KTF_F16, the element type of the half-precision modes below) */
#define KTF_BF16P 3         /* a bf16 PAIR in an fp32-sized slot: bits 0-15 = bf16(v) (round to nearest even), bits 16-31 =
                             * bf16(v - bf16(v)): 16 mantissa bits, the shapes / strides / padding of fp32 (zero = 0x00000000).
                             * Operands of KTF_GEMM_BF16X4; KTF_GEMM_F32 and KTF_GEMM_BF16X4 can write it (y_dtype) */

/* GEMM arithmetic of ktf_tdnn */
#define KTF_GEMM_F32 0      /* v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate (parity path) */
#define KTF_GEMM_BF16 1     /* v_mfma_f32_*_bf16: bf16 operands, fp32 accumulate */
#define KTF_GEMM_BF16X3 2   /* split-bf16: x=hi+lo, w=hi+lo, 3 bf16 MFMA passes, fp32 accumulate */
/* (3 and 4 were KTF_GEMM_F16, one half-precision pass, and KTF_GEMM_F16X2, two half passes with a calibrated one-pass tail: round 2's
 * timed mode, superseded by KTF_GEMM_F16MX -- faster, tighter on speech, no calibration. Removed from the library in round 5;
 * tools/mx/experiments/README.md names the commit at which they were last part of it.) */
#define KTF_GEMM_F16MX 5    /* ONE half-precision MFMA pass plus two block-scaled (OCP MX) residual passes on
                             * v_mfma_scale_f32_16x16x128_f8f6f4, which runs fp4 / fp6 operands at four times the half rate:
                             *   y = x_h * w_h + x_l4 * w_4 + x_4 * w_l6
                             * (x_h, w_h half; x_l4 = e2m1 image of x - x_h; w_4 = e2m1 image of w; x_4 = e2m1 image of x_h;
                             * w_l6 = e2m3 image of w - w_h; one E8M0 scale per 32 K elements). 1.5 MFMA passes per algorithmic
                             * flop with ~15 significant bits on BOTH operands, no calibration. What is left is zero-mean rounding
                             * noise per frame that the statistics pooling averages, so the max-abs x-vector deviation depends on
                             * the voiced length: 1.2e-5 on 10 s of noise, 2-5e-5 on 10 s of speech, 4-6.5e-5 on 5 s, up to 1.2e-4
                             * on 1-1.5 s (tests/test_gpu_margin.py). The host side (Sequential.MIN_FRAMES, XvectorExtractor.route_short_utterances) sends
                             * utterances below 400 voiced frames through KTF_GEMM_BF16X3. Through ktf_tdnn_mx / ktf_tdnn_mx_stats
                             * on the four-plane activation format ktf_mx_planes produces */
#define KTF_GEMM_BF16X4 6   /* all four bf16 products of (x_hi + x_lo)(w_hi + w_lo), fp32 accumulate, on SMALL tiles (64 x 32..96,
                             * csrc/tdnn_pair.hip): x and w of KTF_BF16P, y KTF_F32 or KTF_BF16P, through ktf_tdnn (w_lo NULL). For
                             * batches too small to fill the chip on 256-row tiles -- a single utterance -- where it replaces the
                             * fp32 small-tile kernels in every mode but KTF_GEMM_F32: x-vectors ~1e-5 from the fp64 oracle */

/* activations fused into the ktf_tdnn epilogue */
#define KTF_ACT_NONE 0
#define KTF_ACT_RELU 1
#define KTF_ACT_SIGMOID 2
#define KTF_ACT_TANH 3
/* the rest of tf.keras.activations of the reference's TensorFlow (2.8; layers/tdnn/tdnn.py:117-118 accepts any of its names):
 * ktf_tdnn with KTF_GEMM_F32 and an fp32 output runs them as a second launch over the rows it wrote (ktf_activation_f32); the 16-bit
 * and MX kernels fuse KTF_ACT_NONE / KTF_ACT_RELU only (the host runs such layers on the fp32 kernels) */
#define KTF_ACT_ELU 4            /* x > 0 ? x : exp(x) - 1 */
#define KTF_ACT_SELU 5           /* 1.0507 * (x > 0 ? x : 1.67326 * (exp(x) - 1)) */
#define KTF_ACT_SOFTPLUS 6       /* log(exp(x) + 1) */
#define KTF_ACT_SOFTSIGN 7       /* x / (|x| + 1) */
#define KTF_ACT_SWISH 8          /* x * sigmoid(x) */
#define KTF_ACT_GELU 9           /* 0.5 x (1 + erf(x / sqrt 2)): approximate=False, the default */
#define KTF_ACT_EXPONENTIAL 10   /* exp(x) */
#define KTF_ACT_HARD_SIGMOID 11  /* clip(0.2 x + 0.5, 0, 1) */
#define KTF_ACT_SOFTMAX 12       /* over the units of a row (axis = -1) */

int32_t ktf_version(void);
/* copies the calling thread's last error text (NUL-terminated) into buf; returns its length */
size_t ktf_last_error(char* buf, size_t cap);
/* 16 hex digits of the sha256 over the library's sources (csrc/Makefile): measurements kept under profiles/ name the build they were
 * made on with it (bench.py attaches a stored HBM-traffic figure only to the build it belongs to). A static string. */
const char* ktf_build_id(void);
/* measurement aid (bench.py): ONE wave that stays resident for `us` microseconds beside whatever else runs on `stream`'s device
 * and reads the shader clock (s_memtime) against the constant 100 MHz counter (s_memrealtime). out (device, 4 x uint64):
 * [0] shader clocks and [1] 100 MHz ticks over the whole stay, [2] / [3] the lowest / highest clock in kHz over ~1 ms windows.
 * Launch it on a stream of its own next to the timed work. 0 < us <= 10 000 000. */
int ktf_clock_probe(unsigned long long* out, int64_t us, void* stream);

/* ------------------------------------------------------------------ front-end (a1-a5)
 * Framing   layers/dsp/framing.py:243-265       (tf.gather of frame indexes)
 * Windowing layers/dsp/windowing.py:180-209     (dither, DC removal, log-energy, pre-emphasis, window)
 * FilterBank layers/dsp/filterbank.py:225-242   (pad, tf.signal.rfft, abs, pow, matmul mel, log)
 * DCT       layers/dsp/dct.py:175-176           (matmul)
 * MFCC      layers/dsp/mfcc.py:197-244          (the three above + lifter + C0 <- energy)
 */
typedef struct KtfFrontendCfg {
    int32_t frame_size;    /* samples per frame (= 2*(size//2), framing.py:104-106)            */
    int32_t frame_shift;   /* samples between frame starts                                      */
    int32_t nfft;          /* power of two >= frame_size, 64..2048 (filterbank.py:156-157)       */
    int32_t num_mels;      /* mel bins  (<= 128)                                                 */
    int32_t num_ceps;      /* cepstra kept (<= num_mels)                                         */
    int32_t remove_dc;     /* windowing.py:186-189                                               */
    int32_t raw_energy;    /* energy before (1) or after (0) pre-emphasis+window                 */
    int32_t use_energy;    /* compute log-energy (Windowing.return_energy / MFCC.use_energy)     */
    int32_t use_power;     /* |X|^2 (1) or |X| (0)                                               */
    int32_t use_log;       /* log(max(.,0)+eps) after the mel bank                               */
    int32_t use_lifter;    /* multiply cepstra by `lifter` (mfcc.py:211-212)                     */
    float preemph;         /* 0 disables                                                         */
    float dither;          /* 0 disables; else x += N(0,1)*dither (counter-based RNG, `seed`)    */
    float energy_floor;    /* clip of the LOG energy from below (windowing.py:177)               */
    float eps;             /* epsilon inside both logs                                           */
    int32_t pad_mode;      /* KTF_IN_WAV* only. 0: Framing as the reference (no padding, T = 1+(n-size)/shift).
                            * 1: Kaldi snip-edges=false framing: the waveform is mirror-padded as by the reference's
                            *    kaldi_numpy PadWaveform (kaldi_numpy/frame_extraction.py:28-89) -- fused into the frame
                            *    gather, nothing is materialised; T = (n + shift/2) / shift                             */
    int32_t row_stride;    /* KTF_IN_WAV* only: samples between the starts of consecutive rows of `in`; 0 = n (dense).
                            * A stride < n describes OVERLAPPING windows of one long recording (sliding-window /
                            * diarization extraction, torch `wav.unfold(-1, n, hop)`) without copying them            */
} KtfFrontendCfg;

typedef struct KtfFrontendTables {   /* all DEVICE pointers, built once by the host */
    const float* window;       /* [frame_size]                                             */
    const float* twiddle;      /* [nfft]   : (cos,-sin)(2*pi*k/(nfft/2)), k < nfft/2        */
    const float* rtwiddle;     /* [nfft]   : (cos,-sin)(2*pi*k/nfft),     k < nfft/2        */
    const int32_t* mel_start;  /* [num_mels] first FFT bin of each filter                  */
    const int32_t* mel_len;    /* [num_mels] number of bins of each filter                 */
    const float* mel_w;        /* [num_mels][mel_stride] weights from mel_start            */
    const float* dct;          /* [num_mels][num_ceps] (filterbank.py melBank / dct.py dct) */
    const float* lifter;       /* [num_ceps] or NULL                                       */
    /* optional tables of the register-resident nfft = 512 fast path (all three NULL = generic kernel); `reserved` = bins of the
     * longest mel work item, 1..16 (checked: the shipped-configuration instances read (reserved + 6) / 4 16-byte pieces per item) */
    const float* fast_tw;      /* [64][18] per-lane FFT twiddles: (re,im) of W256^(n0 r), W64^(n1 r), W16^(n2 r), r=1..3,
                                  n0 = (l>>1)+32(l&1), n1 = (l>>1)&15, n2 = (l>>1)&3                                   */
    const int32_t* fast_mel_meta; /* [64][4] per-lane mel work item: first bin, bins (<=16), filter (-1 = idle),
                                     flags (1: lane+1 same filter, 2: lane+2 same filter, 4: first lane of the filter) */
    const float* fast_mel_w;   /* [64][16] weights of the work item                                                  */
    int32_t mel_stride;
    int32_t reserved;
} KtfFrontendTables;

/* input kinds / output stages of ktf_frontend_f32 */
#define KTF_IN_WAV 0         /* in = (B, N) samples; frames are gathered on the fly (Framing fused)   */
#define KTF_IN_FRAMES 1      /* in = (B, T, frame_size) frames                                        */
#define KTF_IN_WINDOWED 2    /* in = (B, T, frame_size) already-windowed frames (FilterBank alone)     */
#define KTF_IN_WAV_I16 3     /* in = (B, N) int16 PCM samples (half the HBM / PCIe bytes of KTF_IN_WAV) */
#define KTF_OUT_FRAMES 0     /* out (B,T,frame_size): Framing.call                                    */
#define KTF_OUT_WINDOWED 1   /* out (B,T,frame_size) [+ energy (B,T)]: Windowing.call                 */
#define KTF_OUT_FBANK 2      /* out (B,T,num_mels): FilterBank.call                                    */
#define KTF_OUT_MFCC 3       /* out (B,T,num_ceps): MFCC.call                                          */

/* Number of frames Framing produces from n samples: 1 + (n - frame_size) / frame_shift (0 if n < size). */
int64_t ktf_num_frames(int64_t n_samples, int32_t frame_size, int32_t frame_shift);
/* The same for a given KtfFrontendCfg.pad_mode (1: (n + shift/2) / shift; -1 if the mirror padding is undefined for n). */
int64_t ktf_num_frames_padded(int64_t n_samples, int32_t frame_size, int32_t frame_shift, int32_t pad_mode);

/* One launch for any prefix/suffix of Framing -> Windowing -> FilterBank -> DCT/lifter/C0.
 * `n` is the number of samples per row for KTF_IN_WAV, else the number of frames T.
 * `energy` (B,T) may be NULL unless out_stage == KTF_OUT_WINDOWED and cfg->use_energy. */
int ktf_frontend_f32(const void* in, int64_t B, int64_t n, int32_t in_kind, const KtfFrontendCfg* cfg,
                     const KtfFrontendTables* tab, int32_t out_stage, float* out, float* energy,
                     uint64_t seed, void* stream);

/* Which kernel instance ktf_frontend_f32 runs for a given call, and on what grid: the launcher takes its decision from the function
 * behind this query, so the two cannot disagree. Host arithmetic only (no GPU call; it works without a GPU). The table POINTERS of
 * `tab` are only tested for NULL, never followed; its two integers are read. The refusals and error codes are those of
 * ktf_frontend_f32 itself, except for the `in` / `out` pointers, which this call does not see. */
#define KTF_FE_NONE 0        /* nothing is launched (no utterance, or no frame)                                              */
#define KTF_FE_FRAMING 1     /* KTF_OUT_FRAMES: the gather kernel (any frame size)                                           */
#define KTF_FE_GENERIC 2     /* frontend_kernel<log2_nfft>: one wave per frame, FFT in LDS, nfft 64..2048                    */
#define KTF_FE_FAST512 3     /* frontend512_kernel<dither, kind, mfix, std, nq>: register-resident nfft = 512                */
typedef struct KtfFrontendPlan {
    int32_t kernel;      /* KTF_FE_*                                                                                         */
    int32_t log2_nfft;   /* 6..11 (GENERIC, FAST512: 9); 0 otherwise                                                         */
    int32_t dither;      /* FAST512: the instance that draws dither noise                                                    */
    int32_t kind;        /* FAST512: 1 = fp32 samples / frames read plainly, 2 = int16 samples, 0 = general (mirror padding) */
    int32_t mfix;        /* FAST512: frame size known at compile time (400), or 0 = cfg->frame_size                          */
    int32_t std;         /* FAST512: the shipped configuration's switches known at compile time                              */
    int32_t nq;          /* FAST512: 16-byte pieces of the power spectrum a mel work item reads (3, 4 or 5)                  */
    int32_t grid_x, grid_y;
    int64_t lds_bytes;   /* dynamic LDS of the launch                                                                        */
    int64_t T;           /* frames per utterance                                                                             */
} KtfFrontendPlan;
int ktf_frontend_plan(int64_t B, int64_t n, int32_t in_kind, const KtfFrontendCfg* cfg, const KtfFrontendTables* tab,
                      int32_t out_stage, KtfFrontendPlan* plan);

/* DCT.call (layers/dsp/dct.py:175-176) on its own: out[r, c] = sum_m x[r, m] * dct[m, c] (* lifter[c]). */
int ktf_dct_f32(const float* x, int64_t rows, int32_t in_dim, int32_t out_dim, const float* dct,
                const float* lifter, float* out, void* stream);

/* ------------------------------------------------------------------ VAD / compaction / CMVN (a6-a8)
 * VAD.call            layers/dsp/vad.py:156-203
 * gather_nd+expand    models/kaldi/xvector_extractor.py:163-165 (per utterance; see DESIGN.md on batch>1)
 * CMVN.call           layers/normalization/cmvn.py:186-250
 */
typedef struct KtfVadCfg {
    float energy_threshold;
    float energy_mean_scale;    /* 0 disables the mean term */
    float proportion_threshold;
    int32_t frames_context;
    int32_t energy_coeff;       /* column of the log-energy */
} KtfVadCfg;

typedef struct KtfCmvnCfg {
    int32_t window;      /* N */
    int32_t norm_vars;   /* divide by the windowed std (no epsilon, as the reference) */
    int32_t valid;       /* padding == "VALID": keep frames [N/2, T-(N-1)/2) when T > N */
    int32_t reserved;
} KtfCmvnCfg;

/* mask (B,T) fp32 of kept frames (VAD.call with return_indexes=False). */
int ktf_vad_mask_f32(const float* feats, int64_t B, int64_t T, int32_t D, const KtfVadCfg* cfg, float* mask,
                     void* stream);
/* per-utterance compaction: idx (B,T) int32 = kept frame numbers in order, lens[B] = their count
 * (VAD.call with return_indexes=True gives the same rows as [b, idx[b, j]], j < lens[b]). */
int ktf_vad_index(const float* feats, int64_t B, int64_t T, int32_t D, const KtfVadCfg* cfg, int32_t* idx,
                  int32_t* lens, void* stream);
/* CMVN of each utterance's first lens[b] rows (lens NULL = T rows). x (B,T,D) rows of stride ldx;
 * out rows of stride ldo >= D, columns D..ldo-1 are written as zeros. `work` = B*T*2*D floats.
 * With cfg->valid the output row j holds input frame j + N/2 and out_lens[b] (may be NULL) gets the count. */
int ktf_cmvn_f32(const float* x, int64_t B, int64_t T, int32_t D, int64_t ldx, const int32_t* lens,
                 const KtfCmvnCfg* cfg, float* out, int64_t ldo, int32_t* out_lens, float* work, void* stream);
/* Fused hot path: VAD -> per-utterance compaction -> CMVN (xvector_extractor.py:162-166).
 * out_dtype KTF_F32 or KTF_BF16. idx_work = B*T int32 (on return: the kept frame numbers of each utterance),
 * work = B*T*2*D floats (touched only when the rows do not fit the LDS beside the frame map: ktf_vad_cmvn_plan). Any T < 2^31 / ldo.
 * Batches of fewer than 256 utterances spread each utterance over up to eight workgroups (same values, bit for bit). */
int ktf_vad_cmvn(const float* feats, int64_t B, int64_t T, int32_t D, const KtfVadCfg* vad, const KtfCmvnCfg* cmvn,
                 void* out, int32_t out_dtype, int64_t ldo, int32_t* lens, int32_t* idx_work, float* work,
                 void* stream);

/* Where ktf_vad_cmvn / ktf_cmvn_f32 keep their working data for a given input size: each launcher decides it per call from
 * (B, T, D, ldo) alone, and these two calls report that decision. Host arithmetic only (no GPU call; they work without a GPU).
 * A field of 0 means "not in LDS": the frame map then lives in idx_work, the rows in `work`, the window sums are summed
 * directly and the vote reads the energy out of the feature rows. */
typedef struct KtfVcPlan {
    int64_t pos_ints;      /* LDS ints of the compacted-row -> frame map (ktf_vad_cmvn only)                       */
    int64_t stage_floats;  /* LDS floats of the staged rows                                                         */
    int64_t bs_floats;     /* LDS floats of the sums of 32-row blocks                                               */
    int64_t col_floats;    /* LDS floats of the energy column (ktf_vad_cmvn only)                                   */
    int64_t lds_bytes;     /* dynamic LDS of the launch: the four above plus the kernels' fixed scratch, in bytes   */
    int32_t nsplit;        /* workgroups per utterance (> 1 only in the all-in-LDS form, batches below 256)         */
    int32_t lds_form;      /* 1: the kernel instantiation that addresses the rows as LDS                            */
} KtfVcPlan;
int ktf_vad_cmvn_plan(int64_t B, int64_t T, int32_t D, int64_t ldo, KtfVcPlan* plan);
int ktf_cmvn_plan(int64_t T, int32_t D, int64_t ldo, KtfVcPlan* plan);

/* Per-utterance routing by voiced length (no reference counterpart: the reference runs one utterance at a time in fp32). lens (B) ->
 * lens_main[b] = lens[b] >= min_frames ? lens[b] : 0 and lens_short[b] = 0 < lens[b] < min_frames ? lens[b] : 0. host_flag (optional):
 * two int32 in PINNED, device-visible host memory: [0] = number of short utterances, then [1] = seq (system-scope release), for a host
 * that polls [1] instead of synchronising the stream. */
int ktf_route_short(const int32_t* lens, int64_t B, int32_t min_frames, int32_t* lens_main, int32_t* lens_short, int32_t* host_flag,
                    int32_t seq, void* stream);

/* ------------------------------------------------------------------ TDNN stack (a9, a10)
 * TDNN.call   layers/tdnn/tdnn.py:251-280 (gather im2col + conv2d 1xK + bias + activation)
 * ReLU / BatchNorm (inference affine)  models/kaldi/sequential.py:72-74, layers/normalization/batchnorm.py:78-88
 *
 * y[b, t, u] = post( act( bias[u] + sum_k sum_d x[b, row(t,k), d] * W[u, k*Din_pad + d] ) )
 *   row(t,k)  = clip(start + t*subsampling + ctx[k], 0, len_b-1)  ("SAME": replicate edges; "VALID": no clip needed)
 *   post(v)   = v * scale[u] + shift[u]   when scale != NULL (BatchNorm folded to an affine)
 * x: (B, T, ldx) of x_dtype; W: (units_pad, nctx*Din_pad) row-major of w_dtype, zero padded, where Din_pad is
 * Din rounded up to a multiple of 32 (must be <= ldx; pad columns of x must be finite) and units_pad is units rounded
 * up to 256 (the widest N-tile of the kernels). For KTF_GEMM_BF16X3 `w` holds the hi part and `w_lo` the lo part (both bf16); x is fp32.
 * y: (B, T_out_max, ldy) of y_dtype; out_lens[b] (may be NULL) receives the valid output rows of utterance b.
 */
typedef struct KtfTdnnDesc {
    int32_t units;
    int32_t din;            /* logical input feature dim */
    int32_t din_pad;        /* multiple of 32, <= ldx     */
    int32_t nctx;           /* <= 16 */
    int32_t ctx[16];        /* sorted ascending */
    int32_t subsampling;
    int32_t valid;          /* padding == "VALID" */
    int32_t act;            /* KTF_ACT_* */
    int32_t gemm;           /* KTF_GEMM_* */
    int32_t x_dtype, w_dtype, y_dtype;
    int32_t flags;          /* KTF_TDNN_* bits, 0 = default */
} KtfTdnnDesc;

/* KtfTdnnDesc.flags */
#define KTF_TDNN_REF_TILES 1      /* KTF_GEMM_F32 only: run the register-staged 32x32x2 tile kernels, the bitwise reference the
                                   * LDS-DMA-staged fp32 kernels are tested against (slower; same bits) */
#define KTF_TDNN_DET_STATS 2      /* ktf_tdnn_stats / ktf_tdnn_split_stats only: run-to-run reproducible pooling. Every
                                   * 128-row block of an utterance stores its fp64 column sums in a slot of its own instead
                                   * of adding them with atomics; `sums` is then (B, ktf_stats_slots(T), 2, units), need not
                                   * be zeroed, and is reduced in slot order by ktf_stats_finalize_slots */
#define KTF_TDNN_K_INTERLEAVED 4  /* ktf_tdnn_split / ktf_tdnn_split_stats only: the K axis of W (both planes) is ordered
                                   * (32-feature chunk, context, feature in chunk) instead of (context, feature), i.e. column
                                   * ((d / 32) * nctx + k) * 32 + d % 32 holds W[u, k * Din_pad + d]. The kernel then walks
                                   * the contexts of one feature chunk in consecutive K-steps, so the three (five) reads of an
                                   * activation row piece by a multi-context layer are adjacent in time and hit in L2 instead of
                                   * returning to HBM / MALL 16 K-steps apart */
#define KTF_TDNN_W_TILED 8        /* ktf_tdnn_split / ktf_tdnn_split_stats only: W (both planes) is stored as the kernel's LDS
                                   * stage images instead of row-major: for N-tile nt (256 units) and K-step ks (32 columns of
                                   * the K order in force) one contiguous 16 KiB block at ((nt * ktot / 32 + ks) * 16 KiB),
                                   * holding for row r and 16-byte position q the columns 32 ks + 8 (q ^ ((4 - (r >> 2)) & 3))
                                   * .. + 7 of unit 256 nt + r at byte 64 r + 16 q. A weight DMA instruction then copies 1 KiB of
                                   * consecutive bytes (8 whole cache lines) instead of gathering 16 rows x 64 B */
/* (16, 32 and bits 8..23 were KTF_TDNN_X_CHUNKED / KTF_TDNN_Y_CHUNKED / KTF_TDNN_LO_PREFIX of KTF_GEMM_F16X2) */

#define KTF_TDNN_MX_LOADER (1 << 24)  /* ktf_tdnn_mx / ktf_tdnn_mx_stats only: the loader-wave kernel (csrc/tdnn_mxl.hip: 192 x 256 tiles,
                                   * eight matrix waves + four loader waves). It reads the weight images of its own
                                   * (mx.weight_images_loader; layout below) and, with KTF_TDNN_DET_STATS, writes one slot per 96-row
                                   * block: `sums` is (B, ktf_mx_stats_slots(T, flags), 2, units), reduced with slot_rows =
                                   * ktf_mx_slot_rows(flags) */
/* (1 << 25 was KTF_TDNN_MX_SLAB, the slab form of the 256-row kernel: measured as fast as the gathering kernel, not faster; 1 << 26 was
 * KTF_TDNN_MX_PERSIST, its persistent form -- one workgroup per CU walking its tiles, the operand ring running on across tile boundaries, the
 * previous tile encoded from registers under the next tile's first K-step: correct, 6 % slower. Both live on under tools/mx/experiments/.) */

/* name of the kernel family the calling thread's last ktf_tdnn* / ktf_tdnn_mx* call launched ("" before the first; a static
 * string). For the dispatch tests: which kernel a (gemm mode, layer shape) pair runs on is part of the library's contract. */
const char* ktf_tdnn_last_kernel(void);


/* number of output rows for an utterance with `len` input rows (tdnn.py:224-234) */
int64_t ktf_tdnn_out_len(int64_t len, const KtfTdnnDesc* d);
/* Alignment of y (and y_lo) and ldy, per kernel family of the 16-bit modes (KTF_GEMM_BF16, KTF_GEMM_BF16X3; ktf_tdnn and ktf_tdnn_split*).
 * Always ldy >= units; columns [units, ldy) and rows at or beyond an utterance's output length are not written. Which family runs is
 * decided by the layer (ktf_tdnn_last_kernel names it), and ldy % 4 != 0 sends ktf_tdnn to the 128 x 128 tdnn_bf16_kernel:
 *   tdnn_bf16_kernel<...>  (KTF_GEMM_BF16 on fp32 x; KTF_GEMM_BF16X3 on fp32 x with units <= 128 or ldy % 4 != 0; bf16 x that none of
 *                          the kernels below takes): element stores -- any ldy, y aligned to its element.
 *   tdnn_bf16g_kernel      (bf16 x, units <= 128, din_pad % 64 == 0, ldy % 4 == 0): 16-byte stores of fp32 rows, 8-byte stores of bf16
 *                          rows -- y 16-byte (fp32) / 8-byte (bf16) aligned. REFUSED otherwise.
 *   tdnn_bf16h_kernel      (bf16 x, units > 128, ldy % 4 == 0, K <= 768, ReLU / none): tests at run time -- 16-byte stores where y is
 *                          16-byte aligned and ldy % 4 == 0 (fp32) / ldy % 8 == 0 (bf16), element stores otherwise. Any y aligned to its element.
 *   tdnn_bf16r16_kernel    (the same layers with K > 768): fp32 rows by unconditional 16-byte stores -- y 16-byte aligned, REFUSED
 *                          otherwise; bf16 rows through the run-time test of tdnn_bf16h_kernel -- any y aligned to its element.
 *   tdnn_bf16r_kernel, tdnn_x3r_kernel  (sigmoid / tanh; KTF_GEMM_BF16X3 on fp32 x; units > 128, ldy % 4 == 0): 16-byte stores of fp32
 *                          rows, 8-byte stores of bf16 rows -- y 16-byte (fp32) / 8-byte (bf16) aligned. REFUSED otherwise.
 *   tdnn_x3s_kernel        (ktf_tdnn_split, ktf_tdnn_split_flat: units > 128 and ldy % 4 == 0 or the call is refused): fp32 rows as
 *                          above; the hi / lo planes by 16-byte stores of 8 columns at column offsets that are multiples of 8, from y and
 *                          y_lo 8-byte aligned: with ldy % 8 == 4 every other row's stores are 8-byte aligned only, which the global
 *                          stores of gfx950 accept (they ask for 4). REFUSED: y or y_lo not 16-byte (fp32) / 8-byte (bf16) aligned.
 * The pooled calls (ktf_tdnn_stats, ktf_tdnn_split_stats, ktf_tdnn_split_flat_stats) write doubles into `sums`, 8-byte aligned. */
/* ... for a batch's lengths on the device: out_lens[b] = ktf_tdnn_out_len(lens[b], d). (ktf_tdnn writes them itself; the entry points on
 * the MX planes have no such argument: a VALID-padded or subsampling layer there is followed by this call.) */
int ktf_tdnn_out_lens(const int32_t* lens, int64_t B, const KtfTdnnDesc* d, int32_t* out_lens, void* stream);

int ktf_tdnn(const void* x, int64_t B, int64_t T, int64_t ldx, const int32_t* lens, const KtfTdnnDesc* d,
             const void* w, const void* w_lo, const float* bias, const float* scale, const float* shift,
             void* y, int64_t ldy, int32_t* out_lens, void* stream);

/* ktf_tdnn fused with the reducing StatsPooling that follows it (sequential.py:68-79 order "tdnn5 -> stats"): the layer
 * output is never written; instead sums[b, 0, u] += sum_t y[b,t,u] and sums[b, 1, u] += sum_t y[b,t,u]^2 (fp64, over
 * the valid rows). `sums` (B, 2, units) must be zeroed by the caller before the call (the order of the fp64 atomic adds
 * of an utterance's row blocks is not fixed: results can differ in the last fp64 bits from run to run; see
 * KTF_TDNN_DET_STATS for the reproducible form). Implemented by the 16-bit ring kernels -- KTF_GEMM_BF16 (bf16 x),
 * KTF_GEMM_BF16X3 (fp32 x, w_lo given): units > 128, SAME padding, subsampling 1 -- and by the bf16-pair small
 * tiles (KTF_GEMM_BF16X4: any layer shape; its KTF_TDNN_DET_STATS slots are ktf_tdnn_stats_slots(T, gemm) of
 * ktf_tdnn_slot_rows(gemm) = 64 rows). */
int ktf_tdnn_stats(const void* x, int64_t B, int64_t T, int64_t ldx, const int32_t* lens, const KtfTdnnDesc* d,
                   const void* w, const void* w_lo, const float* bias, const float* scale, const float* shift, double* sums,
                   void* stream);
/* Split-bf16 activations kept as TWO bf16 planes (hi = bf16(v), lo = bf16(v - hi)) instead of fp32: same bytes, but the
 * GEMM stages them as they are and its K-loop carries no fp32 -> (hi, lo) conversion (28 % shorter on MI355X). desc->gemm
 * must be KTF_GEMM_BF16X3 with x_dtype KTF_BF16; units > 128. y_dtype KTF_BF16 with y_lo != NULL writes the output as
 * planes again (the next layer's input); y_dtype KTF_F32 (y_lo NULL) writes plain fp32. ktf_split_bf16 produces the planes
 * of the first layer's input from fp32 rows (columns [D, ld_dst) are zeroed). */
int ktf_tdnn_split(const void* x_hi, const void* x_lo, int64_t B, int64_t T, int64_t ldx, const int32_t* lens,
                   const KtfTdnnDesc* d, const void* w, const void* w_lo, const float* bias, const float* scale,
                   const float* shift, void* y, void* y_lo, int64_t ldy, int32_t* out_lens, void* stream);
/* ktf_tdnn_split with the M-tiles laid over the batch's VALID rows end to end instead of 256-row tiles per utterance (short
 * utterances: a 1.5 s window is 148 rows, 0.58 of a tile). row_starts: (B + 1) int32 on the device, the exclusive prefix sums of the
 * utterance lengths (row_starts[0] = 0, row_starts[B] = the number of valid rows); a row's context offsets clamp against its own
 * utterance as in ktf_tdnn_split, and rows at or beyond an utterance's length are not written. KTF_GEMM_BF16X3 on row-major hi / lo
 * planes, SAME padding, no subsampling, ReLU or no activation, y as for ktf_tdnn_split (planes or fp32); B <= 4095 and
 * B * T * ldx * 2 < 2^32. Results equal ktf_tdnn_split's bit for bit (same operands into the same MFMAs in the same order). */
int ktf_tdnn_split_flat(const void* x_hi, const void* x_lo, int64_t B, int64_t T, int64_t ldx, const int32_t* row_starts, const int32_t* row_map,
                        const KtfTdnnDesc* d, const void* w, const void* w_lo, const float* bias, const float* scale,
                        const float* shift, void* y, void* y_lo, int64_t ldy, void* stream);
/* ktf_tdnn_split_flat fused with the reducing StatsPooling that follows it (ktf_tdnn_split_stats on the flat row tiles: the pooled
 * layer of 1.5 s windows otherwise computes 256-row tiles of 148 rows). `sums`: with KTF_TDNN_DET_STATS (B, ktf_flat_stats_slots(T), 2,
 * units) doubles, not zeroed by the caller: an utterance of len rows that starts at flat row s = row_starts[b] gets one partial sum per
 * 128-row block OF THE FLAT ROW SPACE it touches, in slots 0 .. ((s + len - 1) >> 7) - (s >> 7), and ktf_stats_finalize_flat adds
 * exactly those in slot order: reproducible run to run; the partition of an utterance's rows into partial sums depends on where the
 * batch places it, so its pooled values can differ in the last fp64 bits from batch to batch. Without the flag (B, 2, units), zeroed by
 * the caller, fp64 atomics (finalize with ktf_stats_finalize). */
int64_t ktf_flat_stats_slots(int64_t T);
/* The row table of the flat tiles: 4 int32 per flat row R < ktf_flat_row_map_rows(B, T) = round_up(B * T, 256) -- (output row b * T + t, or
 * -1 at and beyond row_starts[B]; frame t; length of the row's utterance; b). `row_map` of ktf_tdnn_split_flat / _flat_stats: NULL (every
 * workgroup then derives its 256 entries from row_starts: four dependent loads in front of its first DMA, ~3 us per tile) or this table,
 * made once per batch for all its layers -- same rows, same results. */
int64_t ktf_flat_row_map_rows(int64_t B, int64_t T);
int ktf_flat_row_map(const int32_t* row_starts, int64_t B, int64_t T, int32_t* map, void* stream);
int ktf_tdnn_split_flat_stats(const void* x_hi, const void* x_lo, int64_t B, int64_t T, int64_t ldx, const int32_t* row_starts,
                              const int32_t* row_map, const KtfTdnnDesc* d, const void* w, const void* w_lo, const float* bias, const float* scale,
                              const float* shift, double* sums, void* stream);
int ktf_stats_finalize_flat(const double* sums, int64_t slots, const int32_t* row_starts, int64_t T, int64_t B, int32_t D,
                            int32_t include_std, float eps, float* out, int64_t ld_out, void* stream);
int ktf_tdnn_split_stats(const void* x_hi, const void* x_lo, int64_t B, int64_t T, int64_t ldx, const int32_t* lens,
                         const KtfTdnnDesc* d, const void* w, const void* w_lo, const float* bias, const float* scale,
                         const float* shift, double* sums, void* stream);
int ktf_split_bf16(const float* src, int64_t rows, int32_t D, int64_t ld_src, void* hi, void* lo, int64_t ld_dst,
                   void* stream);
/* ... of a ragged batch: src (B, T, ld_src) -> planes (B, T, ld_dst); only the rows t < lens[b] are converted (lens NULL: all T): the
 * consumers clamp their row reads to the utterance, so the rest is never read. Same values as ktf_split_bf16 on the rows it writes. */
int ktf_split_bf16_rows(const float* src, int64_t B, int64_t T, int32_t D, int64_t ld_src, const int32_t* lens, void* hi, void* lo,
                        int64_t ld_dst, void* stream);
/* KTF_GEMM_F16MX (tdnn.py:251-280 + ReLU + BatchNorm, as ktf_tdnn). Activations are FOUR chunk-major planes; with nch = ceil(D / 32)
 * and record r = (b * nch + d / 32) * T + t of element (b, t, d):
 *   xh  : r * 64 B  32 halves, x_h = half(x) (saturating at +-65504), element d % 32
 *   xl4 : r * 16 B  32 e2m1 codes of x - x_h (element e in nibble e: byte e / 2, low nibble first)
 *   x4  : r * 16 B  32 e2m1 codes of x_h
 *   xs  : r * 4 B   uint32: byte 0 = E8M0 scale of the xl4 block, byte 1 = of the x4 block (value = code * 2^(scale - 127));
 *                   scale = floor(log2(block max)) - 2, one more when the maximum would round past 6
 * ktf_mx_planes makes them from fp32 rows (B, T, ld_src) (rows >= lens[b] are left unwritten); the layer itself writes them for
 * the next layer (yh, yl4, y4, ys; D = units), or fp32 rows (yf, ldy), or -- ktf_tdnn_mx_stats -- the pooled sums of
 * ktf_tdnn_stats (same `sums` layouts, KTF_TDNN_DET_STATS honoured). Exactly one output form per call; the others NULL.
 * Weights, for N-tile nt (256 units, zero rows beyond `units`) and K-step ks of the KTF_TDNN_K_INTERLEAVED order, K-steps
 * zero-padded to a multiple of 4 (nkp; a super-step ss = K-steps 4 ss .. 4 ss + 3):
 *   wh : block (nt * nkp + ks) * 16 KiB: the KTF_TDNN_W_TILED image of w_h
 *   wq : block (nt * nkp / 4 + ss) * 48 KiB, with kb = ks % 4, col = unit % 256, record q = kb * 256 + col:
 *          [0, 16 Ki)       q * 16: 32 e2m1 codes of w (K-step ks, unit col)
 *          [16 Ki, 32 Ki)   q * 16: bits 0..127 of the 32 e2m3 codes (6 bits each, element e at bit 6 e) of w - w_h
 *          [32 Ki, 40 Ki)   q * 8 : bits 128..191 of the same
 *          [40 Ki, 44 Ki)   q * 4 : uint32, byte 0 = E8M0 scale of the e2m1 block, byte 1 = of the e2m3 block
 *          [44 Ki, 48 Ki)   unused
 * ReLU or no activation; scale / shift as in ktf_tdnn (NULL when the BatchNorm is folded into the next layer,
 * TDNN.device_weights_mx). VALID padding and subsampling (tdnn.py:224-249) on the 256-row kernel: the output (planes or fp32 rows)
 * then has ktf_tdnn_out_len(T, d) rows per utterance and the valid rows of utterance b are ktf_tdnn_out_len(lens[b], d)
 * (ktf_tdnn_out_lens makes them for the next layer); ktf_tdnn_mx_stats and KTF_TDNN_MX_LOADER take SAME padding without
 * subsampling only. The 256-row kernel keeps a table of its K-steps in LDS: at most 1144 of them (ceil(D / 32) * nctx, padded to a multiple
 * of 4; K <= 36,608); the planes are read through 32-bit buffer offsets: T * din_pad * 2 < 2^31 - 2^20.
 * With KtfTdnnDesc.flags & KTF_TDNN_MX_LOADER the call runs the loader-wave kernel (csrc/tdnn_mxl.hip: 192 x 256 tiles over the flat row
 * space b * T + t, eight matrix + four loader waves) on the SAME activation planes and on weight images of its own
 * (mx.weight_images_loader): every operand fragment is 64 lanes x 16 (8, 4) consecutive bytes, and inside each 32-unit chunk the image
 * columns hold the units in the order (m >> 2) * 8 + (cb & 1) * 4 + (m & 3) for column m of unit block cb:
 *   wh : block (nt * nkp + ks) * 16 KiB: 16 unit-block fragments x 1 KiB, lane (q, m) = halves 8 q .. 8 q + 7 of the block's unit m
 *   wq : block (nt * nkp / 4 + ss) * 44 KiB = two halves of 22 KiB (unit blocks with (cb >> 1) & 1 == h, in the order
 *        2 (cb >> 2) + (cb & 1)): e2m1 codes 8 x 1 KiB | e2m3 bits 0..127 8 x 1 KiB | e2m3 bits 128..191 8 x 512 B | scale words
 *        8 x 256 B, lane (kb, m) = K block kb of the super-step, unit m of the block.
 * It needs B * T < 2^31 and B * T * ceil(D / 32) < 2^32, writes planes only without scale / shift, and its KTF_TDNN_DET_STATS slots are
 * 96 rows each (ktf_mx_stats_slots / ktf_mx_slot_rows). */
int ktf_mx_planes(const float* src, int64_t B, int64_t T, int32_t D, int64_t ld_src, const int32_t* lens, void* xh, void* xl4,
                  void* x4, void* xs, void* stream);
int ktf_tdnn_mx(const void* xh, const void* xl4, const void* x4, const void* xs, int64_t B, int64_t T, const int32_t* lens,
                const KtfTdnnDesc* d, const void* wh, const void* wq, const float* bias, const float* scale, const float* shift,
                void* yh, void* yl4, void* y4, void* ys, float* yf, int64_t ldy, void* stream);
/* ktf_tdnn_mx with a plane output on FLAT ROW TILES: the 256-row M-tiles cover the batch's valid rows laid end to end (row_starts, row_map:
 * ktf_flat_row_map; as ktf_tdnn_split_flat) instead of ceil(T / 256) tiles per utterance -- 998-frame utterances fill 3.9 of their 4 tiles, a
 * batch the VAD left ragged fewer. SAME padding, no subsampling; B <= 4095, B * T * din_pad * 2 < 2^32. The planes equal ktf_tdnn_mx's bit for
 * bit (same operands into the same MFMAs in the same order); rows at and beyond an utterance's length are not written. */
int ktf_tdnn_mx_flat(const void* xh, const void* xl4, const void* x4, const void* xs, int64_t B, int64_t T, const int32_t* row_starts,
                     const int32_t* row_map, const KtfTdnnDesc* d, const void* wh, const void* wq, const float* bias, const float* scale,
                     const float* shift, void* yh, void* yl4, void* y4, void* ys, void* stream);
/* ... and ktf_tdnn_mx_stats on flat row tiles: `sums` as for ktf_tdnn_split_flat_stats ((B, ktf_flat_stats_slots(T), 2, units) with
 * KTF_TDNN_DET_STATS, reduced by ktf_stats_finalize_flat; else (B, 2, units), zeroed by the caller) */
int ktf_tdnn_mx_flat_stats(const void* xh, const void* xl4, const void* x4, const void* xs, int64_t B, int64_t T, const int32_t* row_starts,
                           const int32_t* row_map, const KtfTdnnDesc* d, const void* wh, const void* wq, const float* bias, const float* scale,
                           const float* shift, double* sums, void* stream);
int ktf_tdnn_mx_stats(const void* xh, const void* xl4, const void* x4, const void* xs, int64_t B, int64_t T, const int32_t* lens,
                      const KtfTdnnDesc* d, const void* wh, const void* wq, const float* bias, const float* scale,
                      const float* shift, double* sums, void* stream);
/* finishes the fused pooling: out[b, c] = sums[b,0,c]/n_b, out[b, D+c] = sqrt(max(sums[b,1,c]/n_b - mean^2, 0) + eps)
 * with n_b = lens[b] (or T when lens is NULL); stats_pooling.py:231-240. */
int ktf_stats_finalize(const double* sums, const int32_t* lens, int64_t T, int64_t B, int32_t D, int32_t include_std,
                       float eps, float* out, int64_t ld_out, void* stream);
/* KTF_TDNN_DET_STATS layout: number of 128-row slots of an utterance of T rows (2 * ceil(T / 256): whole 256-row tiles),
 * and the finalize that adds the slots 0 .. ceil(n_b / slot_rows) - 1 of sums (B, slots, 2, D) in that order before forming
 * mean / std as above (slot_rows = 128 for ktf_tdnn_stats / ktf_tdnn_split_stats, ktf_mx_slot_rows(flags) for ktf_tdnn_mx_stats). */
int64_t ktf_stats_slots(int64_t T);
/* ... of ktf_tdnn_stats for a GEMM mode: KTF_GEMM_BF16X4 (x, w of KTF_BF16P; the small-tile kernel) writes one slot per 64-row tile
 * (ceil(T / 64) slots of ktf_tdnn_slot_rows(gemm) = 64 rows), every other mode ktf_stats_slots(T) slots of 128 rows */
int64_t ktf_tdnn_stats_slots(int64_t T, int32_t gemm);
int32_t ktf_tdnn_slot_rows(int32_t gemm);
/* ... for ktf_tdnn_mx_stats, whose slot geometry depends on the kernel (KtfTdnnDesc.flags & KTF_TDNN_MX_LOADER: 96-row slots, two per
 * 192-row tile; else as ktf_stats_slots) */
int64_t ktf_mx_stats_slots(int64_t T, int32_t flags);
int32_t ktf_mx_slot_rows(int32_t flags);
int ktf_stats_finalize_slots(const double* sums, int64_t slots, int32_t slot_rows, const int32_t* lens, int64_t T, int64_t B, int32_t D,
                             int32_t include_std, float eps, float* out, int64_t ld_out, void* stream);

/* in place over the rows t < lens[b] of y (B, T, ld) fp32 (lens NULL: all T rows): y = act(y) * scale + shift per column, any KTF_ACT_*
 * (KTF_ACT_SOFTMAX: over the D units of each row, then the affine); scale / shift may be NULL (both or neither). The pass ktf_tdnn
 * appends for activations its epilogues do not fuse; rows at and beyond lens[b] are not touched. */
int ktf_activation_f32(float* y, int64_t B, int64_t T, int32_t D, int64_t ld, const int32_t* lens, int32_t act, const float* scale,
                       const float* shift, void* stream);

/* elementwise y = act(x) * scale + shift per column (stand-alone ReLU / BatchNorm layers; any KTF_ACT_* but KTF_ACT_SOFTMAX);
 * scale/shift may be NULL */
int ktf_affine_act_f32(const float* x, int64_t rows, int32_t D, int32_t act, const float* scale, const float* shift,
                       float* y, void* stream);
/* dtype conversion / column padding: dst (rows, ld_dst) <- src (rows, D) with zero fill of the pad columns */
int ktf_convert_pad(const void* src, int32_t src_dtype, int64_t rows, int32_t D, int64_t ld_src, void* dst,
                    int32_t dst_dtype, int64_t ld_dst, void* stream);

/* ------------------------------------------------------------------ statistics pooling (a11)
 * StatsPooling.computeStatsAcrossAll  layers/stats/stats_pooling.py:211-240
 * out (B, ld_out) fp32, columns [0,D) = mean_t and [D,2D) = sqrt(max(E[x^2]-mean^2,0)+eps) over rows
 * 0, input_period, ... < lens[b]; columns beyond are left untouched. */
int ktf_stats_pool(const void* x, int32_t x_dtype, int64_t B, int64_t T, int32_t D, int64_t ldx,
                   const int32_t* lens, int32_t input_period, int32_t include_std, float eps, float* out,
                   int64_t ld_out, void* stream);
/* StatsPooling.computeStatsAcrossWindows  layers/stats/stats_pooling.py:179-209,242-295 (fp32).
 * Output row j covers input rows start + j*output_period + {left..min(right, T-1) step input_period} inside [0,T). */
int ktf_stats_pool_windowed_f32(const float* x, int64_t B, int64_t T, int32_t D, int32_t left, int32_t right,
                                int32_t input_period, int32_t output_period, int32_t start, int64_t T_out,
                                int32_t include_std, float eps, float* out, void* stream);

/* The tail of the extractor in ONE launch: pooled statistics -> the affine after the pooling (tdnn6; sequential.py:68-79, W
 * (units, ldw) fp32 row-major, rows 16-byte aligned, ldw a multiple of 4 >= in_dim = (include_std ? 2 : 1) * D) -> x - mean -> LDA
 * A (units, out_dim) + off -> length normalisation (xvector_extractor.py:174-184). Input: fp32 pooled rows (`pooled`, ld_pooled;
 * stats_pooling.py:231-240 already applied) OR the fp64 sums of ktf_tdnn_stats / ktf_tdnn_mx_stats (`sums`, `slots`, `slot_rows` as for
 * ktf_stats_finalize[_slots]; the finalize happens in the kernel). Workspace: `partial` (B, 64, out_dim) fp32, `counters` (B)
 * uint32 ZEROED once by the caller (the kernel leaves them zero). `h_out` (B, units), optional: the affine's output.
 * Grid = 64 unit slices x ceil(B / group) utterance groups: a workgroup keeps its slice of W in registers and walks `group`
 * utterances (1 for a single utterance: 64 CUs share the 6 MB of W; ~32 for a large batch: W is read once per group). units <=
 * 512, in_dim <= 3072. Sums in a fixed order that does not depend on B or group: reproducible, batch == single bit for bit. */
int ktf_xvec_tail_f32(const float* pooled, int64_t ld_pooled, const double* sums, int64_t slots, int32_t slot_rows, const int32_t* lens, int64_t T,
                      int64_t B, int32_t D, int32_t include_std, float eps, const float* W, int64_t ldw, const float* bias,
                      int32_t units, const float* mean, const float* A, const float* off, int32_t out_dim, float* partial,
                      uint32_t* counters, float* y, float* h_out, int32_t group, int32_t flags, void* stream);
#define KTF_TAIL_SKIP_EMPTY 1     /* ktf_xvec_tail_f32 flags: utterances with lens[b] == 0 are skipped and their rows of y left as they are
                                   * (the second, tighter pass over the short utterances of a batch: XvectorExtractor.route_short_utterances) */
/* ------------------------------------------------------------------ x-vector post-processing (a12)
 * models/kaldi/xvector_extractor.py:174-184: y = (x - mean) @ A + off ; y *= sqrt(out)/||y||_2
 * x (B, in) fp32, A (in, out) row-major, off (out). */
int ktf_xvec_post_f32(const float* x, int64_t B, int32_t in_dim, int32_t out_dim, const float* mean, const float* A,
                      const float* off, float* y, void* stream);

/* ------------------------------------------------------------------ PLDA (a16)
 * PLDA.call  layers/plda/plda.py:247-263. fp64 (reference default) and fp32 variants.
 * x (B, dim); A (dim, dim) row-major; offset = -A*mean (dim); psi (dim).
 * transformed (B, dim); scores (B, B) with scores[i, j] = LLR(x_i | class of x_j). */
int ktf_plda_f64(const double* x, int64_t B, int32_t dim, const double* A, const double* offset, const double* psi,
                 int32_t normalize_length, int32_t simple_length_norm, double* transformed, double* scores,
                 void* stream);
int ktf_plda_f32(const float* x, int64_t B, int32_t dim, const float* A, const float* offset, const float* psi,
                 int32_t normalize_length, int32_t simple_length_norm, float* transformed, float* scores,
                 void* stream);

/* Rectangular trial blocks (plda.py:198-245 logLikelihoodRatio on two sets; the reference only scores a batch against
 * itself): scores[i, j] (N x M, row-major) = LLR(test_tr[i] | class of enroll_tr[j]); both inputs are TRANSFORMED vectors
 * (ktf_plda_* with scores == NULL produces them). Lets a large trial matrix be cut into row blocks, one per GPU. */
int ktf_plda_score_f64(const double* test_tr, int64_t N, const double* enroll_tr, int64_t M, int32_t dim,
                       const double* psi, double* scores, void* stream);
int ktf_plda_score_f32(const float* test_tr, int64_t N, const float* enroll_tr, int64_t M, int32_t dim, const float* psi,
                       float* scores, void* stream);

/* ------------------------------------------------------------------ speaker verification
 * Kaldi's verification recipes (sitw, sre16 v2, voxceleb): ivector-mean over spk2utt, then ivector-subtract-global-mean,
 * transform-vec and ivector-normalize-length (ktf_xvec_post_f32), then ivector-plda-scoring --num-utts over a trial list.
 *
 * ivector-mean: speaker s owns utts[offsets[s] .. offsets[s + 1]) (a CSR map: offsets S + 1 and utts device int32), rows of raw
 * (U, D) fp32. means[s] (S, D) fp32 = the fp64 sum of its rows in list order, divided by the count and rounded once to fp32;
 * num_utts[s] (S, device int32) = the count. A speaker with an empty or out-of-range list, or naming a row outside [0, U), gets a
 * NaN row and num_utts 0 (callers check the map on the host: this only keeps the kernel inside its arrays). n_idx: length of utts. */
int ktf_spk_mean_f32(const float* raw, int64_t U, int32_t D, const int32_t* offsets, int64_t S, const int32_t* utts, int64_t n_idx,
                     float* means, int32_t* num_utts, void* stream);

/* PLDA::TransformIvector(config, ivector, num_examples, ...) (plda.py:163-196 transformVector(inputs, num_examples)): ktf_plda_*'s
 * transform with a count per row, num_examples (B, device, the dtype of x). The length normalisation factor becomes
 * sqrt(dim / sum_d y_d^2 / (psi_d + 1 / n)); simple_length_norm ignores n. With every count 1: ktf_plda_*'s transformed rows, bit
 * for bit. Counts must be > 0 (not checked on the device). */
int ktf_plda_transform_n_f64(const double* x, int64_t B, int32_t dim, const double* A, const double* offset, const double* psi,
                             const double* num_examples, int32_t normalize_length, int32_t simple_length_norm, double* transformed,
                             void* stream);
int ktf_plda_transform_n_f32(const float* x, int64_t B, int32_t dim, const float* A, const float* offset, const float* psi,
                             const float* num_examples, int32_t normalize_length, int32_t simple_length_norm, float* transformed,
                             void* stream);
/* PLDA::LogLikelihoodRatio(transformed_enroll, n, transformed_test) (plda.py:198-245 logLikelihoodRatio(inputs, num_examples)) on
 * the rectangular block of ktf_plda_score_*, class j (enroll column) averaging enroll_num_examples[j] = n_j examples (M, device, the
 * dtype): mean_jd = n_j psi_d / (n_j psi_d + 1) e_jd, var_jd = 1 + psi_d / (n_j psi_d + 1); the no-class term keeps 1 + psi. With
 * every count 1: ktf_plda_score_*'s scores, bit for bit. */
int ktf_plda_score_n_f64(const double* test_tr, int64_t N, const double* enroll_tr, int64_t M, int32_t dim, const double* psi,
                         const double* enroll_num_examples, double* scores, void* stream);
int ktf_plda_score_n_f32(const float* test_tr, int64_t N, const float* enroll_tr, int64_t M, int32_t dim, const float* psi,
                         const float* enroll_num_examples, float* scores, void* stream);
/* ivector-plda-scoring --num-utts over a trial list: scores[t] = the LLR of ktf_plda_score_n_* for the pair trials[2t] = class j
 * (row of enroll_tr, 0 <= j < M), trials[2t + 1] = test i (row of test_tr, 0 <= i < N); trials: T pairs of device int32. A pair
 * outside those ranges scores NaN (nothing outside the arrays is read). A score's bits depend on its two vectors, psi and n_j only,
 * not on its position in the list or the order of the list. workspace: a device buffer of at least
 * ktf_plda_trials_workspace_bytes(N, M, dim, sizeof dtype) bytes (returns a negative KTF_* code on bad arguments). */
int64_t ktf_plda_trials_workspace_bytes(int64_t N, int64_t M, int32_t dim, int32_t dtype_bytes);
int ktf_plda_trials_f64(const double* test_tr, int64_t N, const double* enroll_tr, int64_t M, int32_t dim, const double* psi,
                        const double* enroll_num_examples, const int32_t* trials, int64_t T, double* scores, void* workspace,
                        size_t workspace_bytes, void* stream);
int ktf_plda_trials_f32(const float* test_tr, int64_t N, const float* enroll_tr, int64_t M, int32_t dim, const float* psi,
                        const float* enroll_num_examples, const int32_t* trials, int64_t T, float* scores, void* workspace,
                        size_t workspace_bytes, void* stream);
/* Score normalisation against a cohort (S-norm; adaptive S-norm with top_n, Matejka et al. 2017): mean[r] and std[r] of the top_n
 * largest entries of row r of x (R, C), row stride ld >= C elements; mean and std (R) fp64 on the device whatever the dtype of x.
 * The selected multiset is the top_n largest values, with as many copies of the top_n-th largest as make the count top_n (unique
 * whatever the ties); top_n >= C (INT32_MAX: "all") selects the whole row. mean = sum / top_n; std = sqrt(sum (x - mean)^2 / top_n),
 * the population form, centred in a second pass; an all-tied selection has std exactly 0. One workgroup per row, radix select on
 * order-preserving integer keys, no floating-point atomics: a row's result depends on its values in order, C, top_n and the dtype
 * only (not on R, the row's index, ld or the run). Rows are assumed free of NaN (with one, the row's result is unspecified; nothing
 * outside the arrays is touched). R == 0 launches nothing; C < 1 and top_n < 1 are refused. */
int ktf_topn_stats_f64(const double* x, int64_t R, int64_t C, int64_t ld, int32_t top_n, double* mean, double* std, void* stream);
int ktf_topn_stats_f32(const float* x, int64_t R, int64_t C, int64_t ld, int32_t top_n, double* mean, double* std, void* stream);
/* ktf_topn_stats_* of the PLDA scores of R transformed vectors against a cohort of C transformed vectors, the (R, C) block formed in
 * `workspace` (at least ktf_plda_cohort_workspace_bytes(R, C, dim, sizeof dtype) = R * C * sizeof dtype bytes, 256-byte aligned; a
 * negative KTF_* code on bad arguments) and ranked on the same stream: no host reads, no allocations; the caller bounds the memory
 * by the number of rows it passes per call. role 0 (test side, T-norm): row r is a test vector, the cohort vectors are the classes,
 * counts (C) their examples: x[r][c] = ktf_plda_score_n_*(rows, cohort, counts)[r][c]. role 1 (enroll side, Z-norm): row r is a
 * class, counts (R) the rows' examples, the cohort vectors are the tests: x[r][c] = ktf_plda_score_n_*(cohort, rows, counts)[c][r].
 * counts NULL: every count 1 (ktf_plda_score_*). Every ranked score has the bits those entry points give its pair. */
int64_t ktf_plda_cohort_workspace_bytes(int64_t R, int64_t C, int32_t dim, int32_t dtype_bytes);
int ktf_plda_cohort_stats_f64(const double* rows_tr, int64_t R, const double* cohort_tr, int64_t C, int32_t dim, const double* psi,
                              const double* counts, int32_t role, int32_t top_n, double* mean, double* std, void* workspace,
                              size_t workspace_bytes, void* stream);
int ktf_plda_cohort_stats_f32(const float* rows_tr, int64_t R, const float* cohort_tr, int64_t C, int32_t dim, const float* psi,
                              const float* counts, int32_t role, int32_t top_n, double* mean, double* std, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ dense PLDA scoring with conversation-dependent PCA
 * Kaldi `ivector-plda-scoring-dense` (the scoring stage of x-vector diarization); the reference ships its golden table
 * (testdata/plda/plda_scores.py, RefPldaScores.ark, --target-energy 0.1) and no implementation. For every recording r of a call
 * (rows x[first_r .. first_r + lengths[r]), the vectors PLDA.call takes):
 *   1. m = mean, Sigma = centred covariance, in fp64 (the n x n Gram matrix when n <= dim: the same non-zero spectrum);
 *   2. its eigenvalues lam (descending) and eigenvectors: batched cyclic Jacobi, at most KTF_PLDA_DENSE_MAX_SWEEPS sweeps;
 *   3. d as EstPca chooses it, off-by-one included: tot = sum lam; e = 0; d = 1; while (e / tot <= target) e += lam[d++ - 1];
 *      then clamped to the numerical rank, the count of lam > floor * lam[0] (floor KTF_PLDA_DENSE_RANK_FLOOR_F64 / _F32 by the
 *      dtype of x; rank 0 when lam[0] <= floor * the mean squared row norm, i.e. rows equal up to rounding) -- this project's only deviation from Kaldi, whose SVD fills directions of zero variance arbitrarily (with
 *      n = 2 Kaldi's d is always 2, the rank 1). Rank 0 (n = 1, or all rows equal): the recording is scored without PCA;
 *   4. M = the first d eigenvectors as rows; Plda::ApplyTransform(M) in fp64 gives the model (T', offset', psi') of dimension d;
 *   5. every row x: y = T' M x + offset', length norm (normalize_length / simple_length_norm) in dimension d, num_examples = 1;
 *   6. scores_r[i][j] = LLR(y_i | class of y_j), the formula of ktf_plda_*, with psi'.
 * Steps 1-4 are fp64 whatever the dtype; 5 is fp64 rounded to the dtype; 6 runs in the dtype.
 * target_energy == KTF_PLDA_DENSE_NO_PCA: no PCA, every block is ktf_plda_*'s scores of the recording's rows, bit for bit. Otherwise
 * 0 <= target_energy < 1.
 * x (S, dim) with 1 <= dim <= KTF_PLDA_DENSE_MAX_DIM; lengths: HOST array of R >= 1 counts, each >= 1, summing to S (argument
 * checks and sizes); lengths_dev: the same R values on the device (the per-recording table is built from them on the device).
 * A, offset, psi: the model as ktf_plda_* takes it; mean64 (dim), Tinv64 (dim x dim, the inverse of A), psi64 (dim): the model in
 * fp64 (not read without PCA). Out: scores = the R blocks lengths[r]^2, row-major, one after another; dims (R, device int32) =
 * the retained d per recording, 0 where it was scored without PCA; *status (device int32) = the number of eigenproblems that did
 * not converge or subspaces whose within-class covariance was not positive definite: nonzero means the scores are not to be
 * used. Reading it is the caller's (one word at the end of the call). workspace: a device buffer of at least
 * ktf_plda_dense_workspace_bytes() bytes (returns a negative KTF_* code on bad arguments). Nothing is copied to or from the host. */
#define KTF_PLDA_DENSE_NO_PCA (-1.0)
#define KTF_PLDA_DENSE_MAX_DIM 512
#define KTF_PLDA_DENSE_MAX_SWEEPS 30
#define KTF_PLDA_DENSE_JACOBI_LDS 128            /* eigenproblems up to this size run in LDS (fp64), larger ones in the workspace */
#define KTF_PLDA_DENSE_RANK_FLOOR_F64 1e-10
#define KTF_PLDA_DENSE_RANK_FLOOR_F32 1e-6       /* fp32 inputs carry ~6e-8 relative rounding: a direction of relative variance
                                                  * 1e-6 (amplitude 1e-3) is projected with >= 1e-4 relative error */
int64_t ktf_plda_dense_workspace_bytes(const int32_t* lengths, int32_t R, int32_t dim, double target_energy);
int ktf_plda_dense_f64(const double* x, int64_t S, int32_t dim, const int32_t* lengths, const int32_t* lengths_dev, int32_t R,
                       double target_energy, const double* A, const double* offset, const double* psi, const double* mean64,
                       const double* Tinv64, const double* psi64, int32_t normalize_length, int32_t simple_length_norm,
                       double* scores, int32_t* dims, void* workspace, size_t workspace_bytes, int32_t* status, void* stream);
int ktf_plda_dense_f32(const float* x, int64_t S, int32_t dim, const int32_t* lengths, const int32_t* lengths_dev, int32_t R,
                       double target_energy, const float* A, const float* offset, const float* psi, const double* mean64,
                       const double* Tinv64, const double* psi64, int32_t normalize_length, int32_t simple_length_norm,
                       float* scores, int32_t* dims, void* workspace, size_t workspace_bytes, int32_t* status, void* stream);

/* ------------------------------------------------------------------ agglomerative clustering of dense PLDA scores
 * Kaldi `agglomerative-cluster` (AgglomerativeClusterer, single pass), the stage of x-vector diarization after
 * ktf_plda_dense_*. For every recording r (its n = lengths[r] rows): costs C = read_costs ? scores : -scores, of which only the
 * strict upper triangle (i < j) is read (the diagonal and the lower triangle may hold anything, NaN included). Every row starts
 * as its own cluster (ids 1 .. n, size 1); Sigma(a, b) = the sum of the costs between two clusters, avg = Sigma / dtype(size_a *
 * size_b). While more than min_clusters clusters are active, the eligible pair (avg <= threshold and size_a + size_b <=
 * ceil(fp32(n) * fp32(max_spk_fraction))) with the smallest (avg, lo_id, hi_id) is merged into a cluster with the next id
 * (n + 1, n + 2, ...), Sigma(k, new) = Sigma(k, a) + Sigma(k, b). Labels 1 .. K go to the final clusters in ascending id.
 * All arithmetic is in the dtype of scores (fp32: Kaldi's BaseFloat), threshold is rounded to it.
 * scores: the R blocks lengths[r]^2, row-major, one after another (ktf_plda_dense_*'s output). lengths: HOST array of R >= 1
 * counts, each in 1 .. KTF_AHC_MAX_N (argument checks and sizes); lengths_dev: the same R values on the device. min_clusters_dev:
 * R device int32 (NULL: 1 for every recording). 0 < max_spk_fraction <= 1. Out: labels (S = sum of lengths, device int32, one
 * per row), num_clusters (R, device int32). workspace: a device buffer of at least ktf_ahc_workspace_bytes() bytes (returns a
 * negative KTF_* code on bad arguments; dtype_bytes 4 or 8). Nothing is copied to or from the host. */
#define KTF_AHC_MAX_N 32767                     /* Kaldi's default first-pass-max-utterances: below it Kaldi runs one pass */
#define KTF_AHC_LDS_SLOTS 5120                  /* recordings up to this size keep the merge loop's per-slot state in LDS */
int64_t ktf_ahc_workspace_bytes(const int32_t* lengths, int32_t R, int32_t dtype_bytes);
int ktf_ahc_f64(const double* scores, const int32_t* lengths, const int32_t* lengths_dev, int32_t R, int32_t read_costs,
                double threshold, const int32_t* min_clusters_dev, double max_spk_fraction, int32_t* labels, int32_t* num_clusters,
                void* workspace, size_t workspace_bytes, void* stream);
int ktf_ahc_f32(const float* scores, const int32_t* lengths, const int32_t* lengths_dev, int32_t R, int32_t read_costs,
                double threshold, const int32_t* min_clusters_dev, double max_spk_fraction, int32_t* labels, int32_t* num_clusters,
                void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ sliding-window x-vectors of diarization
 * The project's restatement of the front half of Kaldi's diarization recipe (speech segments -> per-segment sliding CMN ->
 * overlapping subsegments). R recordings' frames lie end to end in one frame stream: recording r owns frames [offsets[r],
 * offsets[r + 1]) (offsets: R + 1 device int32, offsets[0] = 0), frames[r] = offsets[r + 1] - offsets[r] on the HOST (argument checks).
 * seg_work / win_work: 2 * F device int32 each (F = sum of frames): recording r's (start, end) pairs at slot offsets[r]. counts: 2R
 * device int32, segments per recording then windows per recording. Frame numbers are relative to the recording, ends exclusive.
 *
 * Segments of the energy VAD: the threshold and the vote of ktf_vad_cmvn (VAD.call, layers/dsp/vad.py:156-203) over each
 * recording's own frames[r] frames of mfcc (F, D); a segment is a maximal run of voiced frames. Writes seg_work and counts[0, R). */
int ktf_diar_segments(const float* mfcc, int32_t D, const int32_t* frames, const int32_t* offsets, int32_t R, const KtfVadCfg* vad,
                      int32_t* seg_work, int32_t* counts, void* stream);
/* Windows of the counts[r] segments of seg_work: for a segment [s, e) of L frames, [a, a + W) while L > W + M (a += P, L -= P), then
 * [a, e): 1 + max(0, ceil((L - W - M) / P)) windows. Needs W > 0, 0 < P <= W, M >= 0. Writes win_work and counts[R, 2R). */
int ktf_diar_windows(const int32_t* seg_work, const int32_t* frames, const int32_t* offsets, int32_t R, int32_t W, int32_t P, int32_t M,
                     int32_t* win_work, int32_t* counts, void* stream);
/* The compact tables: segments (G, 3) and windows (S, 3) device int32 rows (recording, start, end), recording 0's first; G and S are
 * the sums of the counts (the host reads them in between). */
int ktf_diar_compact(const int32_t* seg_work, const int32_t* win_work, const int32_t* counts, const int32_t* frames, const int32_t* offsets,
                     int32_t R, int64_t G, int64_t S, int32_t* segments, int32_t* windows, void* stream);
/* CMN of every segment's rows of mfcc (F, D) as one utterance: the values of ktf_cmvn_f32 (CMVN.call, layers/normalization/
 * cmvn.py:186-250) on those rows alone, bit for bit, written to out (F, D) at the same frames (other rows untouched). SAME padding
 * only. work: F * D floats (segments too long for the LDS). */
int ktf_diar_segment_cmn(const float* mfcc, int32_t D, const int32_t* frames, const int32_t* offsets, int32_t R, const int32_t* segments,
                         int64_t G, const KtfCmvnCfg* cmvn, float* out, float* work, void* stream);
/* Windows [w0, w0 + n) of the table (S, 3) -> out (n, Tw, ldo) of out_dtype (KTF_F32 / KTF_BF16, round to nearest even): row t < len
 * of window i is row start + t of cmn (F, D), every other element zero; lens[i] = len = min(end - start, Tw). ldo a multiple of 8, cmn
 * and out 16-byte aligned, cmn allocated with 4 floats beyond F * D (16-byte loads). */
int ktf_diar_gather(const float* cmn, int32_t D, const int32_t* frames, const int32_t* offsets, int32_t R, const int32_t* windows, int64_t S,
                    int64_t w0, int64_t n, int32_t Tw, void* out, int32_t out_dtype, int32_t ldo, int32_t* lens, void* stream);

/* ------------------------------------------------------------------ i-vector extraction
 * Kaldi's sid/extract_ivectors.sh core: gmm-global-get-post | scale-post | ivector-extract. The reference ships the extractor's
 * reader (io/kaldi/ivector_extractor_reader.py) and no extraction. Frames of all utterances lie end to end in x (F, D) fp32, row
 * stride ldx; utterance b owns rows [offsets[b], offsets[b + 1]) (offsets: B + 1 device int32).
 *
 * gmm-global-get-post --n=num_gselect --min-post=min_post (DiagGmm::LogLikelihoods, then VectorToPosteriorEntry): per frame the
 * log-likelihoods l_i = gconst_i + x . mi_i - x^2 . iv_i / 2 as one fp32 GEMM of [x, x^2] against W (2D x I, row-major: row d is
 * means_invvars[:, d], row D + d is -inv_vars[:, d] / 2), never written out. Kept: the min(num_gselect, I) largest l (ties: the
 * lower index); p = exp(l - max) over the kept set; the smallest dropped while p < min_post * (sum of the kept p), at least one
 * kept; renormalised. gauss / post: (F, num_gselect) device int32 / fp32, sorted by posterior, unused slots (-1, 0). */
#define KTF_IVECTOR_MAX_FEAT_DIM 128
#define KTF_IVECTOR_MAX_GAUSS 8192
#define KTF_IVECTOR_MAX_GSELECT 64
#define KTF_IVECTOR_MAX_DIM 1024
int ktf_ivector_post_f32(const float* x, int64_t F, int32_t D, int64_t ldx, const float* W, const float* gconst, int32_t I,
                         int32_t num_gselect, float min_post, int32_t* gauss, float* post, void* stream);
/* scale-post posterior_scale, then ivector-extract --acoustic-weight --max-count (IvectorExtractorUtteranceStats::AccStats without
 * second-order stats, IvectorExtractor::GetIvectorDistMean / GetIvectorDistPrior, the solve, ivector(0) -= prior_offset):
 *   p' = fp32(p * posterior_scale); t = acoustic_weight * sum p' (fp64); scale = fp32(acoustic_weight * (max_count > 0 && t > max_count
 *   ? max_count / t : 1)); gamma_i = sum_t fp32(p' * scale), F_i = sum_t fp32(p' * scale) x_t (fp64, each Gaussian's sum in frame
 *   order); linear = sum_i sigma_inv_M_i^T F_i + prior_offset e0; Q = I + sum_i gamma_i U_i; ivector = Q^-1 linear (Cholesky, fp64),
 *   ivector(0) -= prior_offset. An utterance with no frames gets zeros.
 * gauss / post: (F, n) as ktf_ivector_post_f32 writes them (slots with an index outside [0, I) are skipped). sigma_inv_M: (I * D, S)
 * fp64 row-major (SigmaInv_i M_i stacked), U: (I, S(S+1)/2) fp64, the lower triangle of M_i^T SigmaInv_i M_i row by row.
 * ivectors: (B, S) fp32 (out_dtype_bytes 4) or fp64 (8). workspace: 256-byte aligned, at least
 * ktf_ivector_workspace_bytes(B, I, D, S) bytes (returns a negative KTF_* code on bad arguments). An utterance's bits depend on its
 * own frames alone, not on B or its position. */
int64_t ktf_ivector_workspace_bytes(int32_t B, int32_t I, int32_t D, int32_t S);
int ktf_ivector_extract(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* offsets, int32_t B, const int32_t* gauss,
                        const float* post, int32_t n, float posterior_scale, float acoustic_weight, float max_count,
                        const double* sigma_inv_M, const double* U, int32_t I, int32_t S, double prior_offset, void* ivectors,
                        int32_t out_dtype_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* ------------------------------------------------------------------ i-vector extractor training statistics
 * Kaldi's `ivector-extractor-acc-stats` (IvectorExtractorStats::AccStatsForUtterance, update_variances, no ivector-dependent
 * weights) for the B utterances of a call, added in place to fp64 device accumulators. Inputs as ktf_ivector_extract (there is no
 * acoustic_weight and no max_count). Per utterance with at least one frame: p' = fp32(p * posterior_scale); gamma_u, F_u;
 * lin = sum_i sigma_inv_M_i^T F_ui + prior_offset e0; Q = I + sum_i gamma_ui U_i = L L^T; C_u = Q^-1; w_u = C_u lin (the offset is
 * NOT subtracted); W_u = C_u + w_u w_u^T. Then
 *   gamma (I) += gamma_u;  Y (I * D, S) += F_u w_u^T;  R (I, P) += gamma_u W_u (packed lower triangles, P = S(S+1)/2);
 *   ivector_sum (S) += w_u;  ivector_scatter (P) += W_u;  totals[0] += 1;
 *   totals[1] += lin^T w_u / 2 - sum_j log L_jj - prior_offset^2 / 2   (the utterance's term of the marginal log-likelihood).
 * An utterance with no frames adds nothing and is not counted. The sums over the utterances of a call run in ascending utterance
 * order inside every element (ktf_atb_f64), so the same sequence of calls gives the same bits. workspace: 256-byte aligned, at
 * least ktf_ivector_train_workspace_bytes(B, I, D, S) bytes: the extraction workspace plus (B, P + S + 2) fp64. */
int64_t ktf_ivector_train_workspace_bytes(int32_t B, int32_t I, int32_t D, int32_t S);
int ktf_ivector_acc_stats(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* offsets, int32_t B, const int32_t* gauss,
                          const float* post, int32_t n, float posterior_scale, const double* sigma_inv_M, const double* U, int32_t I,
                          int32_t S, double prior_offset, double* gamma, double* Y, double* R, double* ivector_sum,
                          double* ivector_scatter, double* totals, void* workspace, size_t workspace_bytes, void* stream);
/* Second-order statistics: Ssec (I, D, D) fp64 += sum over the frames t and slots of x with gauss = i of p' x_t x_t^T. The (frame,
 * slot) pairs are bucketed by Gaussian with a stable counting sort and every bucket is summed row after row in ascending pair
 * order: bit-identical run to run, each Ssec_i symmetric bit for bit. F * n < 2^31. workspace: 256-byte aligned, at least
 * ktf_ivector_acc2_workspace_bytes(F, I, n) bytes. */
int64_t ktf_ivector_acc2_workspace_bytes(int64_t F, int32_t I, int32_t n);
int ktf_ivector_acc_second_order(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* gauss, const float* post, int32_t n,
                                 float posterior_scale, int32_t I, double* Ssec, void* workspace, size_t workspace_bytes, void* stream);
/* C (M x N, ldc) += A^T B in fp64 on v_mfma_f64_16x16x4_f64: A (K x M, lda) and B (K x N, ldb) row-major device arrays. Every
 * element is C + its K terms in ascending k (four per MFMA); no atomics, no split of K: the bits depend on the operands alone.
 * 1 <= M <= 2^22, 1 <= N <= 2^21; K = 0 leaves C as it is. */
int ktf_atb_f64(const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                void* stream);
/* gmm-gselect --n | fgmm-global-gselect-to-post --min-post (FullGmm::LogLikelihoodsPreselect, then the pruning loop of
 * fgmm-global-gselect-to-post.cc), the posterior stage of every sid/extract_ivectors.sh. The preselection is the diagonal call
 * above with min_post = 0: its gauss output is gmm-gselect's set (its post output is not used). Here, per frame t:
 *   gselect (F, n) device int32 lists the Gaussians; entries outside [0, I) are skipped. For each listed g
 *     l_g = gconst_g + means_invcovars_g . x - x^T inv_covars_g x / 2   (fp32; summed in an order that depends on D alone)
 *   p = exp(l - max) / sum over the listed set. With min_post != 0: every p < min_post is set to 0 and the rest divided by their
 *   sum; if that sum is 0 the arg-max (ties: the lower Gaussian index) gets 1. One pass, not the running-sum loop above.
 *   gauss / post (F, n): the Gaussians with p != 0 sorted by posterior, descending (ties: the lower index), then (-1, 0): the
 *   layout ktf_ivector_extract reads. A frame with nothing listed, or whose listed l are all -inf, gets n unused slots.
 * means_invcovars (I, D), gconst (I), inv_covars (I, D, D): device fp32 row-major; inv_covars holds the FULL matrices (not
 * Kaldi's packed triangle) and must be symmetric bit for bit (element [k][j] is read for [j][k]). workspace: 256-byte aligned, at
 * least ktf_fgmm_workspace_bytes(F, I, D, n) bytes (a negative KTF_* code on bad arguments); F * n < 2^31. The pairs are bucketed
 * by Gaussian and every bucket runs as an exact-fp32 MFMA GEMM against its matrix held in LDS; each pair's value is computed alone,
 * so a frame's output bits depend on its x row and its list alone: not on F, its position, the other frames or the run. */
int64_t ktf_fgmm_workspace_bytes(int64_t F, int32_t I, int32_t D, int32_t n);
int ktf_fgmm_post_f32(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* gselect, int32_t n,
                      const float* means_invcovars, const float* inv_covars, const float* gconst, int32_t I, float min_post,
                      int32_t* gauss, float* post, void* workspace, size_t workspace_bytes, void* stream);
/* ktf_fgmm_post_f32 with one more output: loglike (F) device fp32 or null, the frame's log-likelihood max + log(sum exp(l - max))
 * over the listed set, taken BEFORE the pruning (0 for a frame that counts as an empty list). gauss / post are bit-identical to
 * ktf_fgmm_post_f32's, with or without loglike; ktf_fgmm_post_f32 forwards here with null. */
int ktf_fgmm_post_ll_f32(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* gselect, int32_t n,
                         const float* means_invcovars, const float* inv_covars, const float* gconst, int32_t I, float min_post,
                         int32_t* gauss, float* post, float* loglike, void* workspace, size_t workspace_bytes, void* stream);
/* add-deltas (Kaldi's DeltaFeatures): x (B, T, D) fp32, element (b, t, d) at x[b * stride_b + t * stride_t + d] -> out (B, T,
 * D * (order + 1)) contiguous. coeffs: device fp32 (order + 1, 2 * order * window + 1), row i the order-i filter centred at column
 * order * window and zero beyond +- i * window (the caller computes them in fp32 as DeltaFeatures does). Block i of frame t is
 * sum_j coeffs[i][j] * x[clamp(t + j, 0, len_b - 1)], j ascending, zero coefficients skipped, every step acc = fl(acc + fl(s * x))
 * unfused. lengths: B device int32 or null (= T); rows at and beyond lengths[b] are written as zeros. */
#define KTF_ADD_DELTAS_MAX_CONTEXT 32
int ktf_add_deltas_f32(const float* x, int64_t B, int64_t T, int32_t D, int64_t stride_b, int64_t stride_t, const int32_t* lengths,
                       const float* coeffs, int32_t order, int32_t window, float* out, void* stream);

/* ------------------------------------------------------------------ UBM training statistics
 * The E-steps and accumulators of Kaldi's sid/train_diag_ubm.sh (gmm-global-init-from-feats, gmm-global-acc-stats --gselect) and
 * sid/train_full_ubm.sh (fgmm-global-acc-stats --gselect); the updates run on the host (kaldi_tflite_amd/training.py). Frames x
 * (F, D) fp32, row stride ldx; the limits of the i-vector entries: D <= KTF_IVECTOR_MAX_FEAT_DIM, I <= KTF_IVECTOR_MAX_GAUSS,
 * n <= KTF_IVECTOR_MAX_GSELECT, F * n < 2^31.
 *
 * DiagGmm::LogLikelihoodsPreselect, then the softmax of gmm-global-acc-stats --gselect: gselect (F, n) device int32 lists the
 * Gaussians of a frame, entries outside [0, I) are skipped. For each listed g, in fp32 and ascending d,
 *   l = gconst_g; l = fma(x_d, means_invvars_gd, l); l = fma(-0.5 * fl(x_d * x_d), inv_vars_gd, l)
 * post (F, n) = exp(l - max) / sum in the list's own slot order (no pruning, no sorting; skipped slots 0); loglike (F) = max +
 * log(sum). A frame with nothing listed, or whose listed l are all -inf, gets zeros and loglike 0; *valid (device int32, may be
 * null) is increased by the number of the other frames. A frame's bits depend on its own row and list alone. */
int ktf_gmm_post_preselect_f32(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* gselect, int32_t n,
                               const float* means_invvars, const float* inv_vars, const float* gconst, int32_t I, float* post,
                               float* loglike, int32_t* valid, void* stream);
/* The E-step of gmm-global-init-from-feats (no gselect): the log-likelihoods of all I Gaussians as ktf_ivector_post_f32 computes
 * them (W (2D, I) and gconst as there; the same device code, the same bits), softmax over all I in fp32:
 *   P (F, I) fp64 = fp32(exp(l - max) / sum);  Xaug (F, 2D + 1) fp64 = [1, x, x^2], the squares exact;  loglike (F) fp32 = max + log(sum).
 * The statistics are then ktf_atb_f64(A = P, B = Xaug) into (I, 2D + 1) = [occ, mean_acc, var_acc]. workspace: 256-byte aligned,
 * at least ktf_gmm_post_dense_workspace_bytes(F, I) bytes (F * I fp32; a negative KTF_* code on bad arguments). */
int64_t ktf_gmm_post_dense_workspace_bytes(int64_t F, int32_t I);
int ktf_gmm_post_dense_f32(const float* x, int64_t F, int32_t D, int64_t ldx, const float* W, const float* gconst, int32_t I, double* P,
                           double* Xaug, float* loglike, void* workspace, size_t workspace_bytes, void* stream);
/* AccumDiagGmm / AccumFullGmm::AccumulateFromPosteriors with double accumulators, on (frame, slot) pairs: gauss / post (F, n) device
 * int32 / fp32; a slot with an index outside [0, I) or a weight of 0 is skipped. Added in place to fp64 device accumulators:
 *   occ (I) += sum p;  mean_acc (I, D) += sum p x;  second_acc = var_acc (I, D) += sum p x^2 (full = 0)
 *                                                   or cov_acc (I, D, D) += sum p x x^T (full != 0), symmetric bit for bit.
 * The pairs are bucketed by Gaussian with the stable counting sort of ktf_ivector_acc_second_order; a bucket is cut into items of
 * KTF_GMM_ACC_ITEM_ROWS rows by a rule that depends on its count alone; an item is summed in ascending pair order (diagonal form:
 * fp64 VALU; full form: [1, x]^T diag(p) [1, x] on v_mfma_f64_16x16x4_f64, the lower triangle computed and mirrored); the items of
 * a Gaussian are added in ascending item order and that sum is added to the accumulator. No floating-point atomics: the same call
 * sequence gives the same bits. workspace: 256-byte aligned, at least ktf_gmm_acc_workspace_bytes(F, I, D, n, full) bytes (a
 * negative KTF_* code on bad arguments). */
#define KTF_GMM_ACC_ITEM_ROWS 1024
int64_t ktf_gmm_acc_workspace_bytes(int64_t F, int32_t I, int32_t D, int32_t n, int32_t full);
int ktf_gmm_acc_f64(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* gauss, const float* post, int32_t n, int32_t I,
                    int32_t full, double* occ, double* mean_acc, double* second_acc, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ PLDA back-end training statistics
 * The parts of Kaldi's `ivector-compute-lda`, `ivector-compute-plda` (PldaStats, PldaEstimator) and `est-pca --read-vectors=true`
 * whose cost grows with the rows or the speakers; the D x D factorisations run on the host (kaldi_tflite_amd/training.py). All sums
 * are fp64, split into row chunks by a rule that depends on the row count and D only and added in a fixed order (no atomics):
 * the results are bit-identical run to run and on any device or stream. 1 <= D <= KTF_TRAIN_MAX_DIM.
 *
 * PldaStats::AddSamples / ivector-mean: speaker s owns utts[offsets[s] .. offsets[s + 1]) (offsets S + 1 and utts n_idx device
 * int32) of the rows of x (N, D) fp32. means[s] (S, D) fp64 = the fp64 sum of its rows in list order / the count (not rounded to
 * fp32, unlike ktf_spk_mean_f32); counts[s] (S, device int32). A speaker with an empty or out-of-range list, or naming a row outside
 * [0, N), gets a NaN row and count 0 (callers check the map: this only keeps the kernel inside its arrays). */
#define KTF_TRAIN_MAX_DIM 1024
int ktf_train_class_means(const float* x, int64_t N, int32_t D, const int32_t* offsets, int64_t S, const int32_t* utts,
                          int64_t n_idx, double* means, int32_t* counts, void* stream);
/* Scratch of the two calls below for `rows` rows: a device buffer of at least this many bytes (a negative KTF_* code on bad
 * arguments). */
int64_t ktf_train_workspace_bytes(int64_t rows, int32_t D);
/* mean (D, device fp64) = the column means of rows (rows, D) fp32 / fp64: the global mean of ivector-compute-lda and est-pca, and
 * PldaStats' mean of the class means. Sums over fixed chunks of 256 rows, then the chunks in order. */
int ktf_train_mean_f32(const float* x, int64_t rows, int32_t D, double* mean, void* workspace, size_t workspace_bytes, void* stream);
int ktf_train_mean_f64(const double* y, int64_t rows, int32_t D, double* mean, void* workspace, size_t workspace_bytes, void* stream);
/* G (D x D, device fp64, symmetric bit for bit) = sum_r w_r (y_{i_r} - c)(y_{i_r} - c)^T over the list positions r < rows, with
 * i_r = idx[r] (idx: `rows` device int32; NULL: i_r = r, rows <= N), w_r = weights[r] (NULL: 1) and c = center (D, NULL: 0), all
 * device arrays; y (N, D) fp32 (x) or fp64 (class means, EM rows). The scatter matrices of ivector-compute-lda (total and between
 * class), est-pca's covariance and PldaStats' within-class scatter; the two SYRKs of the PLDA EM. A listed index outside [0, N)
 * contributes nothing (callers check the list). */
int ktf_train_gram_f32(const float* x, int64_t N, int32_t D, const int32_t* idx, int64_t rows, const double* center,
                       const double* weights, double* G, void* workspace, size_t workspace_bytes, void* stream);
int ktf_train_gram_f64(const double* y, int64_t N, int32_t D, const int32_t* idx, int64_t rows, const double* center,
                       const double* weights, double* G, void* workspace, size_t workspace_bytes, void* stream);
/* One PldaEstimator EM step's row transform in the simultaneous diagonalisation P Phi_w P^T = I, P Phi_b P^T = diag(lam):
 * y_s = P (mu_s - mbar) (mu (S, D), mbar (D), P (D x D row-major), all device fp64), then with n = counts[s] (S, device int32)
 * a[s][d] = n lam_d / (1 + n lam_d) y_s[d] and b[s][d] = y_s[d] / (1 + n lam_d) (a, b: (S, D) device fp64). */
int ktf_plda_em_project(const double* mu, int64_t S, int32_t D, const double* mbar, const double* P, const double* lam,
                        const int32_t* counts, double* a, double* b, void* stream);

/* ------------------------------------------------------------------ VB-HMM resegmentation
 * The variational-Bayes HMM of Kaldi's diarization/VB_resegmentation.sh (VB_diarization.py, min_dur = 1) for the N recordings of a
 * call: I Gaussians, D features, R i-vector dimensions, K <= KTF_VB_MAX_SPEAKERS speakers. Frames lie end to end in x (F, D) fp32,
 * row stride ldx: recording r owns frames [offsets[r], offsets[r + 1]) and blocks [boffsets[r], boffsets[r + 1]) of the TB rows of
 * q / lls (both tables: N + 1 device int32); block b of a recording covers its frames [b d, min((b + 1) d, T_r)), d = downsample.
 * Every fp64 sum runs in a fixed order that depends on the recording alone: its results have the same bits alone and in a batch.
 *
 * Posteriors: l as ktf_ivector_post_f32 computes it (W, gconst as there; the same device code) times ll_scale in fp32;
 * loglike (F) = G = max + log sum exp(l - max) over all I; p = fp32(exp(l - G) * stat_scale). A frame keeps the Gaussians with
 * p >= sparsity_thr, largest first, ties to the lower index, at most n, not renormalised: gauss / post (F, n), unused slots (-1, 0).
 * *truncated (device int32) is increased by the number of frames with more than n candidates. workspace: 256-byte aligned, at
 * least ktf_vb_post_workspace_bytes(F, I) bytes (F * I fp32). */
#define KTF_VB_MAX_SPEAKERS 16
#define KTF_VB_FB_CHUNK 128
int64_t ktf_vb_post_workspace_bytes(int64_t F, int32_t I);
int ktf_vb_post_f32(const float* x, int64_t F, int32_t D, int64_t ldx, const float* W, const float* gconst, int32_t I, int32_t n,
                    float ll_scale, float stat_scale, float sparsity_thr, int32_t* gauss, float* post, float* loglike,
                    int32_t* truncated, void* workspace, size_t workspace_bytes, void* stream);
/* The (frame, slot) pairs of gauss (F, n) bucketed by Gaussian with the stable counting sort of ktf_ivector_acc_second_order:
 * start (I + 1) and pairs (F * n) device int32; pairs[start[c] .. start[c + 1]) lists the pair ids t * n + slot of Gaussian c in
 * ascending order (slots with an index outside [0, I) are left out). Once per call of the resegmentation. */
int64_t ktf_vb_bucket_workspace_bytes(int64_t F, int32_t I, int32_t n);
int ktf_vb_bucket(const int32_t* gauss, int64_t F, int32_t n, int32_t I, int32_t* start, int32_t* pairs, void* workspace,
                  size_t workspace_bytes, void* stream);
/* Soft statistics of speaker s of recording r (row r K + s): Nst (N K, I) = sum_t q_ts p_tc, Fst (N K, I D) = sum_t q_ts p_tc
 * (x_t - m_c), over the pairs of c in ascending pair order; q (TB, K) fp64, a frame uses the row of its block; means (I, D) fp64.
 * Every element is written. No floating-point atomics. */
int ktf_vb_speaker_stats(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* offsets, const int32_t* boffsets, int32_t N,
                         int64_t TB, int32_t downsample, const float* post, int32_t n, const int32_t* start, const int32_t* pairs,
                         int32_t I, const double* means, const double* q, int32_t K, double* Nst, double* Fst, void* stream);
/* Speaker posteriors of the B = N K rows: lin = Bm^T vec(F) (Bm (I D, R): row (c, d) = iE_cd M_c[d, :]), Q = I + sum_c N_c U_c =
 * L L^T (U (I, P), P = R(R+1)/2, packed lower triangles: the layouts of ktf_ivector_extract), C = Q^-1, a (B, R) = C lin,
 * Wp (B, P) = C + a a^T packed, kl (B) = (R - tr W) / 2 - sum_j log L_jj, h (B, I D) = Bm a, g (B, I) = tr(U_c W) / 2 (on packed
 * triangles the off-diagonal entries count twice). The two products with B rows run on v_mfma_f64_16x16x4_f64. workspace: 256-byte
 * aligned, at least ktf_vb_update_workspace_bytes(B, I, D, R) bytes. */
int64_t ktf_vb_update_workspace_bytes(int32_t B, int32_t I, int32_t D, int32_t R);
int ktf_vb_speaker_update(const double* Nst, const double* Fst, int32_t B, int32_t I, int32_t D, int32_t R, const double* Bm,
                          const double* U, double* a, double* Wp, double* kl, double* h, double* g, void* workspace,
                          size_t workspace_bytes, void* stream);
/* lls (TB, K) fp64: row b = sum over the block's frames in order, then their slots in order, of p_tc ((x_t - m_c) . h_sc - g_sc). */
int ktf_vb_block_loglike(const float* x, int64_t F, int32_t D, int64_t ldx, const int32_t* offsets, const int32_t* boffsets, int32_t N,
                         int64_t TB, int32_t downsample, const int32_t* gauss, const float* post, int32_t n, int32_t I,
                         const double* means, const double* h, const double* g, int32_t K, double* lls, void* stream);
/* Forward-backward of the HMM with initial probabilities sp (N, K) and transitions i -> j = loop_prob [i = j] + (1 - loop_prob)
 * sp_j over each recording's blocks, emissions exp(lls): a chunked scan in scaled fp64, KTF_VB_FB_CHUNK blocks per chunk (a
 * function of nothing else). q (TB, K) = the state posteriors; tll (N) = log p(blocks) (0 for a recording without blocks); sp_out
 * (N, K) proportional to q_0j + sum_{b >= 1} Pr(block b entered j through the non-loop term), normalised (sp itself for a recording
 * without blocks). workspace: 256-byte aligned, at least ktf_vb_fb_workspace_bytes(TB, N) bytes. */
int64_t ktf_vb_fb_workspace_bytes(int64_t TB, int32_t N);
int ktf_vb_forward_backward(const double* lls, const int32_t* boffsets, int32_t N, int64_t TB, int32_t K, const double* sp,
                            double loop_prob, double* q, double* sp_out, double* tll, void* workspace, size_t workspace_bytes,
                            void* stream);
/* The same forward-backward in its serial form, for measurement only (tools/bench_vb.py times the chunked scan against it; nothing
 * in the package calls it): one wave per recording walks all its blocks, lane i = speaker i, the scaled forward vectors kept in the
 * workspace. Same arguments and results (to rounding; the sums run in another order); workspace: 256-byte aligned, at least
 * ktf_vb_fb_serial_workspace_bytes(TB, N) bytes. */
int64_t ktf_vb_fb_serial_workspace_bytes(int64_t TB, int32_t N);
int ktf_vb_forward_backward_serial(const double* lls, const int32_t* boffsets, int32_t N, int64_t TB, int32_t K, const double* sp,
                                   double loop_prob, double* q, double* sp_out, double* tll, void* workspace, size_t workspace_bytes,
                                   void* stream);
/* The bound. ktf_vb_loglike_sums: gsum (N) fp64 = sum_t G_t over each recording's frames of loglike (F) fp32, thread-strided from
 * the recording's first frame and then a fixed tree (once per call). ktf_vb_bound: bound (N) = stat_scale gsum + tll + sum_s kl
 * (kl (N K), s ascending). Neither depends on where a recording lies in the packed arrays. */
int ktf_vb_loglike_sums(const float* loglike, const int32_t* offsets, int32_t N, int64_t F, double* gsum, void* stream);
int ktf_vb_bound(const double* gsum, const double* tll, const double* kl, int32_t N, int32_t K, double stat_scale, double* bound,
                 void* stream);

/* ------------------------------------------------------------------ VBx
 * The VB-HMM of Landini / Diez / Burget ("Bayesian HMM clustering of x-vector sequences") over the window x-vectors of the N
 * recordings of a call, in the PLDA-transformed space: within-class covariance I, between-class covariance diag(phi), D <=
 * KTF_VBX_MAX_DIM dimensions (512, ktf_plda_dense_*'s limit: no stage keeps a 16 x D block in LDS, so no LDS budget binds it),
 * K <= KTF_VB_MAX_SPEAKERS speakers, everything fp64. Windows lie end to end in time order: recording r owns rows [offsets[r],
 * offsets[r + 1]) of the TB rows of x / rho / gamma / lls (offsets: N + 1 device int32, the convention of ktf_vb_*). One iteration is
 * ktf_vbx_speaker_update, ktf_vbx_loglike, ktf_vb_forward_backward (gamma = q, pi = sp) and ktf_vb_bound with a zero gsum and
 * Fb kl: ELBO = tll + Fb sum_k kl_k. A speaker with pi_k = 0 and a zero gamma column stays at zero and adds 0 to the bound, so a
 * batch runs at one K and zero-pads the speakers a recording does not use.
 * Every fp64 sum runs in a fixed order that depends on the recording alone: its results have the same bits alone, in a batch and
 * at any offset. The orders: G_t: lane l of a wave takes d = l, l + 64, ..., then a butterfly over the 64 lanes. gamma^T rho and
 * N_k: a recording's windows are cut into chunks of KTF_VBX_UPDATE_ROWS counted from its first window, one workgroup per chunk;
 * within a chunk the windows ascend, four per v_mfma_f64_16x16x4_f64; the chunks' partial sums are then added in chunk order. c_k
 * and kl_k: lane j of 16 takes d = j, j + 16, ..., then a butterfly over the 16. lls_tk: d ascending, four per MFMA.
 *
 * ktf_vbx_prepare: x (TB, D), phi (D) > 0 -> rho (TB, D) = x sqrt(phi), G (TB) = -(sum_d x_td^2 + D log 2 pi) / 2. */
#define KTF_VBX_MAX_DIM 512
#define KTF_VBX_UPDATE_ROWS 256
int ktf_vbx_prepare(const double* x, int64_t TB, int32_t D, const double* phi, double* rho, double* G, void* stream);
/* With N_k = sum_t gamma_tk over the recording's windows and f = fa_over_fb: invL (N, K, D) = 1 / (1 + f N_k phi_d), alpha
 * (N, K, D) = f invL sum_t gamma_tk rho_td, c (N, K) = sum_d (invL + alpha^2) phi_d / 2, kl (N, K) = sum_d (log invL - invL -
 * alpha^2 + 1) / 2; gamma (TB, K). A recording without windows gets c = kl = 0 and its rows of alpha and invL are not written.
 * workspace: 256-byte aligned, at least ktf_vbx_update_workspace_bytes(TB, N, D) bytes. */
int64_t ktf_vbx_update_workspace_bytes(int64_t TB, int32_t N, int32_t D);
int ktf_vbx_speaker_update(const double* gamma, const double* rho, int64_t TB, int32_t D, int32_t K, const int32_t* offsets, int32_t N,
                           const double* phi, double fa_over_fb, double* alpha, double* invL, double* c, double* kl, void* workspace,
                           size_t workspace_bytes, void* stream);
/* lls (TB, K): row t of recording r = Fa (sum_d rho_td alpha_rkd - c_rk + G_t), in tiles of 16 windows x 16 speakers on the same
 * MFMA; rows of another recording and speakers past K contribute nothing to a tile. */
int ktf_vbx_loglike(const double* rho, const double* G, int64_t TB, int32_t D, int32_t K, const int32_t* offsets, int32_t N,
                    const double* alpha, const double* c, double Fa, double* lls, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KTF_HIP_H_ */
