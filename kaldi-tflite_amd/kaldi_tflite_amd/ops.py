"""
Thin torch-tensor wrappers over the C-ABI (one function per entry point of include/ktf_hip.h)
plus the host-side constant tables the kernels consume (window, FFT twiddles, sparse mel bank,
DCT matrix, lifter), computed once in float64 exactly as the reference's layer `build()`
methods do and uploaded as fp32.

PyTorch is used for device memory and streams only; all arithmetic on activations happens in
the HIP kernels.
"""

import ctypes as C

import numpy as np
import torch

from . import _lib as L


def _dev(device=None):
    L.require_gpu()
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def default_device():
    return _dev(None)


def to_device_f32(x, device=None):
    """numpy / tensor -> contiguous fp32 tensor on the GPU."""
    dev = _dev(device)
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=torch.float32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float32)), device=dev)


def round_up(n, m):
    return (n + m - 1) // m * m


# ----------------------------------------------------------------------------- host-side tables
def window_function(window_type, M, blackman_coeff=0.42):
    """layers/dsp/windowing.py:110-156 of the reference (float64)."""
    t = window_type.lower()
    n = np.arange(0, M)
    if M == 1:
        return np.ones(1, float)
    if t == "hamming":
        return np.hamming(M)
    if t == "hanning":
        return np.hanning(M)
    if t == "povey":
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / (M - 1))) ** 0.85
    if t == "rectangular":
        return np.ones((M,))
    if t == "sine":
        return np.sin(np.pi * n / (M - 1))
    if t == "blackman":
        w = np.blackman(M)
        if blackman_coeff != 0.42:
            w = w - 0.42 + blackman_coeff
        return w
    raise ValueError(f"window_type '{window_type}' is not recognized")


def next_power_of_2(n):
    if n & (n - 1) == 0 and n != 0:
        return n
    return 2 ** (n - 1).bit_length()


def mel_bank_dense(window_size, num_bins, sample_freq, lower, upper):
    """layers/dsp/filterbank.py:141-189: dense (nfft/2+1, num_bins) fp32 bank (weights in fp64, strict
    left < mel < right, no weight on the Nyquist bin)."""
    nfft = next_power_of_2(window_size)
    bins = nfft // 2
    bw = sample_freq / nfft
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)  # noqa: E731
    mlo, mhi = mel(lower), mel(upper)
    delta = (mhi - mlo) / (num_bins + 1)
    bank = np.zeros([num_bins, bins + 1], dtype=np.float32)
    m = mel(bw * np.arange(bins))
    for i in range(num_bins):
        left = mlo + i * delta
        center = left + delta
        right = center + delta
        inside = (m > left) & (m < right)
        up = (m - left) / (center - left)
        down = (right - m) / (right - center)
        bank[i, :bins] = np.where(inside, np.where(m <= center, up, down), 0.0)
    return nfft, bank.T.copy()


def dct_matrix(input_length, length):
    """layers/dsp/dct.py:98-143 (float64, (input_length, length); column 0 overwritten with sqrt(1/N))."""
    N = float(input_length)
    n = np.arange(input_length)
    k = np.arange(length, dtype=np.float64)[:, None]
    d = np.cos(np.pi / N * (n + 0.5) * k)
    d[0] *= 1.0 / np.sqrt(2.0)
    d *= np.sqrt(2.0 / N)
    d = d.T
    d[:, 0] = np.sqrt(1.0 / N)
    return d


def lifter_coeffs(num_mfccs, q):
    n = np.arange(0, num_mfccs)
    return 1 + 0.5 * np.sin(np.pi * n / q) * q


def fast512_tables(starts, lens, w, maxw=16):
    """Per-lane constants of frontend512.hip: FFT twiddles of the lane-level radix-4 schedule and the split of the
    sparse mel bank into <= 64 (filter, <= maxw-bin slice) work items with <= 4 adjacent lanes per filter."""
    lane = np.arange(64)
    n0 = (lane >> 1) + 32 * (lane & 1)
    n1 = (lane >> 1) & 15
    n2 = (lane >> 1) & 3
    tw = np.zeros((64, 18), np.float64)
    for r in (1, 2, 3):
        for base, nn, N in ((0, n0, 256), (6, n1, 64), (12, n2, 16)):
            ang = -2.0 * np.pi * nn * r / N
            tw[:, base + 2 * (r - 1)] = np.cos(ang)
            tw[:, base + 2 * (r - 1) + 1] = np.sin(ang)
    def split(width):
        its = []                                # (filter, start, len)
        for f, (s0, ln) in enumerate(zip(starts, lens)):
            if ln == 0:
                its.append((f, s0, 0))
                continue
            parts = -(-ln // width)
            if parts > 4:
                return None
            step = -(-ln // parts)
            for p in range(parts):
                a = p * step
                b = min(ln, a + step)
                its.append((f, s0 + a, b - a))
        return its if len(its) <= 64 else None

    items, used = None, None
    for width in range(8, maxw + 1):            # smallest slice width that fits 64 lanes with <= 4 lanes per filter
        items = split(width)
        if items is not None:
            used = max(ln for _, _, ln in items)
            break
    if items is None:
        return None
    meta = np.zeros((64, 4), np.int32)
    meta[:, 2] = -1
    mw = np.zeros((64, maxw), np.float32)
    for i, (f, s0, ln) in enumerate(items):
        meta[i, 0], meta[i, 1], meta[i, 2] = s0, ln, f
        mw[i, :ln] = w[f, s0 - starts[f]: s0 - starts[f] + ln]
    for i, (f, _, _) in enumerate(items):
        fl = 0
        if i + 1 < len(items) and items[i + 1][0] == f:
            fl |= 1
        if i + 2 < len(items) and items[i + 2][0] == f:
            fl |= 2
        if i == 0 or items[i - 1][0] != f:
            fl |= 4
        meta[i, 3] = fl
    return tw, meta, mw, max(int(used), 1)


class FrontendTables:
    """Device copies of every constant ktf_frontend_f32 needs, for one (frame_size, mel, dct) configuration."""

    def __init__(self, frame_size, window=None, mel_bank=None, dct=None, lifter=None, device=None):
        dev = _dev(device)
        self.frame_size = int(frame_size)
        self.nfft = next_power_of_2(self.frame_size)
        n2 = self.nfft // 2
        k = np.arange(n2)
        tw = np.stack([np.cos(2 * np.pi * k / n2), -np.sin(2 * np.pi * k / n2)], -1)
        rtw = np.stack([np.cos(2 * np.pi * k / self.nfft), -np.sin(2 * np.pi * k / self.nfft)], -1)
        f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)  # noqa: E731
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dev)  # noqa: E731
        self.window = f32(window) if window is not None else None
        self.twiddle = f32(tw.reshape(-1))
        self.rtwiddle = f32(rtw.reshape(-1))
        self.mel_start = self.mel_len = self.mel_w = None
        self.mel_stride = 0
        self.num_mels = 0
        if mel_bank is not None:
            bank = np.asarray(mel_bank, dtype=np.float32)          # (nfft/2+1, num_mels)
            assert bank.shape[0] == n2 + 1
            self.num_mels = bank.shape[1]
            starts, lens = [], []
            for f in range(self.num_mels):
                nz = np.nonzero(bank[:n2, f])[0]
                if nz.size == 0:
                    starts.append(0)
                    lens.append(0)
                else:
                    starts.append(int(nz[0]))
                    lens.append(int(nz[-1] - nz[0] + 1))
            self.mel_stride = max(1, max(lens))
            w = np.zeros((self.num_mels, self.mel_stride), np.float32)
            for f in range(self.num_mels):
                w[f, :lens[f]] = bank[starts[f]:starts[f] + lens[f], f]
            self.mel_start, self.mel_len, self.mel_w = i32(starts), i32(lens), f32(w)
        self.dct = f32(dct) if dct is not None else None
        self.lifter = f32(lifter) if lifter is not None else None
        # tables of the register-resident nfft = 512 fast path (frontend512.hip)
        self.fast_tw = self.fast_mel_meta = self.fast_mel_w = None
        fast_maxw = 0
        if self.nfft == 512 and mel_bank is not None and self.num_mels <= 32:
            fast = fast512_tables(starts, lens, w)
            if fast is not None:
                self.fast_tw, self.fast_mel_meta, self.fast_mel_w = f32(fast[0]), i32(fast[1]), f32(fast[2])
                fast_maxw = fast[3]
        self.struct = L.FrontendTables(
            window=L.ptr(self.window), twiddle=L.ptr(self.twiddle), rtwiddle=L.ptr(self.rtwiddle),
            mel_start=L.ptr(self.mel_start), mel_len=L.ptr(self.mel_len), mel_w=L.ptr(self.mel_w),
            dct=L.ptr(self.dct), lifter=L.ptr(self.lifter), fast_tw=L.ptr(self.fast_tw),
            fast_mel_meta=L.ptr(self.fast_mel_meta), fast_mel_w=L.ptr(self.fast_mel_w), mel_stride=self.mel_stride,
            reserved=fast_maxw)


# ----------------------------------------------------------------------------- entry-point wrappers
def num_frames(n_samples, frame_size, frame_shift):
    return int(L.load().ktf_num_frames(int(n_samples), int(frame_size), int(frame_shift)))


def frontend(x, in_kind, cfg, tables, out_stage, n, B, T, seed=0, want_energy=False, out=None):
    """x: fp32 device tensor (int16 for L.IN_WAV_I16). Returns out (B,T,last) [, energy (B,T)]."""
    lib = L.load()
    last = {L.OUT_FRAMES: cfg.frame_size, L.OUT_WINDOWED: cfg.frame_size, L.OUT_FBANK: cfg.num_mels,
            L.OUT_MFCC: cfg.num_ceps}[out_stage]
    if out is None:
        out = torch.empty((B, T, last), dtype=torch.float32, device=x.device)
    energy = torch.empty((B, T), dtype=torch.float32, device=x.device) if want_energy else None
    with L.on_device(x.device):
        rc = lib.ktf_frontend_f32(L.ptr(x), B, n, in_kind, C.byref(cfg), C.byref(tables.struct), out_stage, L.ptr(out),
                                  L.ptr(energy), C.c_uint64(seed & (2**64 - 1)), L.stream_ptr())
    L.check(rc, "ktf_frontend_f32")
    return (out, energy) if want_energy else out


def frontend_plan(B, n, in_kind, cfg, tables, out_stage):
    """Which kernel instance `frontend` runs for this call, on what grid and with how much LDS: a `FrontendPlan`
    (ktf_frontend_plan: the launcher's own decision; host arithmetic, no GPU needed). `tables`: a FrontendTables, or the bare
    `_lib.FrontendTables` struct (its pointers are only tested for NULL)."""
    plan = L.FrontendPlan()
    tab = getattr(tables, "struct", tables)
    L.check(L.load().ktf_frontend_plan(B, n, in_kind, C.byref(cfg), C.byref(tab), out_stage, C.byref(plan)), "ktf_frontend_plan")
    return plan


def dct(x2d, dct_t, lifter_t, out_dim):
    lib = L.load()
    rows, in_dim = x2d.shape
    out = torch.empty((rows, out_dim), dtype=torch.float32, device=x2d.device)
    with L.on_device(x2d.device):
        rc = lib.ktf_dct_f32(L.ptr(x2d), rows, in_dim, out_dim, L.ptr(dct_t), L.ptr(lifter_t), L.ptr(out), L.stream_ptr())
    L.check(rc, "ktf_dct_f32")
    return out


def vad_mask(feats, cfg):
    lib = L.load()
    B, T, D = feats.shape
    mask = torch.empty((B, T), dtype=torch.float32, device=feats.device)
    with L.on_device(feats.device):
        rc = lib.ktf_vad_mask_f32(L.ptr(feats), B, T, D, C.byref(cfg), L.ptr(mask), L.stream_ptr())
    L.check(rc, "ktf_vad_mask_f32")
    return mask


def vad_index(feats, cfg):
    lib = L.load()
    B, T, D = feats.shape
    idx = torch.empty((B, T), dtype=torch.int32, device=feats.device)
    lens = torch.empty((B,), dtype=torch.int32, device=feats.device)
    with L.on_device(feats.device):
        rc = lib.ktf_vad_index(L.ptr(feats), B, T, D, C.byref(cfg), L.ptr(idx), L.ptr(lens), L.stream_ptr())
    L.check(rc, "ktf_vad_index")
    return idx, lens


def cmvn(x, cfg, lens=None, ldo=None, want_lens=False):
    lib = L.load()
    B, T, D = x.shape
    ldo = D if ldo is None else ldo
    out = torch.empty((B, T, ldo), dtype=torch.float32, device=x.device)
    work = torch.empty((B * T * 2 * D + 2 * D,), dtype=torch.float32, device=x.device)
    out_lens = torch.empty((B,), dtype=torch.int32, device=x.device) if want_lens else None
    with L.on_device(x.device):
        rc = lib.ktf_cmvn_f32(L.ptr(x), B, T, D, x.stride(1), L.ptr(lens), C.byref(cfg), L.ptr(out), ldo, L.ptr(out_lens),
                              L.ptr(work), L.stream_ptr())
    L.check(rc, "ktf_cmvn_f32")
    return (out, out_lens) if want_lens else out


def vad_cmvn(feats, vad_cfg, cmvn_cfg, out, lens, idx_work, work):
    lib = L.load()
    B, T, D = feats.shape
    dt = L.ktf_dtype(out.dtype)
    with L.on_device(feats.device):
        rc = lib.ktf_vad_cmvn(L.ptr(feats), B, T, D, C.byref(vad_cfg), C.byref(cmvn_cfg), L.ptr(out), dt, out.stride(1),
                              L.ptr(lens), L.ptr(idx_work), L.ptr(work), L.stream_ptr())
    L.check(rc, "ktf_vad_cmvn")


def vad_cmvn_plan(B, T, D, ldo):
    """Where `vad_cmvn` keeps its working data for a (B, T, D) batch written at row stride ldo: a `VcPlan` (ktf_vad_cmvn_plan;
    host arithmetic, no GPU needed)."""
    plan = L.VcPlan()
    L.check(L.load().ktf_vad_cmvn_plan(B, T, D, ldo, C.byref(plan)), "ktf_vad_cmvn_plan")
    return plan


def cmvn_plan(T, D, ldo=None):
    """The same for `cmvn` on utterances of T frames (ktf_cmvn_plan)."""
    plan = L.VcPlan()
    L.check(L.load().ktf_cmvn_plan(T, D, D if ldo is None else ldo, C.byref(plan)), "ktf_cmvn_plan")
    return plan


def last_kernel():
    """Kernel family the calling thread's last ktf_tdnn* / ktf_tdnn_mx* call launched (include/ktf_hip.h)."""
    return (L.load().ktf_tdnn_last_kernel() or b"").decode()


def build_id():
    """16 hex digits naming the sources the loaded library was built from (ktf_build_id)."""
    return (L.load().ktf_build_id() or b"").decode()


def clock_probe(out, us, stream):
    """Launches the one-wave shader-clock probe on `stream` (a torch.cuda.Stream of its own, next to the measured work): out is a
    (4,) int64 CUDA tensor that receives shader clocks, 100 MHz ticks, lowest / highest kHz over 1 ms windows (ktf_clock_probe)."""
    with L.on_device(out.device):
        rc = L.load().ktf_clock_probe(L.ptr(out), int(us), stream.cuda_stream)
    L.check(rc, "ktf_clock_probe")
    return out


def route_short(lens, min_frames, lens_main, lens_short, host_flag=None, seq=0):
    """lens -> (lens_main, lens_short) by voiced length (ktf_route_short); host_flag: pinned int32[2] CPU tensor that receives the number
    of short utterances and then `seq`."""
    lib = L.load()
    with L.on_device(lens.device):
        rc = lib.ktf_route_short(L.ptr(lens), lens.shape[0], int(min_frames), L.ptr(lens_main), L.ptr(lens_short),
                                 host_flag.data_ptr() if host_flag is not None else None, int(seq), L.stream_ptr())
    L.check(rc, "ktf_route_short")


def tdnn_out_len(T, desc):
    return int(L.load().ktf_tdnn_out_len(int(T), C.byref(desc)))


def tdnn_out_lens(lens, desc, out):
    """out[b] = tdnn_out_len(lens[b]) on the device (for the layers behind ktf_tdnn_mx, which has no out_lens argument)."""
    with L.on_device(lens.device):
        rc = L.load().ktf_tdnn_out_lens(L.ptr(lens), lens.shape[0], C.byref(desc), L.ptr(out), L.stream_ptr())
    L.check(rc, "ktf_tdnn_out_lens")
    return out


def tdnn(x, lens, desc, w, w_lo, bias, scale, shift, y, out_lens=None):
    """x (B,T,ldx) fp32/bf16, y (B,Tout,ldy) preallocated."""
    lib = L.load()
    B, T = x.shape[0], x.shape[1]
    with L.on_device(x.device):
        rc = lib.ktf_tdnn(L.ptr(x), B, T, x.stride(1), L.ptr(lens), C.byref(desc), L.ptr(w), L.ptr(w_lo), L.ptr(bias),
                          L.ptr(scale), L.ptr(shift), L.ptr(y), y.stride(1), L.ptr(out_lens), L.stream_ptr())
    L.check(rc, "ktf_tdnn")
    return y


def stats_slots(T, mx_flags=None):
    """Slots of the reproducible pooling layout (KTF_TDNN_DET_STATS) for utterances of up to T rows: 128-row slots, or -- for
    ktf_tdnn_mx_stats, `mx_flags` = its KtfTdnnDesc.flags -- the slots of the MX kernel in use (mx_slot_rows rows each)."""
    if mx_flags is None:
        return int(L.load().ktf_stats_slots(int(T)))
    return int(L.load().ktf_mx_stats_slots(int(T), int(mx_flags)))


def tdnn_stats_slots(T, gemm):
    """Slots / rows per slot of ktf_tdnn_stats with KTF_TDNN_DET_STATS for a GEMM mode (KTF_GEMM_BF16X4: one per 64-row tile)."""
    return int(L.load().ktf_tdnn_stats_slots(int(T), int(gemm)))


def tdnn_slot_rows(gemm):
    return int(L.load().ktf_tdnn_slot_rows(int(gemm)))


def mx_slot_rows(mx_flags):
    return int(L.load().ktf_mx_slot_rows(int(mx_flags)))


def tdnn_stats(x, lens, desc, w, w_lo, bias, scale, shift, sums, zero=True):
    """Fused TDNN + reducing stats pooling: accumulates fp64 column sums / sums of squares into `sums` (B,2,units), or
    stores them per 128-row block into (B,slots,2,units) when desc.flags has TDNN_DET_STATS (zero=False then)."""
    lib = L.load()
    B, T = x.shape[0], x.shape[1]
    with L.on_device(x.device):
        if zero:
            sums.zero_()
        rc = lib.ktf_tdnn_stats(L.ptr(x), B, T, x.stride(1), L.ptr(lens), C.byref(desc), L.ptr(w), L.ptr(w_lo), L.ptr(bias),
                                L.ptr(scale), L.ptr(shift), L.ptr(sums), L.stream_ptr())
    L.check(rc, "ktf_tdnn_stats")
    return sums


# ----------------------------------------------------------------------------- the back-end wrappers' way into the library
# (the extraction-path wrappers above and split_bf16 .. plda below spell their calls out: they run ~10 times per batch-1 extraction)
def _call(name, device, *args):
    """The library's `name`(*args, stream) with `device` current; a failure raises through L.check."""
    fn = getattr(L.load(), name)
    with L.on_device(device):
        rc = fn(*args, L.stream_ptr())
    L.check(rc, name)


def _typed(stem, t):
    """The `_f64` / `_f32` symbol of `stem` for tensor t."""
    return stem + ("_f64" if t.dtype == torch.float64 else "_f32")


def _size(name, *args):
    """A `*_workspace_bytes` symbol's answer; a negative one raises through L.check."""
    n = int(getattr(L.load(), name)(*args))
    if n < 0:
        L.check(n, name)
    return n


def _workspace(name, *args, device):
    """A fresh uint8 workspace on `device` of the size `name`(*args) asks for."""
    return torch.empty((_size(name, *args),), dtype=torch.uint8, device=device)


def _ld(x):
    """Row stride of a 2-D x; its width when it has no rows."""
    return x.stride(0) if x.shape[0] else x.shape[1]


def _new(like, *shape, dtype=None):
    return torch.empty(shape, dtype=dtype or like.dtype, device=like.device)


def plda_score(test_tr, enroll_tr, psi):
    """scores (N, M) of transformed test vectors against transformed enrollment vectors."""
    N, dim = test_tr.shape
    M = enroll_tr.shape[0]
    scores = _new(test_tr, N, M)
    _call(_typed("ktf_plda_score", test_tr), test_tr.device, L.ptr(test_tr), N, L.ptr(enroll_tr), M, dim, L.ptr(psi), L.ptr(scores))
    return scores


# ----------------------------------------------------------------------------- speaker verification (ktf_spk_mean_f32, ktf_plda_*_n_*)
def spk_mean(raw, offsets, utts, S, means=None, num_utts=None):
    """Kaldi ivector-mean: raw (U, D) fp32, the CSR map offsets (S + 1) / utts on the device (int32) -> (means (S, D) fp32,
    num_utts (S,) int32)."""
    U, D = raw.shape
    if means is None:
        means = _new(raw, S, D, dtype=torch.float32)
    if num_utts is None:
        num_utts = _new(raw, S, dtype=torch.int32)
    _call("ktf_spk_mean_f32", raw.device, L.ptr(raw), U, D, L.ptr(offsets), S, L.ptr(utts), utts.numel(), L.ptr(means), L.ptr(num_utts))
    return means, num_utts


def plda_transform_n(x, A, offset, psi, num_examples, normalize_length, simple_length_norm):
    """transformVector(x, num_examples): x (B, dim), num_examples (B,) on the device in x's dtype -> (B, dim)."""
    B, dim = x.shape
    tr = torch.empty_like(x)
    _call(_typed("ktf_plda_transform_n", x), x.device, L.ptr(x), B, dim, L.ptr(A), L.ptr(offset), L.ptr(psi), L.ptr(num_examples),
          int(normalize_length), int(simple_length_norm), L.ptr(tr))
    return tr


def plda_score_n(test_tr, enroll_tr, psi, enroll_num_examples):
    """scores (N, M) with class j averaging enroll_num_examples[j] examples (device, the dtype of the vectors)."""
    N, dim = test_tr.shape
    M = enroll_tr.shape[0]
    scores = _new(test_tr, N, M)
    _call(_typed("ktf_plda_score_n", test_tr), test_tr.device, L.ptr(test_tr), N, L.ptr(enroll_tr), M, dim, L.ptr(psi),
          L.ptr(enroll_num_examples), L.ptr(scores))
    return scores


def plda_trials(test_tr, enroll_tr, psi, enroll_num_examples, pairs, workspace=None):
    """scores (T,) of the trial list pairs (T, 2) device int32 rows (class j, test i). workspace(nbytes) -> a uint8 device tensor
    (None: a fresh one)."""
    N, dim = test_tr.shape
    M = enroll_tr.shape[0]
    T = pairs.shape[0]
    scores = _new(test_tr, T)
    if T == 0:
        return scores
    nbytes = _size("ktf_plda_trials_workspace_bytes", N, M, dim, test_tr.element_size())
    ws = workspace(nbytes) if workspace is not None else torch.empty((nbytes,), dtype=torch.uint8, device=test_tr.device)
    _call(_typed("ktf_plda_trials", test_tr), test_tr.device, L.ptr(test_tr), N, L.ptr(enroll_tr), M, dim, L.ptr(psi),
          L.ptr(enroll_num_examples), L.ptr(pairs), T, L.ptr(scores), L.ptr(ws), ws.numel())
    return scores


# ----------------------------------------------------------------------------- score normalisation (ktf_topn_stats_*, ktf_plda_cohort_*)
TOPN_ALL = (1 << 31) - 1            # the C-level top_n for "the whole row"


def _top_n(top_n):
    return TOPN_ALL if top_n is None else min(int(top_n), TOPN_ALL)


def topn_stats(x, top_n):
    """(mean, std) of the top_n largest entries of each row of x (R, C) fp32 / fp64 on the device (rows may be strided: a column
    slice of a wider matrix is read in place) -> two (R,) fp64 tensors. top_n None or >= C: the whole row."""
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"topn_stats: x must be a (R, C) fp32 or fp64 tensor, got {x.dtype} {tuple(x.shape)}")
    R, Cn = x.shape
    if R > 1 and not (x.stride(1) == 1 and x.stride(0) >= Cn) or R <= 1 and not x.is_contiguous():
        x = x.contiguous()
    ld = x.stride(0) if R > 1 else Cn
    mean = _new(x, R, dtype=torch.float64)
    std = _new(x, R, dtype=torch.float64)
    _call(_typed("ktf_topn_stats", x), x.device, L.ptr(x), R, Cn, ld, _top_n(top_n), L.ptr(mean), L.ptr(std))
    return mean, std


def plda_cohort_workspace_bytes(R, Cn, dim, dtype_bytes):
    """Bytes of workspace ktf_plda_cohort_stats_* needs for R rows against Cn cohort vectors."""
    return _size("ktf_plda_cohort_workspace_bytes", R, Cn, dim, dtype_bytes)


def plda_cohort_stats(rows_tr, cohort_tr, psi, counts, role, top_n, mean, std, workspace):
    """topn_stats of the PLDA scores of rows_tr (R, dim) against cohort_tr (C, dim) into mean / std (R,) fp64. role 0: the rows are
    tests, counts (C) or None belong to the cohort; role 1: the rows are classes with counts (R) or None. workspace: a uint8
    device tensor of at least plda_cohort_workspace_bytes."""
    R, dim = rows_tr.shape
    Cn = cohort_tr.shape[0]
    _call(_typed("ktf_plda_cohort_stats", rows_tr), rows_tr.device, L.ptr(rows_tr), R, L.ptr(cohort_tr), Cn, dim, L.ptr(psi), L.ptr(counts),
          int(role), _top_n(top_n), L.ptr(mean), L.ptr(std), L.ptr(workspace), workspace.numel())
    return mean, std


def _host_i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _host_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _fresh(device):
    """The `scratch(role, shape, dtype)` of a caller that gave none: a fresh allocation each call."""
    return lambda role, shape, dtype: torch.empty(shape, dtype=dtype, device=device)


def plda_dense_workspace_bytes(lengths, dim, target_energy):
    """Bytes of scratch ktf_plda_dense_* needs (lengths: host ints; target_energy None = no PCA)."""
    lens = _host_i32(lengths)
    t = L.PLDA_DENSE_NO_PCA if target_energy is None else float(target_energy)
    return _size("ktf_plda_dense_workspace_bytes", _host_ptr(lens), len(lens), int(dim), t)


def plda_dense(x, lengths, target_energy, A, offset, psi, mean64, Tinv64, psi64, normalize_length, simple_length_norm,
               scratch=None):
    """Dense per-recording scoring (ktf_plda_dense_*). x (S, dim) on the device, lengths host ints (R), target_energy None = no PCA.
    -> (scores: the R blocks n_r x n_r packed in one 1-D tensor, dims (R,) int32, status (1,) int32 -- the device word the caller
    reads once). `scratch(role, shape, dtype)` hands out workspace tensors (a fresh allocation each call without it)."""
    S, dim = x.shape
    lens = _host_i32(lengths)
    R = len(lens)
    t = L.PLDA_DENSE_NO_PCA if target_energy is None else float(target_energy)
    nbytes = plda_dense_workspace_bytes(lens, dim, target_energy)
    get = scratch or _fresh(x.device)
    ws = get("plda_dense_ws", (nbytes,), torch.uint8)
    status = get("plda_dense_status", (1,), torch.int32)
    lens_dev = get("plda_dense_lengths", (R,), torch.int32)
    lens_dev.copy_(torch.from_numpy(lens))
    scores = _new(x, int(np.sum(lens.astype(np.int64) ** 2)))
    dims = _new(x, R, dtype=torch.int32)
    _call(_typed("ktf_plda_dense", x), x.device, L.ptr(x), S, dim, _host_ptr(lens), L.ptr(lens_dev), R, t, L.ptr(A), L.ptr(offset),
          L.ptr(psi), L.ptr(mean64), L.ptr(Tinv64), L.ptr(psi64), int(normalize_length), int(simple_length_norm), L.ptr(scores),
          L.ptr(dims), L.ptr(ws), ws.numel(), L.ptr(status))
    return scores, dims, status


def ahc_workspace_bytes(lengths, dtype_bytes):
    """Bytes of scratch ktf_ahc_* needs (lengths: host ints)."""
    lens = _host_i32(lengths)
    return _size("ktf_ahc_workspace_bytes", _host_ptr(lens), len(lens), int(dtype_bytes))


def ahc(scores, lengths, threshold, min_clusters, max_spk_fraction, read_costs, scratch=None):
    """Agglomerative clustering (ktf_ahc_*) of R packed blocks: scores 1-D, the blocks lengths[r]^2 one after another (as
    plda_dense returns them), lengths host ints, min_clusters None (1) or host ints (R). -> (labels (S,) int32, counts (R,) int32).
    `scratch(role, shape, dtype)` hands out workspace tensors (a fresh allocation each call without it)."""
    lens = _host_i32(lengths)
    R = len(lens)
    nbytes = ahc_workspace_bytes(lens, scores.element_size())
    get = scratch or _fresh(scores.device)
    ws = get("ahc_ws", (nbytes,), torch.uint8)
    meta = get("ahc_lengths", (2 * R,), torch.int32)          # lengths, then min_clusters
    host = np.concatenate([lens, np.ones(R, np.int32) if min_clusters is None else np.asarray(min_clusters, np.int32)])
    meta.copy_(torch.from_numpy(host))
    labels = _new(scores, int(lens.astype(np.int64).sum()), dtype=torch.int32)
    counts = _new(scores, R, dtype=torch.int32)
    _call(_typed("ktf_ahc", scores), scores.device, L.ptr(scores), _host_ptr(lens), L.ptr(meta), R, int(bool(read_costs)), float(threshold),
          L.ptr(meta[R:]) if min_clusters is not None else None, float(max_spk_fraction), L.ptr(labels), L.ptr(counts), L.ptr(ws),
          ws.numel())
    return labels, counts


def split_bf16(src, D, planes, lens=None):
    """fp32 (B,T,ld_src) rows -> planes (2,B,T,ld) bf16: hi = bf16(v), lo = bf16(v - hi); pad columns zero. `lens`: only the rows
    t < lens[b] are converted (the consumers never read the rest)."""
    lib = L.load()
    with L.on_device(src.device):
        if lens is None:
            rc = lib.ktf_split_bf16(L.ptr(src), src.shape[0] * src.shape[1], D, src.stride(1), L.ptr(planes[0]), L.ptr(planes[1]), planes.shape[-1],
                                    L.stream_ptr())
        else:
            rc = lib.ktf_split_bf16_rows(L.ptr(src), src.shape[0], src.shape[1], D, src.stride(1), L.ptr(lens), L.ptr(planes[0]), L.ptr(planes[1]),
                                         planes.shape[-1], L.stream_ptr())
    L.check(rc, "ktf_split_bf16")
    return planes


def _planes(xp):
    """(hi, lo, B, T, ldx) of a (2,B,T,ldx) pair of bf16 planes."""
    if xp.dim() != 4 or xp.shape[0] != 2:
        raise ValueError(f"expected a (2, B, T, ldx) pair of bf16 planes, got shape {tuple(xp.shape)}")
    return xp[0], xp[1], xp.shape[1], xp.shape[2], xp.stride(2)


def tdnn_split(xp, lens, desc, w, w_lo, bias, scale, shift, y, y_lo=None, out_lens=None):
    """xp: (2,B,T,ldx) bf16 hi/lo planes. y: (B,Tout,ldy) bf16 plane (+ y_lo) or fp32."""
    lib = L.load()
    hi, lo, B, T, ldx = _planes(xp)
    with L.on_device(xp.device):
        rc = lib.ktf_tdnn_split(L.ptr(hi), L.ptr(lo), B, T, ldx, L.ptr(lens), C.byref(desc), L.ptr(w), L.ptr(w_lo),
                                L.ptr(bias), L.ptr(scale), L.ptr(shift), L.ptr(y), L.ptr(y_lo), y.stride(1), L.ptr(out_lens),
                                L.stream_ptr())
    L.check(rc, "ktf_tdnn_split")
    return y


def row_starts(lens, B, T, out):
    """out (B + 1,) int32, out[0] == 0 -> the exclusive prefix sums of the utterance lengths (all T when lens is None):
    ktf_tdnn_split_flat's row map."""
    if lens is None:
        out[1:] = torch.arange(1, B + 1, dtype=torch.int32, device=out.device) * int(T)
    else:
        torch.cumsum(lens, 0, dtype=torch.int32, out=out[1:])
    return out


class FlatRows:
    """Row bookkeeping of a batch on flat row tiles: `starts` (B + 1,) int32 prefix sums of the lengths, `map` the per-row table
    ktf_flat_row_map makes from them (or None: every workgroup derives its entries itself)."""

    def __init__(self, starts, map=None):
        self.starts, self.map = starts, map


def flat_rows(lens, B, T, get):
    """FlatRows of a batch: `get(role, shape, dtype)` hands out the two buffers (a workspace)."""
    lib = L.load()
    starts = row_starts(lens, B, T, get("row_starts", (B + 1,), torch.int32))
    table = get("row_map", (int(lib.ktf_flat_row_map_rows(B, T)), 4), torch.int32)
    with L.on_device(starts.device):
        rc = lib.ktf_flat_row_map(L.ptr(starts), B, T, L.ptr(table), L.stream_ptr())
    L.check(rc, "ktf_flat_row_map")
    return FlatRows(starts, table)


def _flat(starts):
    return (starts.starts, starts.map) if isinstance(starts, FlatRows) else (starts, None)


def tdnn_split_flat(xp, starts, desc, w, w_lo, bias, scale, shift, y, y_lo=None):
    """tdnn_split with M-tiles over the batch's valid rows laid end to end (`starts` = row_starts(lens, ...) or flat_rows(...)): short
    utterances."""
    lib = L.load()
    hi, lo, B, T, ldx = _planes(xp)
    starts, rmap = _flat(starts)
    with L.on_device(xp.device):
        rc = lib.ktf_tdnn_split_flat(L.ptr(hi), L.ptr(lo), B, T, ldx, L.ptr(starts), L.ptr(rmap), C.byref(desc), L.ptr(w), L.ptr(w_lo),
                                     L.ptr(bias), L.ptr(scale), L.ptr(shift), L.ptr(y), L.ptr(y_lo), y.stride(1), L.stream_ptr())
    L.check(rc, "ktf_tdnn_split_flat")
    return y


def tdnn_split_stats(xp, lens, desc, w, w_lo, bias, scale, shift, sums, zero=True):
    lib = L.load()
    hi, lo, B, T, ldx = _planes(xp)
    with L.on_device(xp.device):
        if zero:
            sums.zero_()
        rc = lib.ktf_tdnn_split_stats(L.ptr(hi), L.ptr(lo), B, T, ldx, L.ptr(lens), C.byref(desc), L.ptr(w),
                                      L.ptr(w_lo), L.ptr(bias), L.ptr(scale), L.ptr(shift), L.ptr(sums), L.stream_ptr())
    L.check(rc, "ktf_tdnn_split_stats")
    return sums


def flat_stats_slots(T):
    return int(L.load().ktf_flat_stats_slots(int(T)))


def tdnn_split_flat_stats(xp, starts, desc, w, w_lo, bias, scale, shift, sums, zero=False):
    """tdnn_split_stats on flat row tiles (`starts` = row_starts(lens, ...)). sums: (B, flat_stats_slots(T), 2, units) fp64 with
    KTF_TDNN_DET_STATS in desc.flags (not zeroed: stats_finalize_flat reads the slots that were written), else (B, 2, units), zero=True."""
    lib = L.load()
    hi, lo, B, T, ldx = _planes(xp)
    starts, rmap = _flat(starts)
    with L.on_device(xp.device):
        if zero:
            sums.zero_()
        rc = lib.ktf_tdnn_split_flat_stats(L.ptr(hi), L.ptr(lo), B, T, ldx, L.ptr(starts), L.ptr(rmap), C.byref(desc), L.ptr(w), L.ptr(w_lo),
                                           L.ptr(bias), L.ptr(scale), L.ptr(shift), L.ptr(sums), L.stream_ptr())
    L.check(rc, "ktf_tdnn_split_flat_stats")
    return sums


def stats_finalize_flat(sums, starts, T, D, include_std, eps, out, slots):
    """sums (B, slots, 2, D) fp64 of tdnn_split_flat_stats -> out (B, ld) mean | std."""
    lib = L.load()
    B = sums.shape[0]
    starts, _ = _flat(starts)
    with L.on_device(sums.device):
        rc = lib.ktf_stats_finalize_flat(L.ptr(sums), slots, L.ptr(starts), T, B, D, int(include_std), eps, L.ptr(out), out.stride(0),
                                         L.stream_ptr())
    L.check(rc, "ktf_stats_finalize_flat")
    return out


def mx_planes(src, D, lens, planes):
    """fp32 (B,T,ld) rows -> the four KTF_GEMM_F16MX planes (mx.Planes); rows >= lens[b] are left unwritten."""
    lib = L.load()
    B, T = src.shape[0], src.shape[1]
    with L.on_device(src.device):
        rc = lib.ktf_mx_planes(L.ptr(src), B, T, D, src.stride(1), L.ptr(lens), L.ptr(planes.xh), L.ptr(planes.xl4), L.ptr(planes.x4),
                               L.ptr(planes.xs), L.stream_ptr())
    L.check(rc, "ktf_mx_planes")
    return planes


def tdnn_mx(xp, lens, desc, wh, wq, bias, scale, shift, y):
    """xp: mx.Planes. y: mx.Planes (the next layer's input) or an fp32 tensor, (B, tdnn_out_len(T), ...) either way."""
    lib = L.load()
    B, T, _ = xp.shape
    planes = not isinstance(y, torch.Tensor)
    with L.on_device(xp.device):
        rc = lib.ktf_tdnn_mx(L.ptr(xp.xh), L.ptr(xp.xl4), L.ptr(xp.x4), L.ptr(xp.xs), B, T, L.ptr(lens), C.byref(desc), L.ptr(wh),
                             L.ptr(wq), L.ptr(bias), L.ptr(scale), L.ptr(shift),
                             L.ptr(y.xh) if planes else None, L.ptr(y.xl4) if planes else None, L.ptr(y.x4) if planes else None,
                             L.ptr(y.xs) if planes else None, None if planes else L.ptr(y), 0 if planes else y.stride(1), L.stream_ptr())
    L.check(rc, "ktf_tdnn_mx")
    return y


def tdnn_mx_flat(xp, rows, desc, wh, wq, bias, scale, shift, y):
    """tdnn_mx with a plane output on flat row tiles (`rows` = flat_rows(lens, ...)): the same planes, bit for bit."""
    lib = L.load()
    B, T, _ = xp.shape
    with L.on_device(xp.device):
        rc = lib.ktf_tdnn_mx_flat(L.ptr(xp.xh), L.ptr(xp.xl4), L.ptr(xp.x4), L.ptr(xp.xs), B, T, L.ptr(rows.starts), L.ptr(rows.map), C.byref(desc),
                                  L.ptr(wh), L.ptr(wq), L.ptr(bias), L.ptr(scale), L.ptr(shift), L.ptr(y.xh), L.ptr(y.xl4), L.ptr(y.x4),
                                  L.ptr(y.xs), L.stream_ptr())
    L.check(rc, "ktf_tdnn_mx_flat")
    return y


def tdnn_mx_flat_stats(xp, rows, desc, wh, wq, bias, scale, shift, sums, zero=False):
    """tdnn_mx_stats on flat row tiles; sums as for tdnn_split_flat_stats (finalize: stats_finalize_flat)."""
    lib = L.load()
    B, T, _ = xp.shape
    with L.on_device(xp.device):
        if zero:
            sums.zero_()
        rc = lib.ktf_tdnn_mx_flat_stats(L.ptr(xp.xh), L.ptr(xp.xl4), L.ptr(xp.x4), L.ptr(xp.xs), B, T, L.ptr(rows.starts), L.ptr(rows.map),
                                        C.byref(desc), L.ptr(wh), L.ptr(wq), L.ptr(bias), L.ptr(scale), L.ptr(shift), L.ptr(sums), L.stream_ptr())
    L.check(rc, "ktf_tdnn_mx_flat_stats")
    return sums


def tdnn_mx_stats(xp, lens, desc, wh, wq, bias, scale, shift, sums, zero=True):
    lib = L.load()
    B, T, _ = xp.shape
    with L.on_device(xp.device):
        if zero:
            sums.zero_()
        rc = lib.ktf_tdnn_mx_stats(L.ptr(xp.xh), L.ptr(xp.xl4), L.ptr(xp.x4), L.ptr(xp.xs), B, T, L.ptr(lens), C.byref(desc),
                                   L.ptr(wh), L.ptr(wq), L.ptr(bias), L.ptr(scale), L.ptr(shift), L.ptr(sums), L.stream_ptr())
    L.check(rc, "ktf_tdnn_mx_stats")
    return sums


def stats_finalize(sums, lens, T, D, include_std, eps, out, slots=0, slot_rows=128):
    """sums (B,2,D) [slots == 0] or (B,slots,2,D) fp64 (one slot per `slot_rows` rows) -> out (B, ld) mean | std."""
    lib = L.load()
    B = sums.shape[0]
    with L.on_device(sums.device):
        if slots:
            rc = lib.ktf_stats_finalize_slots(L.ptr(sums), slots, int(slot_rows), L.ptr(lens), T, B, D, int(include_std), eps, L.ptr(out),
                                              out.stride(0), L.stream_ptr())
        else:
            rc = lib.ktf_stats_finalize(L.ptr(sums), L.ptr(lens), T, B, D, int(include_std), eps, L.ptr(out), out.stride(0),
                                        L.stream_ptr())
    L.check(rc, "ktf_stats_finalize")
    return out


def affine_act(x, act, scale=None, shift=None):
    lib = L.load()
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty_like(x)
    with L.on_device(x.device):
        rc = lib.ktf_affine_act_f32(L.ptr(x), rows, D, act, L.ptr(scale), L.ptr(shift), L.ptr(y), L.stream_ptr())
    L.check(rc, "ktf_affine_act_f32")
    return y


def activation_(y, lens, act, scale=None, shift=None):
    """In place over the rows t < lens[b] of y (B, T, D) fp32: y = act(y) * scale + shift (any L.ACT_*, softmax over D)."""
    lib = L.load()
    B, T, D = y.shape
    assert y.dtype == torch.float32 and y.stride(2) == 1 and y.stride(0) == T * y.stride(1)
    with L.on_device(y.device):
        rc = lib.ktf_activation_f32(L.ptr(y), B, T, D, y.stride(1), L.ptr(lens), act, L.ptr(scale), L.ptr(shift), L.stream_ptr())
    L.check(rc, "ktf_activation_f32")
    return y


def pair_encode(t):
    """fp32 tensor -> the KTF_BF16P pairs of its values, as a float32 tensor of the same shape (raw bits: bits 0-15 = bf16(v), round
    to nearest even, bits 16-31 = bf16(v - bf16(v)))."""
    t = t.to(torch.float32).contiguous()
    hi = t.to(torch.bfloat16)
    lo = (t - hi.to(torch.float32)).to(torch.bfloat16)
    bits = (hi.view(torch.int16).to(torch.int32) & 0xFFFF) | (lo.view(torch.int16).to(torch.int32) << 16)
    return bits.view(torch.float32)


def pair_decode(t):
    """The values a KTF_BF16P tensor holds (hi + lo), fp32."""
    bits = t.contiguous().view(torch.int32)
    hi = (bits << 16).view(torch.float32)
    lo = (bits & ~0xFFFF).view(torch.float32)
    return hi + lo


def convert_pad(src, D, dst):
    """src (..., ld_src) / dst (..., ld_dst) 2-D-viewable row-major tensors; copies D columns, zero-fills the pad."""
    lib = L.load()
    rows = src.numel() // src.shape[-1]
    sd, dd = L.ktf_dtype(src.dtype), L.ktf_dtype(dst.dtype)
    with L.on_device(src.device):
        rc = lib.ktf_convert_pad(L.ptr(src), sd, rows, D, src.shape[-1], L.ptr(dst), dd, dst.shape[-1], L.stream_ptr())
    L.check(rc, "ktf_convert_pad")
    return dst


# The pooling / post / tail entry points take a base pointer and at most one row stride per tensor: a view they cannot express -- a time
# slice x[:, :40] of a longer batch, a transposed matrix, a last stride other than 1 -- would make the kernel read other memory
# without a word. The wrappers refuse it by name before the library is called. (A dimension of one element has no stride to speak of.)
def _need_dense(name, t):
    """t (or None) must be contiguous: the library gets its base pointer only."""
    if t is not None and not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous tensor is expected, got shape {tuple(t.shape)} with strides {tuple(t.stride())}")


def _need_rows(name, t):
    """t (..., rows, ld): unit stride along the last axis, the leading axes dense over the row stride -- the library gets the base
    pointer and t.stride(-2)."""
    n = t.dim()
    ok = t.shape[-1] <= 1 or t.stride(-1) == 1
    if ok and n == 3 and t.shape[0] > 1 and t.shape[1] > 0:
        ok = t.stride(0) == t.shape[1] * t.stride(1)
    if not ok:
        raise ValueError(f"{name}: rows of unit stride laid end to end are expected, got shape {tuple(t.shape)} with strides {tuple(t.stride())}")


def stats_pool(x, D, lens, input_period, include_std, eps, out):
    """x (B,T,ldx) fp32/bf16; out (B, ld_out) fp32 preallocated."""
    lib = L.load()
    B, T = x.shape[0], x.shape[1]
    _need_rows("x", x)
    _need_rows("out", out)
    _need_dense("lens", lens)
    dt = L.ktf_dtype(x.dtype)
    with L.on_device(x.device):
        rc = lib.ktf_stats_pool(L.ptr(x), dt, B, T, D, x.stride(1), L.ptr(lens), input_period, int(include_std), eps,
                                L.ptr(out), out.stride(0), L.stream_ptr())
    L.check(rc, "ktf_stats_pool")
    return out


def stats_pool_windowed(x, left, right, input_period, output_period, start, T_out, include_std, eps):
    lib = L.load()
    B, T, D = x.shape
    _need_dense("x", x)
    out = torch.empty((B, T_out, 2 * D if include_std else D), dtype=torch.float32, device=x.device)
    with L.on_device(x.device):
        rc = lib.ktf_stats_pool_windowed_f32(L.ptr(x), B, T, D, left, right, input_period, output_period, start, T_out,
                                             int(include_std), eps, L.ptr(out), L.stream_ptr())
    L.check(rc, "ktf_stats_pool_windowed_f32")
    return out


def xvec_post(x, mean, A, off, out=None):
    lib = L.load()
    B, in_dim = x.shape
    out_dim = A.shape[1]
    for name, t in (("x", x), ("mean", mean), ("A", A), ("off", off), ("out", out)):
        _need_dense(name, t)
    if out is None:
        out = torch.empty((B, out_dim), dtype=torch.float32, device=x.device)
    with L.on_device(x.device):
        rc = lib.ktf_xvec_post_f32(L.ptr(x), B, in_dim, out_dim, L.ptr(mean), L.ptr(A), L.ptr(off), L.ptr(out), L.stream_ptr())
    L.check(rc, "ktf_xvec_post_f32")
    return out


def xvec_tail(pooled, sums, slots, lens, T, D, include_std, eps, W, bias, units, mean, A, off, partial, counters, out, h_out=None, group=1,
              slot_rows=128, skip_empty=False):
    """Fused tail (ktf_xvec_tail_f32): pooled (B, ld) fp32 rows OR fp64 sums -> tdnn6 -> mean-sub -> LDA -> length norm, one launch."""
    lib = L.load()
    B = out.shape[0]
    if (pooled is None) == (sums is None):
        raise ValueError("pooled / sums: exactly one of the two is expected")
    src = pooled if pooled is not None else sums
    if pooled is not None:
        _need_rows("pooled", pooled)
    _need_rows("W", W)
    for name, t in (("sums", sums), ("lens", lens), ("bias", bias), ("mean", mean), ("A", A), ("off", off), ("partial", partial),
                    ("counters", counters), ("out", out), ("h_out", h_out)):
        _need_dense(name, t)
    with L.on_device(src.device):
        rc = lib.ktf_xvec_tail_f32(L.ptr(pooled), pooled.stride(0) if pooled is not None else 0, L.ptr(sums), int(slots), int(slot_rows), L.ptr(lens), int(T), B,
                                   int(D), int(include_std), float(eps), L.ptr(W), W.stride(0), L.ptr(bias), int(units), L.ptr(mean), L.ptr(A),
                                   L.ptr(off), A.shape[1], L.ptr(partial), L.ptr(counters), L.ptr(out), L.ptr(h_out), int(group),
                                   L.TAIL_SKIP_EMPTY if skip_empty else 0, L.stream_ptr())
    L.check(rc, "ktf_xvec_tail_f32")
    return out


def plda(x, A, offset, psi, normalize_length, simple_length_norm, want_scores=True):
    lib = L.load()
    B, dim = x.shape
    tr = torch.empty_like(x)
    scores = torch.empty((B, B), dtype=x.dtype, device=x.device) if want_scores else None
    fn = lib.ktf_plda_f64 if x.dtype == torch.float64 else lib.ktf_plda_f32
    with L.on_device(x.device):
        rc = fn(L.ptr(x), B, dim, L.ptr(A), L.ptr(offset), L.ptr(psi), int(normalize_length), int(simple_length_norm),
                L.ptr(tr), L.ptr(scores), L.stream_ptr())
    L.check(rc, "ktf_plda")
    return scores, tr


# ----------------------------------------------------------------------------- sliding-window diarization front end (ktf_diar_*)
def diar_segments(mfcc, frames, offsets, vad_cfg, seg_work, counts):
    """Energy-VAD speech segments of R recordings laid end to end in mfcc (F, D) (ktf_diar_segments). frames: host ints (R),
    offsets: device int32 (R + 1). Writes seg_work (2F int32) and counts[:R]."""
    fr = _host_i32(frames)
    _call("ktf_diar_segments", mfcc.device, L.ptr(mfcc), mfcc.shape[-1], _host_ptr(fr), L.ptr(offsets), len(fr), C.byref(vad_cfg),
          L.ptr(seg_work), L.ptr(counts))


def diar_windows(seg_work, frames, offsets, W, P, M, win_work, counts):
    """Windows of every segment in seg_work (ktf_diar_windows): writes win_work (2F int32) and counts[R:]."""
    fr = _host_i32(frames)
    _call("ktf_diar_windows", seg_work.device, L.ptr(seg_work), _host_ptr(fr), L.ptr(offsets), len(fr), int(W), int(P), int(M),
          L.ptr(win_work), L.ptr(counts))


def diar_compact(seg_work, win_work, counts, frames, offsets, G, S):
    """-> (segments (G, 3), windows (S, 3)) int32 device tables (ktf_diar_compact)."""
    fr = _host_i32(frames)
    segs = _new(seg_work, G, 3, dtype=torch.int32)
    wins = _new(seg_work, S, 3, dtype=torch.int32)
    _call("ktf_diar_compact", seg_work.device, L.ptr(seg_work), L.ptr(win_work), L.ptr(counts), _host_ptr(fr), L.ptr(offsets), len(fr),
          int(G), int(S), L.ptr(segs), L.ptr(wins))
    return segs, wins


def diar_segment_cmn(mfcc, frames, offsets, segments, cmvn_cfg, out, work):
    """CMN of every segment's rows of mfcc (F, D) into out (F, D) at the same rows (ktf_diar_segment_cmn)."""
    fr = _host_i32(frames)
    _call("ktf_diar_segment_cmn", mfcc.device, L.ptr(mfcc), mfcc.shape[-1], _host_ptr(fr), L.ptr(offsets), len(fr), L.ptr(segments),
          segments.shape[0], C.byref(cmvn_cfg), L.ptr(out), L.ptr(work))


def diar_gather(cmn, D, frames, offsets, windows, w0, n, out, lens):
    """Windows [w0, w0 + n) of the table -> out (n, Tw, ldo) float32 / bfloat16 and lens (n,) (ktf_diar_gather)."""
    fr = _host_i32(frames)
    _call("ktf_diar_gather", cmn.device, L.ptr(cmn), int(D), _host_ptr(fr), L.ptr(offsets), len(fr), L.ptr(windows), windows.shape[0],
          int(w0), int(n), out.shape[1], L.ptr(out), L.ktf_dtype(out.dtype), out.stride(1), L.ptr(lens))


def ivector_post(x, W, gconst, num_gselect, min_post):
    """gmm-global-get-post on frames x (F, D) fp32 (row stride x.stride(0)): W (2D, I), gconst (I) fp32 on the same device ->
    (gauss (F, n) int32, post (F, n) fp32), ktf_ivector_post_f32."""
    F, D = x.shape
    n = int(num_gselect)
    gauss = _new(x, F, n, dtype=torch.int32)
    post = _new(x, F, n, dtype=torch.float32)
    _call("ktf_ivector_post_f32", x.device, L.ptr(x), F, D, _ld(x), L.ptr(W), L.ptr(gconst), gconst.shape[0], n, float(min_post),
          L.ptr(gauss), L.ptr(post))
    return gauss, post


def ivector_workspace_bytes(B, I, D, S):
    return _size("ktf_ivector_workspace_bytes", int(B), int(I), int(D), int(S))


def ivector_extract(x, offsets, gauss, post, posterior_scale, acoustic_weight, max_count, sigma_inv_M, U, prior_offset,
                    dtype=torch.float32):
    """Stats, linear / quadratic terms and the solve (ktf_ivector_extract) for B = offsets.numel() - 1 utterances whose frames lie
    end to end in x (F, D). -> (B, S) i-vectors of `dtype` (float32 or float64)."""
    F, D = x.shape
    B = offsets.numel() - 1
    I, S = U.shape[0], sigma_inv_M.shape[1]
    out = _new(x, B, S, dtype=dtype)
    ws = _workspace("ktf_ivector_workspace_bytes", B, I, D, S, device=x.device)
    _call("ktf_ivector_extract", x.device, L.ptr(x), F, D, _ld(x), L.ptr(offsets), B, L.ptr(gauss), L.ptr(post), gauss.shape[1],
          float(posterior_scale), float(acoustic_weight), float(max_count), L.ptr(sigma_inv_M), L.ptr(U), I, S, float(prior_offset),
          L.ptr(out), out.element_size(), L.ptr(ws), ws.numel())
    return out


def ivector_train_workspace_bytes(B, I, D, S):
    return _size("ktf_ivector_train_workspace_bytes", int(B), int(I), int(D), int(S))


def ivector_acc_stats(x, offsets, gauss, post, posterior_scale, sigma_inv_M, U, prior_offset, gamma, Y, R, ivector_sum,
                      ivector_scatter, totals):
    """ivector-extractor-acc-stats for B = offsets.numel() - 1 utterances whose frames lie end to end in x (F, D), added in place to
    the fp64 device accumulators gamma (I), Y (I * D, S), R (I, P), ivector_sum (S), ivector_scatter (P), totals (2) =
    (num_ivectors, the sum of the utterances' marginal-likelihood scalars): ktf_ivector_acc_stats."""
    F, D = x.shape
    B = offsets.numel() - 1
    I, S = U.shape[0], sigma_inv_M.shape[1]
    ws = _workspace("ktf_ivector_train_workspace_bytes", B, I, D, S, device=x.device)
    _call("ktf_ivector_acc_stats", x.device, L.ptr(x), F, D, _ld(x), L.ptr(offsets), B, L.ptr(gauss), L.ptr(post), gauss.shape[1],
          float(posterior_scale), L.ptr(sigma_inv_M), L.ptr(U), I, S, float(prior_offset), L.ptr(gamma), L.ptr(Y), L.ptr(R),
          L.ptr(ivector_sum), L.ptr(ivector_scatter), L.ptr(totals), L.ptr(ws), ws.numel())


def ivector_acc_second_order(x, gauss, post, posterior_scale, Ssec):
    """Ssec (I, D, D) fp64 += sum_t p'_ti x_t x_t^T over the frames x (F, D) and their slots gauss / post (F, n), bit-identical run
    to run: ktf_ivector_acc_second_order."""
    F, D = x.shape
    I, n = Ssec.shape[0], gauss.shape[1]
    ws = _workspace("ktf_ivector_acc2_workspace_bytes", F, I, n, device=x.device)
    _call("ktf_ivector_acc_second_order", x.device, L.ptr(x), F, D, _ld(x), L.ptr(gauss), L.ptr(post), n, float(posterior_scale), I,
          L.ptr(Ssec), L.ptr(ws), ws.numel())


def atb_f64(A, B, C):
    """C (M, N) += A^T B in place: A (K, M), B (K, N), C fp64 device matrices with unit inner strides (ktf_atb_f64, fp64 MFMA)."""
    K, M = A.shape
    N = B.shape[1]
    if B.shape[0] != K or tuple(C.shape) != (M, N) or any(t.dtype != torch.float64 or (t.numel() and t.stride(1) != 1) for t in (A, B, C)):
        raise ValueError("atb_f64: need fp64 A (K, M), B (K, N), C (M, N) with unit inner strides")
    _call("ktf_atb_f64", C.device, L.ptr(A), _ld(A), L.ptr(B), _ld(B), L.ptr(C), C.stride(0), M, N, K)
    return C


def fgmm_workspace_bytes(F, I, D, n):
    return _size("ktf_fgmm_workspace_bytes", int(F), int(I), int(D), int(n))


def fgmm_post(x, gselect, means_invcovars, inv_covars, gconst, min_post):
    """fgmm-global-gselect-to-post on frames x (F, D) fp32 (row stride x.stride(0)) and the lists gselect (F, n) int32 (entries
    outside [0, I) skipped): means_invcovars (I, D), inv_covars (I, D, D) full symmetric, gconst (I), fp32 on the same device ->
    (gauss (F, n) int32, post (F, n) fp32), ktf_fgmm_post_f32."""
    F, D = x.shape
    n = gselect.shape[1]
    I = gconst.shape[0]
    gauss = _new(x, F, n, dtype=torch.int32)
    post = _new(x, F, n, dtype=torch.float32)
    ws = _workspace("ktf_fgmm_workspace_bytes", F, I, D, n, device=x.device)
    _call("ktf_fgmm_post_f32", x.device, L.ptr(x), F, D, _ld(x), L.ptr(gselect), n, L.ptr(means_invcovars), L.ptr(inv_covars),
          L.ptr(gconst), I, float(min_post), L.ptr(gauss), L.ptr(post), L.ptr(ws), ws.numel())
    return gauss, post


def fgmm_post_ll(x, gselect, means_invcovars, inv_covars, gconst, min_post, want_loglike=True):
    """fgmm_post with the frames' log-likelihoods (before pruning) -> (gauss, post, loglike (F) fp32 or None): ktf_fgmm_post_ll_f32."""
    F, D = x.shape
    n = gselect.shape[1]
    I = gconst.shape[0]
    gauss = _new(x, F, n, dtype=torch.int32)
    post = _new(x, F, n, dtype=torch.float32)
    ll = _new(x, F, dtype=torch.float32) if want_loglike else None
    ws = _workspace("ktf_fgmm_workspace_bytes", F, I, D, n, device=x.device)
    _call("ktf_fgmm_post_ll_f32", x.device, L.ptr(x), F, D, _ld(x), L.ptr(gselect), n, L.ptr(means_invcovars), L.ptr(inv_covars),
          L.ptr(gconst), I, float(min_post), L.ptr(gauss), L.ptr(post), L.ptr(ll), L.ptr(ws), ws.numel())
    return gauss, post, ll


# ----------------------------------------------------------------------------- UBM training statistics (ktf_gmm_*)
def gmm_post_preselect(x, gselect, means_invvars, inv_vars, gconst, valid=None):
    """gmm-global-acc-stats --gselect's E-step on frames x (F, D) fp32 and lists gselect (F, n) int32: -> (post (F, n) fp32 in the
    list's slot order, loglike (F) fp32); `valid` (1,) int32 on the device is increased by the frames with a non-empty list."""
    F, D = x.shape
    n = gselect.shape[1]
    post = _new(x, F, n, dtype=torch.float32)
    ll = _new(x, F, dtype=torch.float32)
    _call("ktf_gmm_post_preselect_f32", x.device, L.ptr(x), F, D, _ld(x), L.ptr(gselect), n, L.ptr(means_invvars), L.ptr(inv_vars),
          L.ptr(gconst), gconst.shape[0], L.ptr(post), L.ptr(ll), L.ptr(valid))
    return post, ll


def gmm_post_dense_workspace_bytes(F, I):
    return _size("ktf_gmm_post_dense_workspace_bytes", int(F), int(I))


def gmm_post_dense(x, W, gconst):
    """The dense E-step of gmm-global-init-from-feats on frames x (F, D) fp32: W (2D, I), gconst (I) as ivector_post takes them ->
    (P (F, I) fp64, Xaug (F, 2D + 1) fp64 = [1, x, x^2], loglike (F) fp32): ktf_gmm_post_dense_f32."""
    F, D = x.shape
    I = gconst.shape[0]
    P = _new(x, F, I, dtype=torch.float64)
    Xaug = _new(x, F, 2 * D + 1, dtype=torch.float64)
    ll = _new(x, F, dtype=torch.float32)
    ws = _workspace("ktf_gmm_post_dense_workspace_bytes", F, I, device=x.device)
    _call("ktf_gmm_post_dense_f32", x.device, L.ptr(x), F, D, _ld(x), L.ptr(W), L.ptr(gconst), I, L.ptr(P), L.ptr(Xaug), L.ptr(ll),
          L.ptr(ws), ws.numel())
    return P, Xaug, ll


def gmm_acc_workspace_bytes(F, I, D, n, full):
    return _size("ktf_gmm_acc_workspace_bytes", int(F), int(I), int(D), int(n), int(bool(full)))


def gmm_acc(x, gauss, post, occ, mean_acc, second_acc):
    """GMM EM statistics on the pairs gauss / post (F, n) of frames x (F, D) fp32, added in place to the fp64 device accumulators occ
    (I), mean_acc (I, D) and second_acc: var_acc (I, D) = the diagonal form, cov_acc (I, D, D) = the full form. ktf_gmm_acc_f64."""
    F, D = x.shape
    I, n = occ.shape[0], gauss.shape[1]
    full = second_acc.dim() == 3
    if tuple(gauss.shape) != (F, n) or tuple(post.shape) != (F, n) or tuple(mean_acc.shape) != (I, D) or \
            tuple(second_acc.shape) != ((I, D, D) if full else (I, D)) or \
            any(t.dtype != torch.float64 or not t.is_contiguous() for t in (occ, mean_acc, second_acc)) or \
            gauss.dtype != torch.int32 or post.dtype != torch.float32 or not gauss.is_contiguous() or not post.is_contiguous():
        raise ValueError("gmm_acc: need gauss int32 / post fp32 (F, n) and contiguous fp64 occ (I), mean_acc (I, D), "
                         "second_acc (I, D) or (I, D, D)")
    ws = _workspace("ktf_gmm_acc_workspace_bytes", F, I, D, n, int(full), device=x.device)
    _call("ktf_gmm_acc_f64", x.device, L.ptr(x), F, D, _ld(x), L.ptr(gauss), L.ptr(post), n, I, int(full), L.ptr(occ), L.ptr(mean_acc),
          L.ptr(second_acc), L.ptr(ws), ws.numel())


def add_deltas(x, lengths, coeffs, order, window):
    """add-deltas on x (B, T, D) fp32 with a unit inner stride; lengths (B,) int32 on the device or None; coeffs (order + 1,
    2 * order * window + 1) fp32 on the device -> (B, T, D * (order + 1)) fp32, ktf_add_deltas_f32."""
    B, T, D = x.shape
    out = _new(x, B, T, D * (order + 1), dtype=torch.float32)
    _call("ktf_add_deltas_f32", x.device, L.ptr(x), B, T, D, x.stride(0) if B > 1 else T * max(x.stride(1), D),
          x.stride(1) if T > 1 else D, L.ptr(lengths), L.ptr(coeffs), int(order), int(window), L.ptr(out))
    return out


# ----------------------------------------------------------------------------- back-end training (ktf_train_*, ktf_plda_em_project)
def train_workspace(rows, D, device):
    """A uint8 device buffer for ktf_train_mean_* / ktf_train_gram_* over up to `rows` rows of dimension D."""
    return _workspace("ktf_train_workspace_bytes", int(rows), int(D), device=device)


def train_class_means(x, offsets, utts, S):
    """x (N, D) fp32, the CSR map offsets (S + 1) / utts on the device (int32) -> (means (S, D) fp64, counts (S,) int32)."""
    N, D = x.shape
    means = _new(x, S, D, dtype=torch.float64)
    counts = _new(x, S, dtype=torch.int32)
    _call("ktf_train_class_means", x.device, L.ptr(x), N, D, L.ptr(offsets), S, L.ptr(utts), utts.numel(), L.ptr(means), L.ptr(counts))
    return means, counts


def train_mean(y, ws):
    """Column means (D,) fp64 of y (rows, D) fp32 or fp64."""
    rows, D = y.shape
    out = _new(y, D, dtype=torch.float64)
    _call(_typed("ktf_train_mean", y), y.device, L.ptr(y), rows, D, L.ptr(out), L.ptr(ws), ws.numel())
    return out


def train_gram(y, ws, idx=None, center=None, weights=None):
    """G (D, D) fp64 = sum_r w_r (y[idx[r]] - c)(y[idx[r]] - c)^T; idx (device int32, None: every row), center (D,) and weights
    (one per listed row) device fp64 or None."""
    N, D = y.shape
    rows = idx.numel() if idx is not None else N
    G = _new(y, D, D, dtype=torch.float64)
    _call(_typed("ktf_train_gram", y), y.device, L.ptr(y), N, D, L.ptr(idx), rows, L.ptr(center), L.ptr(weights), L.ptr(G), L.ptr(ws),
          ws.numel())
    return G


def plda_em_project(mu, mbar, P, lam, counts):
    """One EM step's rows in the diagonal space: mu (S, D), mbar (D,), P (D, D), lam (D,) device fp64, counts (S,) int32 -> a, b."""
    S, D = mu.shape
    a = torch.empty_like(mu)
    b = torch.empty_like(mu)
    _call("ktf_plda_em_project", mu.device, L.ptr(mu), S, D, L.ptr(mbar), L.ptr(P), L.ptr(lam), L.ptr(counts), L.ptr(a), L.ptr(b))
    return a, b


# ----------------------------------------------------------------------------- VB-HMM resegmentation (ktf_vb_*)
def vb_post_workspace_bytes(F, I):
    return _size("ktf_vb_post_workspace_bytes", int(F), int(I))


def vb_post(x, W, gconst, num_slots, ll_scale, stat_scale, sparsity_thr, truncated):
    """Thresholded posteriors over all Gaussians on frames x (F, D) fp32: W (2D, I), gconst (I) as ivector_post takes them ->
    (gauss (F, n) int32, post (F, n) fp32, loglike (F) fp32); `truncated` (1,) int32 on the device is increased by the frames with
    more than n candidates: ktf_vb_post_f32."""
    F, D = x.shape
    n, I = int(num_slots), gconst.shape[0]
    gauss = _new(x, F, n, dtype=torch.int32)
    post = _new(x, F, n, dtype=torch.float32)
    ll = _new(x, F, dtype=torch.float32)
    ws = _workspace("ktf_vb_post_workspace_bytes", F, I, device=x.device)
    _call("ktf_vb_post_f32", x.device, L.ptr(x), F, D, _ld(x), L.ptr(W), L.ptr(gconst), I, n, float(ll_scale), float(stat_scale),
          float(sparsity_thr), L.ptr(gauss), L.ptr(post), L.ptr(ll), L.ptr(truncated), L.ptr(ws), ws.numel())
    return gauss, post, ll


def vb_bucket(gauss, I):
    """The (frame, slot) pairs of gauss (F, n) int32 bucketed by Gaussian in ascending pair order -> (start (I + 1), pairs (F n))
    int32: ktf_vb_bucket."""
    F, n = gauss.shape
    start = _new(gauss, I + 1, dtype=torch.int32)
    pairs = _new(gauss, F * n, dtype=torch.int32)
    ws = _workspace("ktf_vb_bucket_workspace_bytes", F, I, n, device=gauss.device)
    _call("ktf_vb_bucket", gauss.device, L.ptr(gauss), F, n, I, L.ptr(start), L.ptr(pairs), L.ptr(ws), ws.numel())
    return start, pairs


def vb_speaker_stats(x, offsets, boffsets, downsample, post, start, pairs, means, q):
    """Soft statistics of the N = offsets.numel() - 1 recordings in x (F, D): q (TB, K) fp64, means (I, D) fp64 -> (Nst (N K, I),
    Fst (N K, I D)) fp64: ktf_vb_speaker_stats."""
    F, D = x.shape
    N, (TB, K), I = offsets.numel() - 1, q.shape, means.shape[0]
    Nst = _new(x, N * K, I, dtype=torch.float64)
    Fst = _new(x, N * K, I * D, dtype=torch.float64)
    _call("ktf_vb_speaker_stats", x.device, L.ptr(x), F, D, _ld(x), L.ptr(offsets), L.ptr(boffsets), N, TB, int(downsample), L.ptr(post),
          post.shape[1], L.ptr(start), L.ptr(pairs), I, L.ptr(means), L.ptr(q), K, L.ptr(Nst), L.ptr(Fst))
    return Nst, Fst


def vb_speaker_update(Nst, Fst, Bm, U):
    """Nst (B, I), Fst (B, I D), Bm (I D, R), U (I, P) fp64 -> a (B, R), W (B, P) packed, kl (B), h (B, I D), g (B, I):
    ktf_vb_speaker_update."""
    B, I = Nst.shape
    R = Bm.shape[1]
    D = Bm.shape[0] // I
    P = R * (R + 1) // 2
    f = lambda *s: _new(Nst, *s, dtype=torch.float64)  # noqa: E731
    a, Wp, kl, h, g = f(B, R), f(B, P), f(B), f(B, I * D), f(B, I)
    ws = _workspace("ktf_vb_update_workspace_bytes", B, I, D, R, device=Nst.device)
    _call("ktf_vb_speaker_update", Nst.device, L.ptr(Nst), L.ptr(Fst), B, I, D, R, L.ptr(Bm), L.ptr(U), L.ptr(a), L.ptr(Wp), L.ptr(kl),
          L.ptr(h), L.ptr(g), L.ptr(ws), ws.numel())
    return a, Wp, kl, h, g


def vb_block_loglike(x, offsets, boffsets, downsample, TB, gauss, post, means, h, g, K):
    """lls (TB, K) fp64 of the blocks: ktf_vb_block_loglike."""
    F, D = x.shape
    N, I = offsets.numel() - 1, means.shape[0]
    lls = _new(x, TB, K, dtype=torch.float64)
    _call("ktf_vb_block_loglike", x.device, L.ptr(x), F, D, _ld(x), L.ptr(offsets), L.ptr(boffsets), N, TB, int(downsample), L.ptr(gauss),
          L.ptr(post), gauss.shape[1], I, L.ptr(means), L.ptr(h), L.ptr(g), int(K), L.ptr(lls))
    return lls


def _forward_backward(name, size, lls, boffsets, sp, loop_prob):
    TB, K = lls.shape
    N = boffsets.numel() - 1
    q, sp_out, tll = _new(lls, TB, K, dtype=torch.float64), _new(lls, N, K, dtype=torch.float64), _new(lls, N, dtype=torch.float64)
    ws = _workspace(size, TB, N, device=lls.device)
    _call(name, lls.device, L.ptr(lls), L.ptr(boffsets), N, TB, K, L.ptr(sp), float(loop_prob), L.ptr(q), L.ptr(sp_out), L.ptr(tll),
          L.ptr(ws), ws.numel())
    return q, sp_out, tll


def vb_forward_backward(lls, boffsets, sp, loop_prob):
    """lls (TB, K), sp (N, K) fp64, boffsets (N + 1) int32 -> (q (TB, K), sp_out (N, K), tll (N)) fp64: ktf_vb_forward_backward."""
    return _forward_backward("ktf_vb_forward_backward", "ktf_vb_fb_workspace_bytes", lls, boffsets, sp, loop_prob)


def vb_forward_backward_serial(lls, boffsets, sp, loop_prob):
    """The forward-backward in its serial form (one wave per recording walks every block), for tools/bench_vb.py to time the chunked
    scan against; the package itself never calls it. Arguments and results as vb_forward_backward: ktf_vb_forward_backward_serial."""
    return _forward_backward("ktf_vb_forward_backward_serial", "ktf_vb_fb_serial_workspace_bytes", lls, boffsets, sp, loop_prob)


def vb_loglike_sums(loglike, offsets):
    """gsum (N) fp64 = each recording's sum of loglike (F) fp32 in a fixed order of its own: ktf_vb_loglike_sums."""
    N = offsets.numel() - 1
    gsum = _new(loglike, N, dtype=torch.float64)
    _call("ktf_vb_loglike_sums", loglike.device, L.ptr(loglike), L.ptr(offsets), N, loglike.shape[0], L.ptr(gsum))
    return gsum


def vb_bound(gsum, tll, kl, stat_scale):
    """bound (N) fp64 = stat_scale gsum + tll + the recording's K entries of kl (N K) added in order: ktf_vb_bound."""
    N = gsum.shape[0]
    bound = _new(gsum, N, dtype=torch.float64)
    _call("ktf_vb_bound", gsum.device, L.ptr(gsum), L.ptr(tll), L.ptr(kl), N, kl.numel() // N, float(stat_scale), L.ptr(bound))
    return bound


# ----------------------------------------------------------------------------- VBx (ktf_vbx_*)
def vbx_prepare(x, phi):
    """x (TB, D), phi (D) fp64 -> (rho (TB, D) = x sqrt(phi), G (TB) = -(sum_d x^2 + D log 2 pi) / 2): ktf_vbx_prepare."""
    TB, D = x.shape
    rho = _new(x, TB, D, dtype=torch.float64)
    G = _new(x, TB, dtype=torch.float64)
    _call("ktf_vbx_prepare", x.device, L.ptr(x), TB, D, L.ptr(phi), L.ptr(rho), L.ptr(G))
    return rho, G


def vbx_speaker_update(gamma, rho, phi, fa_over_fb, offsets):
    """gamma (TB, K), rho (TB, D), phi (D) fp64, offsets (N + 1) int32 -> (alpha (N, K, D), invL (N, K, D), c (N, K), kl (N, K)); the
    rows of alpha and invL of a recording without windows are zero: ktf_vbx_speaker_update."""
    (TB, K), D, N = gamma.shape, rho.shape[1], offsets.numel() - 1
    dev = gamma.device
    alpha = torch.zeros((N, K, D), dtype=torch.float64, device=dev)
    invL = torch.zeros((N, K, D), dtype=torch.float64, device=dev)
    c = _new(gamma, N, K, dtype=torch.float64)
    kl = _new(gamma, N, K, dtype=torch.float64)
    ws = _workspace("ktf_vbx_update_workspace_bytes", TB, N, D, device=dev)
    _call("ktf_vbx_speaker_update", dev, L.ptr(gamma), L.ptr(rho), TB, D, K, L.ptr(offsets), N, L.ptr(phi), float(fa_over_fb), L.ptr(alpha),
          L.ptr(invL), L.ptr(c), L.ptr(kl), L.ptr(ws), ws.numel())
    return alpha, invL, c, kl


def vbx_loglike(rho, G, alpha, c, Fa, offsets):
    """lls (TB, K) fp64 = Fa (rho alpha^T - c + G) per recording: ktf_vbx_loglike."""
    TB, D = rho.shape
    N, K = c.shape
    lls = _new(rho, TB, K, dtype=torch.float64)
    _call("ktf_vbx_loglike", rho.device, L.ptr(rho), L.ptr(G), TB, D, K, L.ptr(offsets), N, L.ptr(alpha), L.ptr(c), float(Fa), L.ptr(lls))
    return lls


# ----------------------------------------------------------------------------- waveform augmentation (include/ktf_augment.h)
def _host_or_null(a):
    return _host_ptr(a) if a is not None and a.size else None


def aug_partition():
    """P: the partition size of the convolution, in samples."""
    return int(L.load().ktf_aug_partition())


def aug_tables(device):
    """The twiddle tables of the convolution's transforms, fp32 on `device`."""
    tables = torch.empty((_size("ktf_aug_tables_floats"),), dtype=torch.float32, device=device)
    _call("ktf_aug_tables", device, L.ptr(tables))
    return tables


def aug_rir_prepare(h, offsets, offsets_dev, fs, tables):
    """h: the bank's taps one RIR after another (fp32, device); offsets: host int32 (R + 1), offsets_dev the same on the device ->
    (meta (R, AUG_META) int32, spectra fp32): peak index, early window and partition spectra of every RIR."""
    offsets = _host_i32(offsets)
    R = offsets.size - 1
    meta = _new(h, R, L.AUG_META, dtype=torch.int32)
    spectra = _new(h, _size("ktf_aug_rir_spectra_floats", _host_ptr(offsets), R, int(fs)), dtype=torch.float32)
    _call("ktf_aug_rir_prepare", h.device, L.ptr(h), _host_ptr(offsets), L.ptr(offsets_dev), R, int(fs), L.ptr(tables), L.ptr(meta),
          L.ptr(spectra))
    return meta, spectra


def aug_workspace_bytes(n, rir_ids, rir_lengths, fs, num_additives):
    """Bytes of the workspace aug_convolve and aug_mix share for the rows n / rir_ids (host int32) of a bank with rir_lengths."""
    n, rir_ids, rir_lengths = _host_i32(n), _host_i32(rir_ids), _host_i32(rir_lengths)
    return _size("ktf_aug_workspace_bytes", _host_or_null(n), _host_or_null(rir_ids), n.size, _host_or_null(rir_lengths), rir_lengths.size,
                 int(fs), int(num_additives))


def aug_convolve(x, n, n_dev, rir_ids, rir_ids_dev, rir_lengths, fs, h, offsets_dev, meta, spectra, tables, num_additives, stats, workspace):
    """Steps 1 and 2 of the augmentation on x (B, T) fp32 / int16 (rows may be strided): the unshifted y into `workspace` (uint8, at
    least aug_workspace_bytes), p_before and p_sig into stats (B, AUG_STATS) fp64. n, rir_ids, rir_lengths: host int32; *_dev: the
    same on the device; h / offsets_dev / meta / spectra / tables: the bank as aug_rir_prepare took and left it, and aug_tables'
    (None for a batch without an RIR)."""
    n, rir_ids, rir_lengths = _host_i32(n), _host_i32(rir_ids), _host_i32(rir_lengths)
    _call("ktf_aug_convolve", x.device, L.ptr(x), int(x.dtype == torch.int16), _ld(x), _host_or_null(n), L.ptr(n_dev), _host_or_null(rir_ids),
          L.ptr(rir_ids_dev), n.size, _host_or_null(rir_lengths), rir_lengths.size, int(fs), L.ptr(h), L.ptr(offsets_dev), L.ptr(meta), L.ptr(spectra),
          L.ptr(tables), int(num_additives), L.ptr(stats), L.ptr(workspace), workspace.numel())
    return stats


def aug_mix(n, n_dev, rir_ids, rir_ids_dev, rir_lengths, fs, meta, add_offsets, add_offsets_dev, adds, adds_dev, noise, noise_offsets,
            noise_offsets_dev, shift_output, normalize_output, volume, out, stats, workspace):
    """Steps 3 to 5 on the y aug_convolve left in `workspace`: the additives adds (host (A, 4) int32 rows noise, snr_db's fp32 bits,
    start, duration; CSR add_offsets (B + 1) host int32) from the bank noise (fp32) / noise_offsets (host int64, M + 1), the scale and
    the window into out (B, T_out) fp32 / int16; p_after and the scale into stats."""
    n, rir_ids, rir_lengths = _host_i32(n), _host_i32(rir_ids), _host_i32(rir_lengths)
    add_offsets, adds = _host_i32(add_offsets), _host_i32(adds)
    noise_offsets = np.ascontiguousarray(noise_offsets, dtype=np.int64)
    _call("ktf_aug_mix", out.device, _host_or_null(n), L.ptr(n_dev), _host_or_null(rir_ids), L.ptr(rir_ids_dev), n.size,
          _host_or_null(rir_lengths), rir_lengths.size, int(fs), L.ptr(meta), _host_ptr(add_offsets), L.ptr(add_offsets_dev),
          _host_or_null(adds), L.ptr(adds_dev), L.ptr(noise), _host_ptr(noise_offsets), L.ptr(noise_offsets_dev), noise_offsets.size - 1,
          int(bool(shift_output)), int(bool(normalize_output)), float(volume), L.ptr(out), int(out.dtype == torch.int16), _ld(out),
          out.shape[1], L.ptr(stats), L.ptr(workspace), workspace.numel())
    return out, stats


# ----------------------------------------------------------------------------- sample-rate conversion (include/ktf_resample.h)
def rs_tile():
    """Consecutive outputs of one row per workgroup of the resampling kernel."""
    return int(L.load().ktf_rs_tile())


def rs_plan(fi, fo, cutoff, zeros):
    """The polyphase plan of fi -> fo (rules 1 and 2 of ktf_resample.h), host only -> (iu, ou, first (ou,) int32, taps (ou,) int32,
    w (ou, max taps) fp32, zero past a phase's taps)."""
    lib = L.load()
    sizes = (C.c_int32 * 3)()
    at = lambda k: C.c_void_p(C.addressof(sizes) + 4 * k)  # noqa: E731
    L.check(lib.ktf_rs_plan_sizes(int(fi), int(fo), float(cutoff), int(zeros), at(0), at(1), at(2)), "ktf_rs_plan_sizes")
    ou, iu, max_taps = (int(v) for v in sizes)
    first, taps, w = np.zeros(ou, np.int32), np.zeros(ou, np.int32), np.zeros((ou, max_taps), np.float32)
    L.check(lib.ktf_rs_plan(int(fi), int(fo), float(cutoff), int(zeros), _host_ptr(first), _host_ptr(taps), _host_ptr(w), max_taps), "ktf_rs_plan")
    return iu, ou, first, taps, w


def rs_num_out(n, fi, fo):
    """Output samples of n input samples (rule 3)."""
    return _size("ktf_rs_num_out", int(n), int(fi), int(fo))


def rs_resample(x, n, n_dev, iu, ou, first, taps, first_dev, taps_dev, w_dev, out):
    """Rows x (B, T) fp32 / int16 (rows may be strided) of n samples (host int32; n_dev the same on the device) through the plan
    (first / taps host int32, *_dev on the device, w_dev (ou, ldw) fp32) into out (B, T_out) fp32 / int16: zeros from a row's own
    length on."""
    n, first, taps = _host_i32(n), _host_i32(first), _host_i32(taps)
    _call("ktf_rs_resample", out.device, L.ptr(x), int(x.dtype == torch.int16), _ld(x), _host_or_null(n), L.ptr(n_dev), n.size, int(iu),
          int(ou), _host_ptr(first), _host_ptr(taps), L.ptr(first_dev), L.ptr(taps_dev), L.ptr(w_dev), _ld(w_dev), L.ptr(out),
          int(out.dtype == torch.int16), _ld(out), out.shape[1])
    return out


# ----------------------------------------------------------------------------- gradients of the TDNN and the pooling (include/ktf_grad.h)
def grad_tdnn_slot_rows():
    """Flat rows b * T_out + t per partial sum of the weight gradient."""
    return int(L.load().ktf_grad_tdnn_slot_rows())


def grad_tdnn_workspace(B, T, desc, device):
    """The workspace both TDNN gradient calls of a (B, T) batch of layer `desc` take."""
    return _workspace("ktf_grad_tdnn_workspace_bytes", int(B), int(T), C.byref(desc), device=device)


def grad_tdnn_data(g, lens, desc, w, dx, workspace):
    """g (B, T_out, ldg) fp32 dense rows, w the forward operand, dx (B, T, ldx) fp32 preallocated: every element of dx is written."""
    B, T, ldx = dx.shape
    _call("ktf_grad_tdnn_data", dx.device, L.ptr(g), g.shape[2], B, T, L.ptr(lens), C.byref(desc), L.ptr(w), L.ptr(dx), ldx,
          L.ptr(workspace), workspace.numel())
    return dx


def grad_tdnn_weights(x, lens, desc, g, dw, dbias, workspace):
    """x (B, T, ldx) fp32 dense rows as the forward read them, g (B, T_out, ldg); dw in the forward operand's layout and dbias (units,)
    or None, both preallocated: every element is written."""
    B, T, ldx = x.shape
    _call("ktf_grad_tdnn_weights", x.device, L.ptr(x), B, T, ldx, L.ptr(lens), C.byref(desc), L.ptr(g), g.shape[2], L.ptr(dw), L.ptr(dbias),
          L.ptr(workspace), workspace.numel())
    return dw, dbias


def grad_tdnn16_workspace(B, T, desc, gemm, device):
    """The workspace both 16-bit TDNN gradient calls (`gemm` = L.GEMM_BF16 / L.GEMM_BF16X3) of a (B, T) batch of layer `desc` take."""
    return _workspace("ktf_grad_tdnn16_workspace_bytes", int(B), int(T), C.byref(desc), int(gemm), device=device)


def grad_tdnn16_data(g, lens, desc, w, dx, workspace, gemm):
    """grad_tdnn_data on the bf16 MFMA: the same fp32 g, w (the fp32 forward operand) and dx; `gemm` = L.GEMM_BF16 / L.GEMM_BF16X3."""
    B, T, ldx = dx.shape
    _call("ktf_grad_tdnn16_data", dx.device, L.ptr(g), g.shape[2], B, T, L.ptr(lens), C.byref(desc), L.ptr(w), L.ptr(dx), ldx,
          L.ptr(workspace), workspace.numel(), int(gemm))
    return dx


def grad_tdnn16_weights(x, lens, desc, g, dw, dbias, workspace, gemm):
    """grad_tdnn_weights on the bf16 MFMA: the same fp32 x and g, dw and dbias; `gemm` = L.GEMM_BF16 / L.GEMM_BF16X3."""
    B, T, ldx = x.shape
    _call("ktf_grad_tdnn16_weights", x.device, L.ptr(x), B, T, ldx, L.ptr(lens), C.byref(desc), L.ptr(g), g.shape[2], L.ptr(dw), L.ptr(dbias),
          L.ptr(workspace), workspace.numel(), int(gemm))
    return dw, dbias


def grad_stats_pool(x, D, lens, input_period, include_std, eps, gout, dx):
    """x (B, T, ldx) fp32 dense rows, gout (B, D or 2 D) the gradient of ops.stats_pool's output, dx (B, T, ld_dx) preallocated."""
    B, T, ldx = x.shape
    for name, t in (("x", x), ("lens", lens), ("gout", gout), ("dx", dx)):
        _need_dense(name, t)
    _call("ktf_grad_stats_pool", x.device, L.ptr(x), B, T, int(D), ldx, L.ptr(lens), int(input_period), int(include_std), float(eps),
          L.ptr(gout), gout.shape[1], L.ptr(dx), dx.shape[2])
    return dx


# ----------------------------------------------------------------------------- ReLU + BatchNorm in training (include/ktf_norm.h)
def norm_slot_rows():
    """Flat rows b * T + t per partial sum of the batch statistics."""
    return int(L.load().ktf_norm_slot_rows())


def norm_workspace(B, T, D, device):
    """The workspace either call of a (B, T, D) batch takes."""
    return _workspace("ktf_norm_workspace_bytes", int(B), int(T), int(D), device=device)


def _rows_ptr(t, other):
    """Pointer of a (B, T, ld) operand; one without rows has no storage, and `other`'s non-null pointer stands for it (the library
    refuses null and reads no row)."""
    return L.ptr(t if t.numel() else other)


def norm_relu_bn_forward(z, D, lens, relu, training, gamma, moving_mean, moving_var, momentum, eps, y, saved, workspace):
    """z (B, T, ldz) fp32 dense rows of which D columns count, y (B, T, ldy) and saved (2, D) fp64 preallocated: every element of both
    is written; training updates moving_mean / moving_var (D,) in place."""
    B, T, ldz = z.shape
    _call("ktf_norm_relu_bn_forward", z.device, _rows_ptr(z, saved), ldz, B, T, int(D), L.ptr(lens), int(bool(relu)), int(bool(training)), L.ptr(gamma),
          L.ptr(moving_mean), L.ptr(moving_var), float(momentum), float(eps), _rows_ptr(y, saved), y.shape[2], L.ptr(saved), L.ptr(workspace),
          workspace.numel())
    return y, saved


def norm_relu_bn_backward(gy, z, D, lens, relu, training, gamma, saved, dz, dgamma, workspace):
    """gy (B, T, ldg) and z (B, T, ldz) fp32 dense rows, saved as the forward call left it; dz (B, T, ld_dz) and dgamma (D,) or None
    preallocated: every element is written."""
    B, T, ldz = z.shape
    _call("ktf_norm_relu_bn_backward", z.device, _rows_ptr(gy, saved), gy.shape[2], _rows_ptr(z, saved), ldz, B, T, int(D), L.ptr(lens), int(bool(relu)),
          int(bool(training)), L.ptr(gamma), L.ptr(saved), _rows_ptr(dz, saved), dz.shape[2], L.ptr(dgamma), L.ptr(workspace), workspace.numel())
    return dz, dgamma


# ----------------------------------------------------------------------------- the classification head's loss (include/ktf_loss.h)
LOSS_KINDS = {"softmax": 0, "am": 1, "aam": 2}


def loss_slot_rows():
    """Batch rows per partial sum of dinv_w."""
    return int(L.load().ktf_loss_slot_rows())


def loss_workspace(B, N, device):
    """The workspace either loss call of a (B, N) batch takes."""
    return _workspace("ktf_loss_workspace_bytes", int(B), int(N), device=device)


def _mat(t, other):
    """(pointer, leading dimension) of a 2-D fp32 operand whose rows are dense (a view with a row stride is fine); one without rows
    has no storage, and `other`'s non-null pointer stands for it (the library refuses null and reads no row)."""
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"expected a 2-D fp32 tensor with dense rows, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    return L.ptr(t if t.numel() else other), max(_ld(t), t.shape[1])


def _ptr_or(other):
    """t -> the pointer of an optional 1-D operand of the loss calls: None for None; a tensor without elements (B = 0) has no storage,
    and `other`'s non-null pointer stands for it as in _mat."""
    return lambda t: None if t is None else L.ptr(t if t.numel() else other)


def loss_row_inv_norm(x, eps, inv):
    """x (rows, D) fp32 with dense rows, inv (rows,) fp32 preallocated: inv[r] = 1 / max(|x[r]|, eps)."""
    if x.shape[0] == 0:
        return inv
    px, ldx = _mat(x, inv)
    _call("ktf_loss_row_inv_norm", x.device, px, ldx, x.shape[0], x.shape[1], float(eps), L.ptr(inv))
    return inv


def loss_row_inv_norm_backward(x, eps, inv, ginv, dx):
    """The gradient of loss_row_inv_norm: ginv (rows,) -> dx (rows, lddx >= D) preallocated, every element written."""
    if x.shape[0] == 0:
        return dx
    px, ldx = _mat(x, x)
    pd, lddx = _mat(dx, dx)
    _call("ktf_loss_row_inv_norm_backward", x.device, px, ldx, x.shape[0], x.shape[1], float(eps), L.ptr(inv), L.ptr(ginv), pd, lddx)
    return dx


def loss_margin_softmax_forward(z, labels, inv_x, inv_w, kind, margin, scale, loss, pred, lse, workspace):
    """z (B, N) fp32 with dense rows, labels (B,) int32, inv_x (B,) / inv_w (N,) fp32 or both None; loss (B,) fp32, pred (B,) int32 or
    None and lse (B,) fp64 preallocated. kind: "softmax", "am", "aam" or the KTF_LOSS_* number."""
    B, N = z.shape
    pz, ldz = _mat(z, workspace)
    at = _ptr_or(workspace)
    _call("ktf_loss_margin_softmax_forward", z.device, pz, ldz, B, N, at(labels), at(inv_x), at(inv_w), int(LOSS_KINDS.get(kind, kind)),
          float(margin), float(scale), at(loss), at(pred), at(lse), L.ptr(workspace), workspace.numel())
    return loss, pred, lse


def loss_margin_softmax_backward(z, labels, inv_x, inv_w, kind, margin, scale, lse, gloss, dz, dinv_x, dinv_w, workspace):
    """The gradient of sum_b gloss[b] * loss[b] (gloss None: ones): dz (B, lddz >= N), which may be z itself, and for a cosine head
    dinv_x (B,), dinv_w (N,), all preallocated and written whole."""
    B, N = z.shape
    pz, ldz = _mat(z, workspace)
    pd, lddz = _mat(dz, workspace)
    at = _ptr_or(workspace)
    _call("ktf_loss_margin_softmax_backward", z.device, pz, ldz, B, N, at(labels), at(inv_x), at(inv_w), int(LOSS_KINDS.get(kind, kind)),
          float(margin), float(scale), at(lse), at(gloss), pd, lddz, at(dinv_x), at(dinv_w), L.ptr(workspace), workspace.numel())
    return dz, dinv_x, dinv_w


# ------------------------------------------------- the head's loss with sub-centres, inter-top-k and smoothing (include/ktf_head.h)
def head_slot_rows():
    """Batch rows per partial sum of dinv_w."""
    return int(L.load().ktf_head_slot_rows())


def head_workspace(B, N, K, device):
    """The workspace either head call of a (B, N classes x K centres) batch takes."""
    return _workspace("ktf_head_workspace_bytes", int(B), int(N), int(K), device=device)


def _head_classes(z, K):
    K = int(K)
    if K < 1 or z.shape[1] % K:
        raise ValueError(f"sub_centers {K} does not divide the {z.shape[1]} columns of z")
    return z.shape[1] // K, K


def head_forward(z, K, labels, inv_x, inv_w, kind, margin, scale, topk, penalty, smoothing, loss, pred, lse, hard, sub_y, workspace):
    """z (B, N * K) fp32 with dense rows, class-major; labels (B,) int32, inv_x (B,) / inv_w (N * K,) fp32 or both None; loss (B,)
    fp32, pred (B,) int32 or None, lse (B,) fp64, hard (B, max(topk, 1)) int32 (None allowed when topk = 0) and sub_y (B,) int32 or
    None preallocated. kind as in loss_margin_softmax_forward."""
    B = z.shape[0]
    N, K = _head_classes(z, K)
    pz, ldz = _mat(z, workspace)
    at = _ptr_or(workspace)
    _call("ktf_head_forward", z.device, pz, ldz, B, N, K, at(labels), at(inv_x), at(inv_w), int(LOSS_KINDS.get(kind, kind)), float(margin),
          float(scale), int(topk), float(penalty), float(smoothing), at(loss), at(pred), at(lse), at(hard), at(sub_y), L.ptr(workspace),
          workspace.numel())
    return loss, pred, lse, hard, sub_y


def head_backward(z, K, labels, inv_x, inv_w, kind, margin, scale, topk, penalty, smoothing, lse, hard, gloss, dz, dinv_x, dinv_w,
                  workspace):
    """The gradient of sum_b gloss[b] * loss[b] (gloss None: ones) with the forward call's lse and hard: dz (B, lddz >= N * K), which
    may be z itself, and for a cosine head dinv_x (B,), dinv_w (N * K,), all preallocated and written whole."""
    B = z.shape[0]
    N, K = _head_classes(z, K)
    pz, ldz = _mat(z, workspace)
    pd, lddz = _mat(dz, workspace)
    at = _ptr_or(workspace)
    _call("ktf_head_backward", z.device, pz, ldz, B, N, K, at(labels), at(inv_x), at(inv_w), int(LOSS_KINDS.get(kind, kind)), float(margin),
          float(scale), int(topk), float(penalty), float(smoothing), at(lse), at(hard), at(gloss), pd, lddz, at(dinv_x), at(dinv_w),
          L.ptr(workspace), workspace.numel())
    return dz, dinv_x, dinv_w


# ----------------------------------------------------------------------------- attentive statistics pooling (include/ktf_attn.h)
def _attn_rows(name, t):
    """(pointer, row stride) of a (B, T, ld) fp32 operand of the attentive pooling."""
    if t.dim() != 3 or t.dtype != torch.float32:
        raise ValueError(f"{name}: a 3-D fp32 tensor is expected, got {t.dtype} {tuple(t.shape)}")
    _need_rows(name, t)
    return L.ptr(t), (t.stride(1) if t.shape[1] else t.shape[2])


def _attn_mat(name, t, dtype=torch.float32):
    if t.dim() != 2 or t.dtype != dtype:
        raise ValueError(f"{name}: a 2-D {dtype} tensor is expected, got {t.dtype} {tuple(t.shape)}")
    _need_rows(name, t)
    return L.ptr(t), _ld(t)


def _attn_sizes(x, e, D, H):
    if x.dim() != 3 or e.dim() != 3 or x.shape[:2] != e.shape[:2]:
        raise ValueError(f"x (B, T, ldx) and e (B, T, lde) with the same B and T are expected, got {tuple(x.shape)} and {tuple(e.shape)}")
    D = x.shape[2] if D is None else int(D)
    H = e.shape[2] if H is None else int(H)
    return x.shape[0], x.shape[1], D, H


def attn_pool(x, e, lens, include_std, eps, out, norm, stats=None, D=None, H=None):
    """x (B, T, ldx) and e (B, T, lde) fp32 rows with D channels / H heads (default: every column), lens (B,) int32 or None; out
    (B, ld_out) fp32, norm (B, H, 2) fp64 and stats (B, 2, D) fp64 (or None) preallocated."""
    B, T, D, H = _attn_sizes(x, e, D, H)
    if B == 0:
        return out, norm, stats
    px, ldx = _attn_rows("x", x)
    pe, lde = _attn_rows("e", e)
    po, ldo = _attn_mat("out", out)
    for name, t in (("lens", lens), ("norm", norm), ("stats", stats)):
        _need_dense(name, t)
    _call("ktf_attn_pool", x.device, px, B, T, D, ldx, pe, H, lde, L.ptr(lens), int(bool(include_std)), float(eps), po, ldo, L.ptr(norm),
          L.ptr(stats))
    return out, norm, stats


def attn_pool_backward_workspace(B, D, H, device):
    """The workspace attn_pool_backward takes for B utterances of D channels and H heads."""
    return _workspace("ktf_attn_pool_backward_workspace_bytes", int(B), int(D), int(H), device=device)


def attn_pool_backward(x, e, lens, include_std, eps, norm, stats, gout, dx, de, workspace, D=None, H=None):
    """The gradient of attn_pool's out: gout (B, ld_gout) -> dx (B, T, ld_dx) and de (B, T, ld_de) preallocated, every element
    written; norm and stats are the forward call's."""
    B, T, D, H = _attn_sizes(x, e, D, H)
    if B == 0 or T == 0:
        return dx, de
    px, ldx = _attn_rows("x", x)
    pe, lde = _attn_rows("e", e)
    pg, ldg = _attn_mat("gout", gout)
    pdx, ld_dx = _attn_rows("dx", dx)
    pde, ld_de = _attn_rows("de", de)
    if dx.shape[:2] != x.shape[:2] or de.shape[:2] != e.shape[:2]:
        raise ValueError(f"dx {tuple(dx.shape)} / de {tuple(de.shape)} do not have the rows of x {tuple(x.shape)}")
    for name, t in (("lens", lens), ("norm", norm), ("stats", stats), ("workspace", workspace)):
        _need_dense(name, t)
    _call("ktf_attn_pool_backward", x.device, px, B, T, D, ldx, pe, H, lde, L.ptr(lens), int(bool(include_std)), float(eps), L.ptr(norm),
          L.ptr(stats), pg, ldg, pdx, ld_dx, pde, ld_de, L.ptr(workspace), 0 if workspace is None else workspace.numel())
    return dx, de


# ----------------------------------------------------------------------------- training examples (include/ktf_egs.h)
EGS_DTYPES = {torch.float32: L.KTF_F32, torch.float16: L.KTF_F16}


def egs_philox(ctr, key):
    """Philox4x32-10 on the host (no GPU): ctr four and key two 32-bit words -> four 32-bit words."""
    c, k, out = (C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), (C.c_uint32 * 4)()
    L.check(L.load().ktf_egs_philox(c, k, out), "ktf_egs_philox")
    return tuple(int(v) for v in out)


def egs_index(spk_order, spk_off, spk_utts, spk_utt_len):
    """The KtfEgsIndex of four int32 device tensors (which the caller keeps alive)."""
    for t in (spk_order, spk_off, spk_utts, spk_utt_len):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError("the index arrays are contiguous int32 tensors")
    return L.EgsIndex(spk_order.data_ptr(), spk_off.data_ptr(), spk_utts.data_ptr(), spk_utt_len.data_ptr())


def _egs_bank(bank):
    """(pointer, dtype code, rows, ldb, D) of a bank (rows, D) with dense rows; a view with a row stride is fine."""
    if bank.dim() != 2 or bank.dtype not in EGS_DTYPES or (bank.shape[1] > 1 and bank.stride(1) != 1):
        raise ValueError(f"expected a 2-D fp32 / fp16 bank with dense rows, got {bank.dtype} {tuple(bank.shape)} strides {bank.stride()}")
    return L.ptr(bank), EGS_DTYPES[bank.dtype], bank.shape[0], max(_ld(bank), bank.shape[1]), bank.shape[1]


def _egs_out(out, D):
    """(pointer, ldo) of out (B, T, D) fp32 whose (T, ldo) chunks follow one another (a view with a row stride ldo >= D is fine)."""
    ok = out.dim() == 3 and out.dtype == torch.float32 and out.shape[2] == D
    if ok:
        B, T = out.shape[0], out.shape[1]
        ldo = out.stride(1) if T > 1 else (out.stride(0) if B > 1 else D)
        ok = ldo >= D and (D == 1 or out.stride(2) == 1) and (B == 1 or out.stride(0) == T * ldo)
    if not ok:
        raise ValueError(f"expected out (B, T, {D}) fp32 as one (B * T, ldo) matrix, got {out.dtype} {tuple(out.shape)} strides {out.stride()}")
    return L.ptr(out), ldo


def egs_draw(index, S, U, n_spk, seed, step, T, b0, b_stride, utt, offset, label):
    """Rules 1 - 7 for the global rows b0 + i * b_stride: utt, offset, label (B,) int32 preallocated."""
    if utt.numel():
        _call("ktf_egs_draw", utt.device, C.byref(index), int(S), int(U), int(n_spk), int(seed), int(step), int(T), int(b0), int(b_stride),
              utt.numel(), L.ptr(utt), L.ptr(offset), L.ptr(label))
    return utt, offset, label


def egs_gather(bank, row0, lens, utt, offset, T, out):
    """An explicit plan (utt, offset (B,) int32) -> out (B, T, D) fp32 preallocated, every element of its (T, ldo) chunks written."""
    if utt.numel():
        pb, dt, rows, ldb, D = _egs_bank(bank)
        po, ldo = _egs_out(out, D)
        _call("ktf_egs_gather", bank.device, pb, dt, rows, ldb, D, L.ptr(row0), L.ptr(lens), row0.numel(), L.ptr(utt), L.ptr(offset), int(T),
              utt.numel(), po, ldo)
    return out


def egs_sample(index, S, n_spk, seed, step, T, b0, b_stride, bank, row0, lens, out, utt, offset, label):
    """egs_draw and egs_gather of what it drew, in one launch."""
    if utt.numel():
        pb, dt, rows, ldb, D = _egs_bank(bank)
        po, ldo = _egs_out(out, D)
        _call("ktf_egs_sample", bank.device, C.byref(index), int(S), row0.numel(), int(n_spk), int(seed), int(step), int(T), int(b0),
              int(b_stride), utt.numel(), pb, dt, rows, ldb, D, L.ptr(row0), L.ptr(lens), po, ldo, L.ptr(utt), L.ptr(offset), L.ptr(label))
    return out, utt, offset, label


# ----------------------------------------------------------------------------- the optimiser step (include/ktf_optim.h)
OPTIM_KINDS = {"sgd": L.OPTIM_SGD, "adam": L.OPTIM_ADAM}


def optim_slot_elems():
    """Elements per slot of partial sums; every segment of the arenas begins at a multiple of it."""
    return int(L.load().ktf_optim_slot_elems())


def optim_workspace(total, n_seg, device):
    """The workspace a step over arenas of `total` elements in n_seg segments takes."""
    return _workspace("ktf_optim_workspace_bytes", int(total), int(n_seg), device=device)


def optim_segments(rows, device=None):
    """The segment table of rows (begin, end, group, max_change): the host array (a ctypes array of KtfOptimSeg; one spare entry
    keeps an empty table addressable) and, with a device, its copy there as a uint8 tensor."""
    host = (L.OptimSeg * max(len(rows), 1))()
    for i, (begin, end, group, max_change) in enumerate(rows):
        host[i] = L.OptimSeg(int(begin), int(end), int(group), float(max_change))
    if device is None:
        return host
    dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(device)
    return host, dev


def optim_step(p, g, m, v, segs_host, segs_dev, n_seg, groups, kind, momentum=0.0, nesterov=False, betas=(0.9, 0.999), eps=1e-8, step=1,
               decoupled=False, clip_norm=0.0, max_change_global=0.0, stats=None, workspace=None):
    """One step on the arenas p, g (and m, v or None): 1-D fp32 tensors of one length. segs_host / segs_dev: optim_segments' pair;
    groups: (lr, weight_decay) per group, read now; kind: "sgd", "adam" or the KTF_OPTIM_* number; stats: (5 + n_seg,) fp64 on the
    device or None. No host synchronisation."""
    total = p.numel()
    for t in (p, g, m, v):
        if t is not None and (t.dim() != 1 or t.dtype != torch.float32 or t.numel() != total or not t.is_contiguous()):
            raise ValueError(f"the arenas are contiguous 1-D fp32 tensors of one length, got {t.dtype} {tuple(t.shape)}")
    if stats is not None and (stats.dtype != torch.float64 or stats.numel() < 5 + n_seg or not stats.is_contiguous()):
        raise ValueError(f"stats holds 5 + n_seg = {5 + n_seg} contiguous fp64 values")
    if workspace is None:
        workspace = optim_workspace(total, n_seg, p.device)
    hg = (L.OptimGroup * max(len(groups), 1))()
    for i, (lr, wd) in enumerate(groups):
        hg[i] = L.OptimGroup(float(lr), float(wd))
    _call("ktf_optim_step", p.device, L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), total, C.cast(segs_host, C.c_void_p), L.ptr(segs_dev), int(n_seg),
          C.cast(hg, C.c_void_p), len(groups), int(OPTIM_KINDS.get(kind, kind)), float(momentum), int(bool(nesterov)), float(betas[0]),
          float(betas[1]), float(eps), int(step), int(bool(decoupled)), float(clip_norm), float(max_change_global), L.ptr(stats),
          L.ptr(workspace), workspace.numel())
    return p
