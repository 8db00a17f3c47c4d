"""Reference, yardstick, checker and cases for the front-end kernels (csrc/frontend.hip, csrc/frontend512.hip). Shared by
test_frontend_ref_cpu.py (pins the yardstick, shows that the bound rejects wrong arithmetic, scans the launcher's plan) and
test_gpu_frontend_instances.py (runs every kernel instance).

Reference: the fp64 oracle (oracle/ktf_oracle.py: pad_waveform, framing, windowing, filterbank, mfcc) on exactly the samples the
kernel reads. Yardstick: `ref32`, the same chain in fp32 with torch on the CPU (fp32 window, DC, pre-emphasis; torch.fft.rfft on
float32; fp32 mel product, log, DCT) -- one honest fp32 implementation, whose distance from the oracle says what fp32 costs for this
case and this output. Bound, per case and per output:

    rms(got - ref64) <= 4 * rms(ref32 - ref64)          max|got - ref64| <= 8 * max|ref32 - ref64|

4 is the project's margin for fp32 FFT pipelines (test_gpu_augment.py; worst ratio measured there 2.58). Two independent fp32
restatements (numpy's float32 FFT against torch's) differ from each other by 0.61 .. 0.96 in rms error and 0.36 .. 1.03 in max error:
the maximum of a few thousand errors moves about twice as much as their rms, hence 8.
"""

import dataclasses
import math
import zlib

import numpy as np
import torch

from kaldi_tflite_amd import _lib as L, ops
from oracle import ktf_oracle as O

RMS_MARGIN, MAX_MARGIN = 4.0, 8.0
TINY_DITHER = 2.0 ** -40
FE_WAVES = 4                    # csrc/frontend.hip: frames per workgroup of the generic kernel; its grid stops at 2048 workgroups
KINDS = {"wav": L.IN_WAV, "i16": L.IN_WAV_I16, "frames": L.IN_FRAMES, "windowed": L.IN_WINDOWED}
STAGES = {"windowed": L.OUT_WINDOWED, "fbank": L.OUT_FBANK, "mfcc": L.OUT_MFCC}


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    want: tuple = ()            # the instance the launcher must pick: ("fast512", dither, kind, mfix, std, nq) or ("generic", log2 nfft)
    sf: float = 16000.0
    M: int = 400                # frame size in samples (even)
    shift: int = 160
    num_mels: int = 30
    num_ceps: int = 30
    low: float = 20.0
    high: float = 7600.0
    lifter: float = 22
    window: str = "povey"
    use_energy: bool = True
    raw_energy: bool = True
    remove_dc: bool = True
    use_power: bool = True
    use_log: bool = True
    preemph: float = 0.97
    energy_floor: float = 0.0
    eps: float = 1e-7
    dither: float = 0.0
    kind: str = "wav"           # wav | i16 | frames | windowed
    pad: bool = False           # Framing(snip_edges=False): mirror padding fused into the gather
    out: str = "mfcc"           # windowed | fbank | mfcc
    B: int = 2
    n: int = 0                  # samples per row (wav, i16) or frames per row
    row_stride: int = 0         # > 0: rows are overlapping windows of one recording
    fast: bool = True           # False: the fast tables are withheld (the generic kernel at nfft 512)
    speech: bool = False        # the committed recording instead of noise: rms bound plus the 1e-3 maximum

    @property
    def nfft(self):
        return max(64, O.next_pow2(self.M))

    @property
    def is_wav(self):
        return self.kind in ("wav", "i16")

    def frames_per_row(self):
        if not self.is_wav:
            return self.n
        if self.pad:
            return (self.n + self.shift // 2) // self.shift
        return 1 + (self.n - self.M) // self.shift


def _ms(samples, sf):
    """A duration in ms that the oracle's frame_params turns back into `samples`."""
    v = samples * 1000.0 / sf
    while int(sf * v / 1000.0) < samples:
        v = np.nextafter(v, np.inf)
    assert int(sf * v / 1000.0) == samples
    return float(v)


def framing_kwargs(c):
    return dict(frame_length_ms=_ms(c.M, c.sf), frame_shift_ms=_ms(c.shift, c.sf), sample_frequency=c.sf)


def windowing_kwargs(c):
    return dict(window_type=c.window, remove_dc_offset=c.remove_dc, preemphasis_coefficient=c.preemph,
                raw_energy=c.raw_energy, energy_floor=c.energy_floor, epsilon=c.eps)


def fbank_kwargs(c):
    return dict(sample_frequency=c.sf, high_freq_cutoff=c.high, low_freq_cutoff=c.low, use_log_fbank=c.use_log, use_power=c.use_power,
                epsilon=c.eps)


def mfcc_kwargs(c):
    """Keyword arguments of the MFCC layer and of the oracle's mfcc() alike (dither apart: the reference never draws any)."""
    kw = dict(num_mfccs=c.num_ceps, num_mels=c.num_mels, cepstral_lifter=c.lifter, use_energy=c.use_energy, **windowing_kwargs(c))
    kw.update(sample_frequency=c.sf, high_freq_cutoff=c.high, low_freq_cutoff=c.low, use_log_fbank=c.use_log, use_power=c.use_power)
    return kw


# ----------------------------------------------------------------------------- inputs
def noise(shape, seed):
    """Integer-valued samples, sigma = 1000, clipped to int16, zeros replaced by 1: the same numbers are valid as fp32 and as int16,
    no mel energy is anywhere near eps, and |x| >= 1 everywhere (what the tiny-dither argument needs)."""
    rng = np.random.default_rng(seed)
    x = np.clip(np.round(1000.0 * rng.standard_normal(shape)), -32767, 32767)
    x[x == 0] = 1.0
    return x


def samples(c):
    """-> (buffer, rows): `buffer` is what goes to the device (1-D recording when the rows overlap, else (B, n) or (B, T, M)), `rows`
    the (B, n) / (B, T, M) float64 array of what the kernel reads from it."""
    seed = zlib.crc32(c.name.encode())
    if c.speech:
        import synth
        buf = synth.second_speech_wav().astype(np.float64)[None, :c.n].repeat(c.B, 0)
        return buf, buf
    if not c.is_wav:
        buf = noise((c.B, c.n, c.M), seed)
        return buf, buf
    if c.row_stride:
        buf = noise(((c.B - 1) * c.row_stride + c.n,), seed)
        return buf, np.stack([buf[b * c.row_stride: b * c.row_stride + c.n] for b in range(c.B)], 0)
    buf = noise((c.B, c.n), seed)
    return buf, buf


# ----------------------------------------------------------------------------- fp64 reference (the oracle)
def _split(c, feats, energy=None):
    """The outputs of a case by name. MFCC's C0 is the log-energy when use_energy is set: another quantity, with another error, than the
    cepstra beside it, so it is bounded on its own."""
    if c.out == "windowed":
        return {"windowed": feats, "energy": energy[..., 0]} if c.use_energy else {"windowed": feats}
    if c.out == "fbank":
        return {"fbank": feats}
    if not c.use_energy:
        return {"ceps": feats}
    out = {"c0": feats[..., 0]}
    if feats.shape[-1] > 1:
        out["ceps"] = feats[..., 1:]
    return out


def ref64(c, rows):
    x = np.asarray(rows, np.float64)
    if c.is_wav:
        if c.pad:
            x = O.pad_waveform(x, c.M, c.shift)
        x = O.framing(x, **framing_kwargs(c))
    if c.out == "mfcc":
        assert c.kind != "windowed"
        return _split(c, O.mfcc(x, **mfcc_kwargs(c), dtype=np.float64))
    energy = None
    if c.kind != "windowed":
        r = O.windowing(x, **windowing_kwargs(c), return_energy=c.use_energy, dtype=np.float64)
        x, energy = r if c.use_energy else (r, None)
    if c.out == "windowed":
        return _split(c, x, energy)
    return _split(c, O.filterbank(x, num_bins=c.num_mels, **fbank_kwargs(c), dtype=np.float64))


# ----------------------------------------------------------------------------- fp32 yardstick
CORRUPTIONS = ("mel_tail", "twiddle", "window_shift", "preemph_first", "pad_left", "dc_nfft", "bf16_spectrum", "post_energy",
               "no_lifter", "magnitude", "frame_start")


def sparse_bank(bank):
    """(nfft/2+1, num_mels) dense bank -> first bin, bin count and weights of each filter, as ops.FrontendTables stores them."""
    n2 = bank.shape[0] - 1
    starts, lens = [], []
    for f in range(bank.shape[1]):
        nz = np.nonzero(bank[:n2, f])[0]
        starts.append(int(nz[0]) if nz.size else 0)
        lens.append(int(nz[-1] - nz[0] + 1) if nz.size else 0)
    w = np.zeros((bank.shape[1], max(1, max(lens))), np.float32)
    for f in range(bank.shape[1]):
        w[f, :lens[f]] = bank[starts[f]:starts[f] + lens[f], f]
    return starts, lens, w


def mel_items(c):
    """The fast kernel's mel work items for a case's bank: (meta (64, 4), longest item) or None (ops.fast512_tables)."""
    _, bank = O.mel_bank(c.M, c.num_mels, c.sf, c.high, c.low)
    fast = ops.fast512_tables(*sparse_bank(bank)) if c.nfft == 512 and c.num_mels <= 32 else None
    return None if fast is None else (fast[1], fast[3])


def ref32(c, rows, fft="torch", reverse=False, corrupt=None):
    """The chain in fp32. `fft`: "torch" (the yardstick) or "numpy" (numpy's float32 FFT: a second, independent restatement);
    `reverse`: every sum taken in the opposite order; `corrupt`: one of CORRUPTIONS, each a way a kernel can be subtly wrong."""
    assert corrupt is None or corrupt in CORRUPTIONS
    f32 = torch.float32
    M, shift, nfft, n2 = c.M, c.shift, c.nfft, c.nfft // 2
    x = torch.as_tensor(np.asarray(rows, np.float32))

    def rsum(v):
        return (v.flip(-1) if reverse else v).sum(-1, keepdim=True)

    def matmul(a, b):
        return a.flip(-1) @ b.flip(0) if reverse else a @ b

    def log_energy(v):
        e = torch.log(torch.clamp(rsum(v * v), min=0.0) + f32_(c.eps))
        return torch.clamp(e, min=c.energy_floor)

    def f32_(v):
        return torch.tensor(v, dtype=f32)

    if c.is_wav:
        if c.pad:
            n = x.shape[-1]
            left = (M - shift) // 2
            right = ((n + shift // 2) // shift - 1) * shift + M - n - left
            lo = 1 if corrupt == "pad_left" else 0
            x = torch.cat([x[..., lo:lo + left].flip(-1), x, x[..., n - right:].flip(-1)], -1)
        T = 1 + (x.shape[-1] - M) // shift
        idx = (torch.arange(T) * shift)[:, None] + torch.arange(M)[None, :] + (1 if corrupt == "frame_start" else 0)
        x = x[..., idx.clamp(max=x.shape[-1] - 1)]
    energy = None
    if c.kind != "windowed":
        if c.remove_dc:
            x = x - rsum(x) / f32_(float(nfft if corrupt == "dc_nfft" else M))
        if c.use_energy and c.raw_energy:
            energy = log_energy(x)
        if c.preemph > 0:
            prev = torch.cat([x[..., :1], x[..., :-1]], -1)
            if corrupt == "preemph_first":
                prev[..., 0] = 0.0
            x = x - f32_(c.preemph) * prev
        w = torch.as_tensor(O.window_function(c.window, M).astype(np.float32))
        x = x * (w.roll(1) if corrupt == "window_shift" else w)
        if c.use_energy and (not c.raw_energy or corrupt == "post_energy"):
            energy = log_energy(x)
    if c.out == "windowed":
        return {k: v.numpy() for k, v in _split(c, x, energy).items()}

    _, bank = O.mel_bank(M, c.num_mels, c.sf, c.high, c.low)
    bank = bank.copy()
    live = np.nonzero(bank.sum(1))[0]
    if corrupt == "twiddle":
        # the last stage of a decimation-in-time FFT, X[k] = E[k] + W^k O[k], with ONE twiddle taken from its neighbour
        xp = torch.nn.functional.pad(x, (0, nfft - M))
        E, Od = torch.fft.fft(xp[..., 0::2]), torch.fft.fft(xp[..., 1::2])
        k = np.arange(n2 + 1)
        ang = -2.0 * np.pi * k / nfft
        k0 = int(live[len(live) // 2])
        ang[k0] = ang[k0 + 1]
        W = torch.as_tensor(np.exp(1j * ang).astype(np.complex64))
        spec = E[..., k % n2] + W * Od[..., k % n2]
    elif fft == "torch":
        spec = torch.fft.rfft(x, n=nfft)
    else:
        spec = np.fft.rfft(x.numpy(), n=nfft)
        assert spec.dtype == np.complex64, "numpy's FFT did not stay in single precision"
        spec = torch.as_tensor(spec)
    assert spec.dtype == torch.complex64
    re, im = spec.real, spec.imag
    if corrupt == "bf16_spectrum":
        re, im = re.bfloat16().float(), im.bfloat16().float()
    p = re * re + im * im
    if not c.use_power or corrupt == "magnitude":
        p = torch.sqrt(p)
    if corrupt == "mel_tail":
        # what an understated NQ does: the longest work item read as two 16-byte pieces, its bins past them lost
        meta, _ = mel_items(c)
        i = int(np.argmax(meta[:, 1]))
        s0, ln, f = (int(v) for v in meta[i, :3])
        drop = -(-ln // 4) * 4 - 8
        assert drop > 0
        bank[s0 + ln - drop: s0 + ln, f] = 0.0
    feats = matmul(p, torch.as_tensor(bank))
    if c.use_log:
        feats = torch.log(torch.clamp(feats, min=0.0) + f32_(c.eps))
    if c.out == "fbank":
        return {"fbank": feats.numpy()}
    ceps = matmul(feats, torch.as_tensor(O.dct_matrix(c.num_mels, c.num_ceps).astype(np.float32)))
    if c.lifter > 1 and corrupt != "no_lifter":
        ceps = ceps * torch.as_tensor(O.lifter_coeffs(c.num_ceps, c.lifter).astype(np.float32))
    if c.use_energy:
        ceps = torch.cat([energy, ceps[..., 1:]], -1)
    return {k: v.numpy() for k, v in _split(c, ceps).items()}


# ----------------------------------------------------------------------------- the bound
def errors(got, want):
    d = np.asarray(got, np.float64) - np.asarray(want, np.float64)
    return float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())


def ratios(got, r64, r32):
    """{output: (rms ratio, max ratio, rms error, max error)} of `got` against the yardstick's own errors."""
    assert set(got) == set(r64) == set(r32), (sorted(got), sorted(r64), sorted(r32))
    out = {}
    for k in r64:
        assert got[k].shape == r64[k].shape == r32[k].shape, (k, got[k].shape, r64[k].shape, r32[k].shape)
        assert np.isfinite(got[k]).all(), k
        (gr, gm), (yr, ym) = errors(got[k], r64[k]), errors(r32[k], r64[k])
        div = lambda a, b: a / b if b > 0 else (0.0 if a == 0 else math.inf)  # noqa: E731
        out[k] = (div(gr, yr), div(gm, ym), gr, gm)
    return out


def violations(got, r64, r32, rms_only=False, max_abs=None):
    """The outputs that miss the bound, as text ([] = the case passes)."""
    bad = []
    for k, (rr, mr, gr, gm) in ratios(got, r64, r32).items():
        if rr > RMS_MARGIN:
            bad.append(f"{k}: rms error {gr:.3e} is {rr:.2f} x the fp32 yardstick's (> {RMS_MARGIN})")
        if not rms_only and mr > MAX_MARGIN:
            bad.append(f"{k}: max error {gm:.3e} is {mr:.2f} x the fp32 yardstick's (> {MAX_MARGIN})")
        if max_abs is not None and gm > max_abs:
            bad.append(f"{k}: max error {gm:.3e} > {max_abs}")
    return bad


# ----------------------------------------------------------------------------- what the launcher is asked
def frontend_cfg(c):
    """KtfFrontendCfg of a case the way XvectorExtractor._features builds it: the MFCC layer's own, then the framing's fields."""
    import kaldi_tflite_amd as ktf
    mf = ktf.layers.MFCC(**mfcc_kwargs(c), dither=c.dither)
    mf.build((None, None, c.M))
    cfg = L.FrontendCfg.from_buffer_copy(mf._cfg)
    cfg.frame_size, cfg.frame_shift = c.M, (c.shift if c.is_wav else c.M)
    cfg.pad_mode = 1 if (c.pad and c.is_wav) else 0
    cfg.row_stride = c.row_stride
    assert cfg.nfft == c.nfft
    return mf, cfg


def host_tables(c, reserved=None):
    """A KtfFrontendTables for ktf_frontend_plan without a GPU: the plan only asks which tables are there, so every pointer the
    configuration has is a dummy; mel_stride and `reserved` are what ops.FrontendTables computes."""
    _, bank = O.mel_bank(c.M, c.num_mels, c.sf, c.high, c.low)
    _, lens, _ = sparse_bank(bank)
    items = mel_items(c) if c.fast else None
    t = L.FrontendTables(window=1, twiddle=1, rtwiddle=1, mel_start=1, mel_len=1, mel_w=1, dct=1, lifter=1 if c.lifter > 1 else None,
                         mel_stride=max(1, max(lens)))
    if items is not None:
        t.fast_tw = t.fast_mel_meta = t.fast_mel_w = 1
        t.reserved = items[1] if reserved is None else reserved
    return t


def plan_key(p):
    if p.kernel == L.FE_FAST512:
        return ("fast512", bool(p.dither), p.kind, p.mfix, bool(p.std), p.nq)
    if p.kernel == L.FE_GENERIC:
        return ("generic", p.log2_nfft)
    return ({L.FE_NONE: "none", L.FE_FRAMING: "framing"}[p.kernel],)


def plan(c, tables, cfg=None):
    cfg = cfg or frontend_cfg(c)[1]
    return ops.frontend_plan(c.B, c.n, KINDS[c.kind], cfg, tables, STAGES[c.out])


# Every kernel instance the two launchers can start: the fifteen of ktf_frontend512_launch and the six of ktf_frontend_f32.
def _fast(dither, kind, mfix, std=False, nq=5):
    return ("fast512", dither, kind, mfix, std, nq)


INSTANCES = frozenset(
    [_fast(False, k, 400, True, nq) for k in (1, 2) for nq in (3, 4, 5)]
    + [_fast(d, k, m) for d, m in ((True, 0), (False, 400), (False, 0)) for k in (0, 1, 2)]
    + [("generic", lg) for lg in range(6, 12)])

# mel banks of the fast kernel's NQ instances: (num_mels, low, high) -> bins of the longest work item
BANK_NQ3 = dict(num_mels=32, low=20.0, high=2000.0)     # 6-bin items  -> 3 pieces
BANK_NQ4 = dict(num_mels=30, low=20.0, high=7600.0)     # 10-bin items -> 4
BANK_NQ4_SPLIT = dict(num_mels=23, low=20.0, high=0.0)  # 13-bin items -> 4 (46 items: every filter split)
BANK_NQ5 = dict(num_mels=18, low=20.0, high=0.0)        # 16-bin items -> 5
BANK_ITEMS = ((BANK_NQ3, 6, 3), (BANK_NQ4, 10, 4), (BANK_NQ4_SPLIT, 13, 4), (BANK_NQ5, 16, 5))
ODD = 400 + 4 * 160 + 1         # B = 3 rows of an odd length: int16 rows start at 4-byte and at 2-byte alignment in turn


def _c(name, want, **kw):
    kw.update(kw.pop("bank", {}))
    if "num_mels" in kw and "num_ceps" not in kw:
        kw["num_ceps"] = kw["num_mels"]
    return Case(name=name, want=want, **kw)


def fast_cases():
    """The fast kernel at the smallest shapes that still reach every path (one line per reason in the issue's list)."""
    s = lambda k, nq: _fast(False, k, 400, True, nq)  # noqa: E731
    return [
        # shipped hot path (STD): two passes of the frame loop, the second with one live wave (B = 1024: gx = 2, three groups of 8)
        _c("std_f32_nq4_two_passes", s(1, 4), bank=BANK_NQ4, B=1024, n=400 + 16 * 160),
        _c("std_i16_nq4_split_filters", s(2, 4), bank=BANK_NQ4_SPLIT, kind="i16", B=3, n=ODD),
        _c("std_f32_nq4_split_filters", s(1, 4), bank=BANK_NQ4_SPLIT, B=2, n=400 + 9 * 160),
        _c("std_f32_nq3_T1", s(1, 3), bank=BANK_NQ3, B=2, n=400),
        _c("std_i16_nq3", s(2, 3), bank=BANK_NQ3, kind="i16", B=3, n=ODD),
        _c("std_f32_nq5_overlapping_rows", s(1, 5), bank=BANK_NQ5, B=4, n=400 + 4 * 160, row_stride=333),
        _c("std_i16_nq5", s(2, 5), bank=BANK_NQ5, kind="i16", B=3, n=ODD),
        _c("std_f32_speech", s(1, 4), bank=BANK_NQ4, B=1, n=48000, speech=True),
        # frame 400 outside the shipped switches
        _c("f400_frames_fbank_linear", _fast(False, 1, 400), kind="frames", out="fbank", use_log=False, B=2, n=9),
        _c("f400_windowed_fbank_magnitude", _fast(False, 1, 400), kind="windowed", out="fbank", use_power=False, B=1, n=9),
        _c("f400_f32_no_energy_no_lifter_hamming", _fast(False, 1, 400), use_energy=False, lifter=0, window="hamming", B=2, n=ODD),
        _c("f400_i16_post_energy_hanning", _fast(False, 2, 400), kind="i16", raw_energy=False, window="hanning", B=3, n=ODD),
        _c("f400_i16_fbank_no_dc_no_preemph_rect", _fast(False, 2, 400), kind="i16", out="fbank", remove_dc=False, preemph=0.0,
           window="rectangular", B=3, n=ODD),
        _c("f400_pad_f32_both_edges_mirror", _fast(False, 0, 400), pad=True, B=2, n=200),
        _c("f400_pad_f32_smallest_n", _fast(False, 0, 400), pad=True, B=2, n=140),
        _c("f400_pad_i16", _fast(False, 0, 400), kind="i16", pad=True, B=3, n=ODD),
        # other frame sizes (MFIX = 0)
        _c("f512_f32_32mels_energy_floor", _fast(False, 1, 0), M=512, num_mels=32, high=0.0, energy_floor=50.0, B=2, n=512 + 9 * 160),
        _c("f258_frames_fbank_blackman", _fast(False, 1, 0), M=258, kind="frames", out="fbank", window="blackman", B=2, n=9),
        _c("f320_i16_one_cep_sine", _fast(False, 2, 0), M=320, kind="i16", num_ceps=1, window="sine", B=3, n=320 + 4 * 160 + 1),
        _c("f320_pad_f32", _fast(False, 0, 0), M=320, pad=True, B=2, n=1000),
        _c("f258_pad_i16_fbank", _fast(False, 0, 0), M=258, shift=100, kind="i16", pad=True, out="fbank", B=3, n=1001),
        # dither instances, with a dither too small to change any sample
        _c("dither_f32", _fast(True, 1, 0), dither=TINY_DITHER, B=2, n=ODD),
        _c("dither_i16", _fast(True, 2, 0), kind="i16", dither=TINY_DITHER, B=3, n=ODD),
        _c("dither_pad_i16", _fast(True, 0, 0), kind="i16", pad=True, dither=TINY_DITHER, B=3, n=ODD),
        _c("dither_pad_f32_fbank", _fast(True, 0, 0), pad=True, out="fbank", dither=TINY_DITHER, B=2, n=200),
        # one mel bin too many for the fast kernel
        _c("33mels_generic", ("generic", 9), num_mels=33, high=0.0, B=2, n=ODD),
    ]


def generic_cases():
    """The generic kernel: every nfft at frame = nfft and frame = nfft / 2 + 2, the realistic sizes, every input kind."""
    mels = {64: 5, 128: 8, 256: 23, 512: 30, 1024: 40, 2048: 40}
    out = []
    for lg in range(6, 12):
        nf = 1 << lg
        g = ("generic", lg)
        k = dict(num_mels=mels[nf], num_ceps=min(mels[nf], 13), high=0.0, fast=False)
        out.append(_c(f"nfft{nf}_full_frame_fbank_linear", g, M=nf, shift=nf // 2 - 3, out="fbank", use_log=False, B=2,
                      n=nf + 6 * (nf // 2 - 3) + 1, **k))
        out.append(_c(f"nfft{nf}_short_frame_mfcc_i16_pad", g, M=nf // 2 + 2, shift=nf // 4, kind="i16", pad=True, B=3,
                      n=5 * (nf // 4) + 1, **k))
    k = dict(fast=False, high=0.0)
    out += [
        _c("8k_frame200_mfcc", ("generic", 8), sf=8000.0, M=200, shift=80, num_mels=23, B=2, n=200 + 9 * 80, **k),
        _c("32k_frame800_mfcc_i16", ("generic", 10), sf=32000.0, M=800, shift=320, num_mels=40, num_ceps=20, kind="i16", B=3,
           n=800 + 4 * 320 + 1, **k),
        _c("44k_frame1102_fbank", ("generic", 11), sf=44100.0, M=1102, shift=441, num_mels=40, out="fbank", B=2, n=1102 + 5 * 441, **k),
        _c("nfft128_frames_mfcc_post_energy", ("generic", 7), M=100, kind="frames", num_mels=8, raw_energy=False, B=2, n=7, **k),
        _c("nfft256_windowed_fbank_magnitude", ("generic", 8), M=256, kind="windowed", out="fbank", num_mels=23, use_power=False, B=1,
           n=7, **k),
        _c("nfft1024_dither_f32", ("generic", 10), M=600, shift=200, num_mels=40, num_ceps=13, dither=TINY_DITHER, B=2, n=600 + 5 * 200, **k),
        _c("nfft64_dither_i16_pad", ("generic", 6), M=48, shift=16, num_mels=5, kind="i16", pad=True, dither=TINY_DITHER, B=3, n=161, **k),
        _c("nfft512_frames_windowed_energy", ("generic", 9), M=400, kind="frames", out="windowed", B=2, n=7, **k),
        _c("nfft256_frames_windowed_no_energy", ("generic", 8), M=200, kind="frames", out="windowed", use_energy=False, B=1, n=5, **k),
        # rows = 2048 * FE_WAVES + 5: the grid-stride loop runs a second pass in which workgroup 1 has one live wave and the rest none
        _c("nfft64_grid_stride", ("generic", 6), M=34, shift=16, num_mels=5, num_ceps=5, B=1, n=34 + 16 * (2048 * FE_WAVES + 4), **k),
    ]
    return out
