"""Waveform augmentation on the GPU: what the x-vector recipes' steps/data/reverberate_data_dir.py and
steps/data/augment_data_dir.py script per utterance as a wav-reverberate command line -- convolution with a room impulse response,
noise / music / babble added at an SNR measured against the early-reverberation energy, power normalisation -- on a ragged batch.
The semantics are the project's own, stated in include/ktf_augment.h; tests/_augment_ref.py restates them in fp64.

    rirs = ktf.augment.RirBank([h0, h1, ...])                    # spectra prepared once
    noises = ktf.augment.NoiseBank([n0, n1, ...])
    plan = ktf.augment.plan_additives("babble", [len(w) / 16000 for w in wavs], noises.lengths_s, seed=0)
    out, lengths = ktf.augment.augment(wavs, rirs=rirs, rir_ids=[0, 1, -1, ...], noises=noises, additives=plan)
    xvectors = extractor(out)                                      # (equal lengths; else [out[b, :l] for b, l in enumerate(lengths)])

Sample-rate conversion (the rules are stated in include/ktf_resample.h, tests/_resample_ref.py restates them in
fp64): a windowed-sinc polyphase resampler after Kaldi's LinearResample in its whole-signal mode, and speed perturbation on top.

    to8k = ktf.augment.Resampler(16000, 8000)                      # the plan, computed once
    out, lengths = to8k(wavs)                                      # wavs as augment() takes them, fp32 or int16
    out, lengths = ktf.augment.resample(wavs, 44100, 16000)        # one-shot; equal rates return the input
    fast, lengths = ktf.augment.speed_perturb(wavs, 1.1)           # sox `speed 1.1`: 11 -> 10, read at the old rate

augment() still refuses a bank at another rate than the signals': convert the arrays first and build the bank at the new rate.

    rirs8k, n = to8k(rirs16k)                                      # 16 kHz RIRs and noises for an 8 kHz recipe
    rirs = ktf.augment.RirBank([rirs8k[r, :l].cpu().numpy() for r, l in enumerate(n)], sample_rate=8000)
    noise8k, n = to8k(noises16k)
    noises = ktf.augment.NoiseBank([noise8k[r, :l].cpu().numpy() for r, l in enumerate(n)], sample_rate=8000)
    out, lengths = ktf.augment.augment(wavs8k, rirs=rirs, rir_ids=ids, noises=noises, additives=plan, sample_rate=8000)
"""

import fractions

import numpy as np
import torch

from . import _lib as L, ops
from ._host import host, is_int, is_real, max_under

PRE_S, POST_S = 0.001, 0.05        # the early-reverberation window about the RIR's peak, in seconds

# what plan_additives draws per kind: (SNRs in dB, foreground, (min, max) pieces; None = as many as fit)
KINDS = {
    "noise": ((15, 10, 5, 0), True, None),
    "music": ((15, 10, 8, 5), False, (1, 1)),
    "babble": ((20, 17, 15, 13), False, (3, 7)),
}
FOREGROUND_INTERVAL_S = 1.0


def _sample_rate(sample_rate):
    if not is_int(sample_rate) or sample_rate <= 0:
        raise ValueError(f"sample_rate must be a positive int, got {sample_rate!r}")
    return int(sample_rate)


def _one_dim(items, what):
    """A list of 1-D recordings -> [fp32 NumPy arrays]; a recording with channels is refused."""
    if isinstance(items, (np.ndarray, torch.Tensor)) and items.ndim == 1:
        items = [items]
    out = []
    for i, a in enumerate(items):
        a = host(a)
        if a.ndim != 1:
            raise ValueError(f"{what} {i} has shape {tuple(a.shape)}: multi-channel {what}s are not supported (give one 1-D array each)")
        if a.size == 0:
            raise ValueError(f"{what} {i} is empty")
        a = a.astype(np.float32)
        if not np.isfinite(a).all():
            raise ValueError(f"{what} {i} holds a non-finite sample")
        out.append(a)
    return out


def _ragged(arrays, device):
    """[1-D fp32 arrays] -> (flat device tensor, host offsets int64 (len + 1))."""
    off = np.zeros(len(arrays) + 1, np.int64)
    off[1:] = np.cumsum([a.size for a in arrays])
    flat = np.concatenate(arrays) if arrays else np.zeros(0, np.float32)
    return torch.as_tensor(flat, device=device), off


class RirBank:
    """Room impulse responses, one 1-D array each (any lengths). The peak index, the early window and the partition spectra of every
    RIR are computed on the device once, here. `.lengths` (taps) and `.peak` (the lowest index of each RIR's signed maximum) are
    host int32 arrays."""

    def __init__(self, rirs, sample_rate=16000, device=None):
        self.sample_rate = _sample_rate(sample_rate)
        arrays = _one_dim(rirs, "RIR")
        self.lengths = np.array([a.size for a in arrays], np.int32)
        if int(self.lengths.sum()) > 1 << 30:
            raise ValueError("more than 2^30 taps in one RirBank")
        L.require_gpu()
        self.device = torch.device(device) if device is not None else ops.default_device()
        self.taps, off = _ragged(arrays, self.device)
        self.offsets = off.astype(np.int32)
        self._peak = None
        with L.launch_scope(self.device):
            self.tables = ops.aug_tables(self.device)
            self.offsets_dev = torch.as_tensor(self.offsets, device=self.device)
            self.meta, self.spectra = ops.aug_rir_prepare(self.taps, self.offsets, self.offsets_dev, self.sample_rate, self.tables)

    def __len__(self):
        return int(self.lengths.size)

    @property
    def peak(self):
        if self._peak is None:
            self._peak = host(self.meta[:, 0], np.int32) if len(self) else np.zeros(0, np.int32)
        return self._peak


class NoiseBank:
    """Noise / music / speech recordings to add, one 1-D array each: ragged device storage (flat samples and offsets)."""

    def __init__(self, noises, sample_rate=16000, device=None):
        self.sample_rate = _sample_rate(sample_rate)
        arrays = _one_dim(noises, "noise")
        self.lengths = np.array([a.size for a in arrays], np.int64)
        L.require_gpu()
        self.device = torch.device(device) if device is not None else ops.default_device()
        self.flat, self.offsets = _ragged(arrays, self.device)
        self.offsets_dev = torch.as_tensor(self.offsets, device=self.device)

    def __len__(self):
        return int(self.lengths.size)

    @property
    def lengths_s(self):
        return self.lengths / float(self.sample_rate)


def plan_additives(kind, lengths_s, noise_lengths_s, seed):
    """What steps/data/augment_data_dir.py draws for the recipes' three kinds, per utterance of lengths_s seconds, from a pool of
    noises of noise_lengths_s seconds: [[(noise_id, snr_db, start_s, duration_s)]], augment()'s `additives`. Host only.
      "noise":  foreground noises one after another, a new one every 1 s of the utterance, each its own length (cut at the
                utterance's end), SNR from {15, 10, 5, 0};
      "music":  one background piece over the whole utterance (repeated to its length), SNR from {15, 10, 8, 5};
      "babble": 3 to 7 background speakers over the whole utterance, SNR from {20, 17, 15, 13}.
    Every draw comes from np.random.default_rng(seed), utterance by utterance: (background) the count, then per piece the noise id
    and the SNR."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
    lengths_s = np.atleast_1d(np.asarray(lengths_s, np.float64))
    pool = np.atleast_1d(np.asarray(noise_lengths_s, np.float64))
    if pool.size == 0 or not (pool > 0).all():
        raise ValueError("plan_additives needs a pool of noises of positive length")
    if not (lengths_s >= 0).all():
        raise ValueError("negative utterance length")
    snrs, foreground, count = KINDS[kind]
    rng = np.random.default_rng(seed)
    plan = []
    for dur in lengths_s:
        row = []
        if foreground:
            t = 0.0
            while t < dur:
                nid = int(rng.integers(pool.size))
                snr = float(snrs[int(rng.integers(len(snrs)))])
                row.append((nid, snr, t, float(min(pool[nid], dur - t))))
                t += FOREGROUND_INTERVAL_S
        elif dur > 0:
            for _ in range(int(rng.integers(count[0], count[1] + 1))):
                nid = int(rng.integers(pool.size))
                snr = float(snrs[int(rng.integers(len(snrs)))])
                row.append((nid, snr, 0.0, float(dur)))
        plan.append(row)
    return plan


def _signals(wavs, lengths):
    """wavs as XvectorExtractor takes them -> ((B, T) device tensor fp32 / int16 with unit sample stride, host lengths int32)."""
    from .layers import Framing
    if isinstance(wavs, (list, tuple)):
        if lengths is not None:
            raise ValueError("lengths= goes with a (B, T) tensor; a list of recordings carries its own")
        items = []
        for r, w in enumerate(wavs):
            if not isinstance(w, torch.Tensor):
                w = torch.as_tensor(np.asarray(w))
            if w.dim() != 1:
                raise ValueError(f"recording {r} has shape {tuple(w.shape)}: multi-channel signals are not supported")
            items.append(w)
        i16 = bool(items) and all(w.dtype == torch.int16 for w in items)
        dev = next((w.device for w in items if w.is_cuda), ops.default_device())
        n = np.array([w.numel() for w in items], np.int32)
        x = torch.zeros((len(items), int(n.max()) if len(items) else 0), dtype=torch.int16 if i16 else torch.float32, device=dev)
        for r, w in enumerate(items):
            x[r, :w.numel()] = w.to(dev)
        return x, n
    if isinstance(wavs, (np.ndarray, torch.Tensor)) and wavs.ndim > 2:
        raise ValueError(f"wavs has shape {tuple(wavs.shape)}: multi-channel signals are not supported")
    x, _ = Framing.device_samples(wavs)
    if x.dim() == 1:
        x = x.unsqueeze(0)
    B, T = x.shape
    if lengths is None:
        n = np.full(B, T, np.int32)
    else:
        n = host(lengths).astype(np.int64).reshape(-1)
        if n.size != B or (n < 0).any() or (n > T).any():
            raise ValueError(f"lengths must be {B} values in 0 .. {T}")
        n = n.astype(np.int32)
    return x, n


def _additive_rows(additives, B, fs):
    """additives -> (host CSR offsets int32 (B + 1), host rows (A, 4) int32: noise id, the fp32 bits of snr_db, start and duration
    in samples)."""
    if additives is None:
        return np.zeros(B + 1, np.int32), np.zeros((0, 4), np.int32)
    if isinstance(additives, tuple) and len(additives) == 2 and isinstance(additives[0], torch.Tensor):
        off = host(additives[0]).astype(np.int64).reshape(-1)          # CSR: offsets (B + 1), rows (A, 4) as the list form's tuples
        table = host(additives[1]).astype(np.float64).reshape(-1, 4)
        if off.size != B + 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != table.shape[0]:
            raise ValueError("additives CSR: offsets must be B + 1 ascending values from 0 to the number of rows")
    else:
        if len(additives) != B:
            raise ValueError(f"additives must hold one list per row ({B}), got {len(additives)}")
        off = np.zeros(B + 1, np.int64)
        off[1:] = np.cumsum([len(row) for row in additives])
        flat = [a for row in additives for a in row]
        try:
            table = np.array(flat, np.float64).reshape(-1, 4)
        except (TypeError, ValueError):
            raise ValueError("an additive is (noise_id, snr_db, start_s, duration_s)") from None
    if (table[:, 0] != np.floor(table[:, 0])).any():
        raise ValueError("additives: noise ids must be integers")
    if not np.isfinite(table[:, 2:]).all() or (np.abs(table[:, 2:]) * fs >= 2 ** 31).any():
        raise ValueError("additives: start_s / duration_s must be finite and below 2^31 samples")
    rows = np.zeros((table.shape[0], 4), np.int32)
    rows[:, 0] = table[:, 0].astype(np.int32)
    rows[:, 1] = table[:, 1].astype(np.float32).view(np.int32)
    rows[:, 2] = np.round(table[:, 2] * fs).astype(np.int32)
    rows[:, 3] = np.where(table[:, 3] > 0, np.maximum(1, np.round(table[:, 3] * fs)), 0).astype(np.int32)   # 0 stays "its own length"
    return off.astype(np.int32), rows


def _row_chunks(n, ids, rir_lengths, fs, add_off, limit):
    """[(lo, hi)] consecutive rows whose workspace stays under `limit` bytes (a row that alone exceeds it is a chunk of its own)."""
    B = n.size
    out, lo = [], 0
    while lo < B:
        need = lambda c: ops.aug_workspace_bytes(n[lo:lo + c], ids[lo:lo + c], rir_lengths, fs, int(add_off[lo + c] - add_off[lo]))  # noqa: E731
        hi = lo + max_under(need, limit, min(B - lo, 65535))
        out.append((lo, hi))
        lo = hi
    return out


def augment(wavs, lengths=None, rirs=None, rir_ids=None, noises=None, additives=None, shift_output=True, normalize_output=True,
            volume=0.0, out_dtype=torch.float32, workspace_limit=1 << 30, sample_rate=16000, duration=None, return_stats=False):
    """Reverberate and corrupt a ragged batch. wavs: a (B, T) tensor / array (with lengths= (B,) or all T), one 1-D recording, or a
    list of 1-D recordings; fp32 in int16 scale or int16 PCM. rirs: a RirBank with rir_ids (B,) ints, -1 for none (rir_ids None: no
    row is reverberated). noises: a NoiseBank with additives, per row a list of (noise_id, snr_db, start_s, duration_s) with
    duration_s = 0 for the noise's own length, or the CSR tuple (offsets (B + 1,), rows (A, 4)) of tensors.
    -> (out (B, T_out) out_dtype on the device, zeros past each row's length; out_lengths, B host ints): with shift_output row b is
    y[k : k + n], else all n + L - 1 samples. return_stats=True adds a third value, (B, 4) fp64 on the device: p_before, p_sig,
    p_after and the scale applied. Rows are processed in chunks whose workspace stays under workspace_limit bytes; a row's bits
    depend on neither the chunking nor the other rows."""
    if duration not in (None, 0):
        raise ValueError("duration: repeating or cutting the main signal to a duration is not supported")
    fs = _sample_rate(sample_rate)
    for bank, what in ((rirs, "rirs"), (noises, "noises")):
        if bank is not None and bank.sample_rate != fs:
            raise ValueError(f"{what} are at {bank.sample_rate} Hz, the signals at {fs} Hz: resampling is not supported")
    if out_dtype not in (torch.float32, torch.int16):
        raise ValueError(f"out_dtype must be torch.float32 or torch.int16, got {out_dtype}")
    if not is_real(volume) or not np.isfinite(volume):
        raise ValueError(f"volume must be a finite number, got {volume!r}")
    L.require_gpu()
    x, n = _signals(wavs, lengths)
    B = n.size
    dev = x.device
    for bank, what in ((rirs, "rirs"), (noises, "noises")):
        if bank is not None and bank.device != dev:
            raise ValueError(f"{what} live on {bank.device}, the signals on {dev}")
    R = len(rirs) if rirs is not None else 0
    if rir_ids is None:
        ids = np.full(B, -1, np.int32)
    else:
        ids = host(rir_ids).astype(np.int64).reshape(-1)
        if ids.size != B or (ids < -1).any() or (ids >= R).any():
            raise ValueError(f"rir_ids must be {B} values in -1 .. {R - 1}")
        ids = ids.astype(np.int32)
    rir_lengths = rirs.lengths if rirs is not None else np.zeros(0, np.int32)
    add_off, adds = _additive_rows(additives, B, fs)
    M = len(noises) if noises is not None else 0
    if adds.shape[0] and ((adds[:, 0] < 0).any() or (adds[:, 0] >= M).any()):
        raise ValueError(f"additives: noise ids must lie in 0 .. {M - 1}")
    ylen = np.where((ids >= 0) & (n > 0), n.astype(np.int64) + (rir_lengths[np.maximum(ids, 0)] if R else 0) - 1, n.astype(np.int64))
    out_len = n.astype(np.int64) if shift_output else ylen
    T_out = int(out_len.max()) if B else 0
    out = torch.empty((B, T_out), dtype=out_dtype, device=dev)
    stats = torch.empty((B, L.AUG_STATS), dtype=torch.float64, device=dev)
    with L.launch_scope(dev):
        n_dev, ids_dev = torch.as_tensor(n, device=dev), torch.as_tensor(ids, device=dev)
        adds_dev = torch.as_tensor(adds, device=dev)
        ws = None
        for lo, hi in _row_chunks(n, ids, rir_lengths, fs, add_off, int(workspace_limit)):
            a0, a1 = int(add_off[lo]), int(add_off[hi])
            nbytes = ops.aug_workspace_bytes(n[lo:hi], ids[lo:hi], rir_lengths, fs, a1 - a0)
            if ws is None or ws.numel() < nbytes:
                ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            off_c = (add_off[lo:hi + 1] - a0).astype(np.int32)
            bank = (rirs.taps, rirs.offsets_dev, rirs.meta, rirs.spectra, rirs.tables) if R else (None,) * 5
            ops.aug_convolve(x[lo:hi], n[lo:hi], n_dev[lo:hi], ids[lo:hi], ids_dev[lo:hi], rir_lengths, fs, *bank, a1 - a0, stats[lo:hi], ws)
            ops.aug_mix(n[lo:hi], n_dev[lo:hi], ids[lo:hi], ids_dev[lo:hi], rir_lengths, fs, rirs.meta if R else None, off_c,
                        torch.as_tensor(off_c, device=dev), adds[a0:a1], adds_dev[a0:a1], noises.flat if M else None,
                        noises.offsets if M else np.zeros(1, np.int64), noises.offsets_dev if M else None, shift_output,
                        normalize_output, volume, out[lo:hi], stats[lo:hi], ws)
    lens = [int(v) for v in out_len]
    return (out, lens, stats) if return_stats else (out, lens)


# ----------------------------------------------------------------------------- sample-rate conversion (include/ktf_resample.h)
def _rate(rate, what):
    if not is_int(rate) or rate <= 0:
        raise ValueError(f"{what} must be a positive int, got {rate!r}")
    return int(rate)


class Resampler:
    """orig_rate -> new_rate (different positive ints) with Kaldi's LinearResample rules: lowpass_cutoff in Hz (None: 0.99 of the
    lower Nyquist frequency), num_zeros zero crossings of the sinc on each side. The polyphase plan is computed on the host here
    (`.iu` input and `.ou` output samples per repeating unit, `.first`, `.taps`, `.weights`) and uploaded once, at the first call.
    Only the ratio matters: Resampler(11, 10) and Resampler(17600, 16000) hold the same filter."""

    def __init__(self, orig_rate, new_rate, lowpass_cutoff=None, num_zeros=6, device=None):
        self.orig_rate, self.new_rate = _rate(orig_rate, "orig_rate"), _rate(new_rate, "new_rate")
        if self.orig_rate == self.new_rate:
            raise ValueError(f"Resampler: equal rates ({self.orig_rate}): nothing to resample (resample() passes such input through)")
        if not is_int(num_zeros) or num_zeros < 1:
            raise ValueError(f"num_zeros must be an int >= 1, got {num_zeros!r}")
        if lowpass_cutoff is None:
            lowpass_cutoff = 0.99 * 0.5 * min(self.orig_rate, self.new_rate)
        if not is_real(lowpass_cutoff) or not 0 < lowpass_cutoff <= 0.5 * min(self.orig_rate, self.new_rate):
            raise ValueError(f"lowpass_cutoff must lie in (0, {0.5 * min(self.orig_rate, self.new_rate)}], got {lowpass_cutoff!r}")
        self.cutoff, self.num_zeros = float(lowpass_cutoff), int(num_zeros)
        self.iu, self.ou, self.first, self.taps, self.weights = ops.rs_plan(self.orig_rate, self.new_rate, self.cutoff, self.num_zeros)
        L.require_gpu()
        self.device = torch.device(device) if device is not None else None
        self._dev = None

    def num_out(self, n):
        """Output samples of n input samples."""
        return ops.rs_num_out(n, self.orig_rate, self.new_rate)

    def _plan_on(self, device):
        if self._dev is None or self._dev[0] != device:
            self._dev = (device,) + tuple(torch.as_tensor(a, device=device) for a in (self.first, self.taps, self.weights))
        return self._dev[1:]

    def __call__(self, wavs, lengths=None, out_dtype=None):
        """wavs as augment() takes them, fp32 or int16 -> (out (B, T_out) on the device, out_dtype or the input's dtype, zeros past
        each row's length; lengths, B host ints). A row's bits depend on that row alone."""
        if out_dtype not in (None, torch.float32, torch.int16):
            raise ValueError(f"out_dtype must be torch.float32 or torch.int16, got {out_dtype}")
        L.require_gpu()
        x, n = _signals(wavs, lengths)
        if self.device is not None and x.device != self.device:
            raise ValueError(f"the Resampler lives on {self.device}, the signals on {x.device}")
        if n.size and int(n.max()) > L.RS_MAX_SAMPLES:
            raise ValueError("more than 2^30 samples in a row")
        m = [self.num_out(int(v)) for v in n]
        B, T_out = n.size, max(m, default=0)
        out = torch.empty((B, T_out), dtype=out_dtype or x.dtype, device=x.device)
        with L.launch_scope(x.device):
            first_dev, taps_dev, w_dev = self._plan_on(x.device)
            n_dev = torch.as_tensor(n, device=x.device)
            for lo in range(0, B, 65535):
                hi = min(B, lo + 65535)
                ops.rs_resample(x[lo:hi], n[lo:hi], n_dev[lo:hi], self.iu, self.ou, self.first, self.taps, first_dev, taps_dev, w_dev,
                                out[lo:hi])
        return out, m


def resample(wavs, orig_rate, new_rate, lengths=None, out_dtype=None, **kw):
    """One-shot Resampler(orig_rate, new_rate, **kw)(wavs, lengths, out_dtype). Equal rates return the input unfiltered (Kaldi's
    ResampleWaveform would low-pass it): a (B, T) tensor as it is, anything else as the padded (B, T) device tensor."""
    if _rate(orig_rate, "orig_rate") != _rate(new_rate, "new_rate"):
        return Resampler(orig_rate, new_rate, **kw)(wavs, lengths, out_dtype)
    if isinstance(wavs, torch.Tensor) and wavs.dim() == 2:
        B, T = wavs.shape
        n = np.full(B, T, np.int64) if lengths is None else host(lengths).astype(np.int64).reshape(-1)
        if n.size != B or (n < 0).any() or (n > T).any():
            raise ValueError(f"lengths must be {B} values in 0 .. {T}")
        x = wavs
    else:
        L.require_gpu()
        x, n = _signals(wavs, lengths)
    if out_dtype not in (None, x.dtype):
        raise ValueError(f"equal rates return the input as it is ({x.dtype}): out_dtype {out_dtype} would need a conversion")
    return x, [int(v) for v in n]


def speed_rates(factor):
    """The integer rates (p, q) a speed factor resamples between: fractions.Fraction(str(factor)) = p / q."""
    try:
        fr = fractions.Fraction(str(factor))
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"factor must be a positive number, got {factor!r}") from None
    if fr <= 0:
        raise ValueError(f"factor must be a positive number, got {factor!r}")
    return fr.numerator, fr.denominator


def speed_perturb(wavs, factor, lengths=None, out_dtype=None, **kw):
    """What `sox speed factor` does (utils/data/perturb_data_dir_speed.sh: 0.9 and 1.1): a resampling p -> q for factor = p / q whose
    result is read at the old rate, so 1.1 leaves 10 samples for every 11. factor 1 returns the input."""
    p, q = speed_rates(factor)
    return resample(wavs, p, q, lengths=lengths, out_dtype=out_dtype, **kw)
