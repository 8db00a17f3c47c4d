"""
ktf.layers — the reference's operator API (Keras layer protocol) on torch (ROCm) tensors.

Same class names, constructor kwargs, defaults, return conventions and exceptions as
kaldi_tflite/lib/layers/* of the reference; each `call` launches hand-written HIP kernels
through the C-ABI (see include/ktf_hip.h) instead of TensorFlow ops. The one deliberate
API difference is the tensor type (torch.Tensor on an MI355X instead of tf.Tensor).
"""

import collections
import itertools
import zlib

import numpy as np
import torch

from . import _lib as L
from . import ops
from ._host import chunks, host, is_int, max_under, per_device

_name_counters = collections.defaultdict(int)


def _auto_name(cls_name):
    base = "".join(("_" + c.lower()) if c.isupper() and i else c.lower() for i, c in enumerate(cls_name))
    base = {"m_f_c_c": "mfcc", "v_a_d": "vad", "c_m_v_n": "cmvn", "t_d_n_n": "tdnn", "d_c_t": "dct", "p_l_d_a": "plda",
            "re_l_u": "re_lu"}.get(base, base)
    n = _name_counters[base]
    _name_counters[base] += 1
    return base if n == 0 else f"{base}_{n}"


def _to_device(x):
    """numpy / CPU tensor -> device tensor (float64 is kept, everything else becomes float32)."""
    dev = ops._dev()
    if isinstance(x, torch.Tensor):
        if not x.is_cuda:
            x = x.to(dev)
        if x.dtype not in (torch.float32, torch.float64, torch.bfloat16):
            x = x.to(torch.float32)
        return x
    a = np.asarray(x)
    dt = np.float64 if a.dtype == np.float64 else np.float32
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)


class Layer:
    """Minimal stand-in for tf.keras.layers.Layer: name, build-on-first-call, get_config/from_config, weights."""

    def __init__(self, trainable=False, name=None, dtype="float32", **kwargs):
        if kwargs:
            # keras rejects unknown kwargs except a known few; mirror the permissive ones used by the reference tests
            allowed = {"input_shape", "batch_input_shape", "batch_size", "weights", "activity_regularizer", "autocast",
                       "implementation", "reduce"}
            bad = set(kwargs) - allowed
            if bad:
                raise TypeError(f"Keyword argument not understood: {sorted(bad)}")
        self.name = name if name is not None else _auto_name(type(self).__name__)
        self.trainable = trainable
        self.dtype = dtype
        self.built = False

    def build(self, input_shape):
        self.built = True

    def _maybe_build(self, inputs):
        if not self.built:
            self.build(tuple(inputs.shape))
            self.built = True

    def __call__(self, inputs, *args, **kwargs):
        inputs = _to_device(inputs)
        self._maybe_build(inputs)
        return self.call(inputs, *args, **kwargs)

    def call(self, inputs):
        raise NotImplementedError

    def get_config(self):
        return {"name": self.name, "trainable": self.trainable, "dtype": self.dtype}

    @classmethod
    def from_config(cls, config):
        # `trainable` and `dtype` are the base layer's own entries of get_config() (keras.layers.Layer takes them back); the layers here fix
        # both in their constructors, so a get_config() -> from_config() round trip drops them instead of passing them twice
        config = {k: v for k, v in dict(config).items() if k not in ("trainable", "dtype")}
        return cls(**config)

    def get_weights(self):
        return []

    def set_weights(self, weights):
        if len(weights) != 0:
            raise ValueError(f"layer {self.name} has no weights, got {len(weights)}")

    def compute_output_shape(self, input_shape):
        return input_shape


# =============================================================================== dsp
class Framing(Layer):
    """layers/dsp/framing.py:25 — frames of `frame_length_ms` every `frame_shift_ms`, no padding.

    Extensions (not in the reference): `snip_edges=False` frames the waveform as Kaldi's --snip-edges=false does, i.e. as
    if it had been mirror-padded with the reference's `kaldi_numpy.PadWaveform` (frame_extraction.py:54-89) first — done
    inside the frame gather on the device; int16 tensors are consumed as they are (no fp32 copy)."""

    def __init__(self, frame_length_ms=25.0, frame_shift_ms=10.0, sample_frequency=16000.0, name=None,
                 dynamic_input_shape=False, snip_edges=True, **kwargs):
        super().__init__(trainable=False, name=name, **kwargs)
        self.snipEdges = bool(snip_edges)
        self.sampleFreq = sample_frequency
        self.frameSizeMs = frame_length_ms
        self.frameShiftMs = frame_shift_ms
        self.dynamicInputShape = dynamic_input_shape
        self.batchAxis, self.sampleAxis = 0, -1
        if self.frameSizeMs <= 0 or self.frameShiftMs <= 0 or self.sampleFreq <= 0:
            raise ValueError("frame_length, frame_shift and sample_frequency should be > 0")
        self.frameSize = int(sample_frequency * frame_length_ms / 1000.0)
        self.frameShift = int(sample_frequency * frame_shift_ms / 1000.0)
        if self.frameSize <= 0:
            raise ValueError("frame_length should be high enough to contain at least 1 sample")
        if self.frameShift <= 0:
            raise ValueError("frame_shift should be high enough to shift by at least 1 sample")
        self.halfFrameSize = self.frameSize // 2
        self.frameWidth = 2 * self.halfFrameSize        # framing.py:104-106: offsets are range(-half, half)
        self.numInputSamples = None

    def build(self, input_shape):
        n = input_shape[self.sampleAxis]
        if n is None and not self.dynamicInputShape:
            raise ValueError("input_shape must not be unknown if dynamic_input_shape set to False")
        if n is not None:
            if n < self.minSamples():
                raise ValueError(f"input sample size (axis={self.sampleAxis}) must be >= frame size ({self.frameSize})")
            self.numInputSamples = n
        self.built = True

    def numFrames(self, n):
        if not self.snipEdges:
            # kaldi_numpy PadWaveform + Framing: M = round(n / shift) frames over the mirror-padded waveform
            M = (n + self.frameShift // 2) // self.frameShift
            Nv = (M - 1) * self.frameShift + self.frameWidth
            left = (self.frameWidth - self.frameShift) // 2
            right = (Nv - n) - left
            if M < 1 or Nv < n or left < 0 or right < 0 or left > n or right > n:
                raise ValueError(f"snip_edges=False: mirror padding is undefined for {n} samples")
            return M
        # centres = range(half, n - half + 1, shift)
        span = n - 2 * self.halfFrameSize
        return 0 if span < 0 else 1 + span // self.frameShift

    def minSamples(self):
        return self.frameSize if self.snipEdges else 1

    @staticmethod
    def device_samples(inputs):
        """(tensor, in_kind) the kernels read: int16 PCM stays int16, everything else becomes fp32."""
        x = inputs
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            if isinstance(x, np.ndarray) and x.dtype == np.int16:
                x = torch.as_tensor(x).to(ops.default_device())
            elif isinstance(x, torch.Tensor) and x.dtype == torch.int16:
                x = x.to(ops.default_device())
            else:
                x = ops.to_device_f32(x)
        kind = L.IN_WAV_I16 if x.dtype == torch.int16 else L.IN_WAV
        if x.dtype != torch.int16:
            x = x.to(torch.float32)
        # (B, N) views with unit sample stride are read in place: overlapping windows of one recording
        # (`wav.unfold(-1, N, hop)`, sliding-window / diarization extraction) are not materialised
        if not (x.dim() == 2 and x.stride(1) == 1 and 0 < x.stride(0) < 2**31):
            x = x.contiguous()
        return x, kind

    def compute_output_shape(self, input_shape):
        n = input_shape[self.sampleAxis]
        if n is None and not self.dynamicInputShape:
            raise ValueError("input_shape must not be unknown if dynamic_input_shape set to False")
        out = list(input_shape[:-1])
        out.extend([None if n is None else self.numFrames(n), self.frameWidth])
        return out

    def get_config(self):
        c = super().get_config()
        c.update({"frame_length": self.frameSizeMs, "frame_shift": self.frameShiftMs,
                  "sample_frequency": self.sampleFreq, "dynamic_input_shape": self.dynamicInputShape})
        if not self.snipEdges:
            c["snip_edges"] = False
        return c

    def _cfg(self):
        return L.FrontendCfg(frame_size=self.frameWidth, frame_shift=self.frameShift,
                             nfft=max(64, ops.next_power_of_2(self.frameWidth)), num_mels=1, num_ceps=1,
                             pad_mode=0 if self.snipEdges else 1)

    def call(self, inputs):
        x, kind = self.device_samples(inputs)
        n = x.shape[-1]
        if not self.dynamicInputShape and self.numInputSamples is not None and n != self.numInputSamples:
            raise ValueError(f"layer was built for {self.numInputSamples} samples, got {n}")
        if n < self.minSamples():
            raise ValueError(f"input sample size (axis={self.sampleAxis}) must be >= frame size ({self.frameSize})")
        lead = x.shape[:-1]
        B = int(np.prod(lead)) if len(lead) else 1
        T = self.numFrames(n)
        cfg = self._cfg()
        tables = per_device(self, x.device, lambda: ops.FrontendTables(self.frameWidth, device=x.device))
        if x.dim() == 2 and not x.is_contiguous():
            cfg.row_stride = x.stride(0)
        else:
            x = x.reshape(B, n)
        out = ops.frontend(x, kind, cfg, tables, L.OUT_FRAMES, n, B, T)
        if self.dynamicInputShape:
            return out.reshape(lead[0] if len(lead) else 1, -1, self.frameWidth)
        return out.reshape(*lead, T, self.frameWidth)


class Windowing(Layer):
    """layers/dsp/windowing.py:27."""

    def __init__(self, window_type="povey", blackman_coeff=0.42, dither=0.0, remove_dc_offset=True,
                 preemphasis_coefficient=0.97, return_energy=True, raw_energy=True, energy_floor=0.0, epsilon=1e-7,
                 name=None, **kwargs):
        super().__init__(trainable=False, name=name, **kwargs)
        self.preemphasisCoeff = preemphasis_coefficient
        if self.preemphasisCoeff < 0 or self.preemphasisCoeff > 1.0:
            raise ValueError("preemphasis_coefficient should be between 0.0 and 1.0")
        self.windowType = window_type.lower()
        if self.windowType not in ["hamming", "hanning", "povey", "rectangular", "sine", "blackman"]:
            raise ValueError(f"window_type '{window_type}' is not recognized")
        self.blackmanCoeff = blackman_coeff
        self.dither = dither
        self.removeDCOffset = remove_dc_offset
        self.returnEnergy = return_energy
        self.rawEnergy = raw_energy
        self.energyFloor = energy_floor
        self.eps = float(epsilon)
        self.windowFunc = None
        self.sampleAxis = -1
        self._seed = itertools.count(0x5EED + 1)      # (next() of a count is atomic: concurrent callers never draw the same dither seed)

    def build(self, input_shape):
        M = input_shape[self.sampleAxis]
        if M == 0:
            raise ValueError(f"window size (input shape axis = {self.sampleAxis}) needs to be > 0")
        self.windowFunc = ops.window_function(self.windowType, M, self.blackmanCoeff)
        self._M = M
        self._dev_cache = {}
        self.built = True

    def get_config(self):
        c = super().get_config()
        c.update({"window_type": self.windowType, "blackman_coeff": self.blackmanCoeff, "dither": self.dither,
                  "remove_dc_offset": self.removeDCOffset, "preemphasis_coefficient": self.preemphasisCoeff,
                  "return_energy": self.returnEnergy, "raw_energy": self.rawEnergy, "energy_floor": self.energyFloor,
                  "epsilon": self.eps})
        return c

    def _cfg(self, M):
        return L.FrontendCfg(frame_size=M, frame_shift=M, nfft=max(64, ops.next_power_of_2(M)), num_mels=1, num_ceps=1,
                             remove_dc=int(self.removeDCOffset), raw_energy=int(self.rawEnergy),
                             use_energy=int(self.returnEnergy), preemph=self.preemphasisCoeff, dither=self.dither,
                             energy_floor=self.energyFloor, eps=self.eps)

    def call(self, inputs):
        x = inputs.to(torch.float32).contiguous()
        M = x.shape[-1]
        if M != self._M:
            raise ValueError(f"layer was built for frames of {self._M} samples, got {M}")
        lead = x.shape[:-1]
        rows = int(np.prod(lead))
        tables = per_device(self, x.device, lambda: ops.FrontendTables(M, window=self.windowFunc, device=x.device))
        r = ops.frontend(x.reshape(1, rows, M), L.IN_FRAMES, self._cfg(M), tables, L.OUT_WINDOWED, rows, 1, rows,
                         seed=next(self._seed), want_energy=self.returnEnergy)
        if self.returnEnergy:
            out, en = r
            return out.reshape(*lead, M), en.reshape(*lead, 1)
        return r.reshape(*lead, M)


class FilterBank(Layer):
    """layers/dsp/filterbank.py:27 — zero-padded rFFT -> |.|(^2) -> mel bank -> log."""

    def __init__(self, num_bins=23, sample_frequency=16000.0, high_freq_cutoff=0.0, low_freq_cutoff=20.0,
                 use_log_fbank=True, use_power=True, epsilon=1e-7, name=None, **kwargs):
        super().__init__(trainable=False, name=name, **kwargs)
        self.numBins = num_bins
        if self.numBins <= 2:
            raise ValueError(f"num_bins must be >= 3, got {num_bins}")
        self.sampleFreq = sample_frequency
        self.nyquist = sample_frequency / 2.0
        if self.sampleFreq <= 0:
            raise ValueError(f"sample_frequency must be > 0, got {sample_frequency}")
        self.lowerCutoff = low_freq_cutoff
        if self.lowerCutoff > self.nyquist or self.lowerCutoff < 0:
            raise ValueError(f"low_freq_cutoff must be > 0 and < Nyquist Rate ({self.nyquist} Hz)")
        self.upperCutoff = high_freq_cutoff
        if self.upperCutoff <= 0:
            self.upperCutoff += self.nyquist
        if self.lowerCutoff >= self.upperCutoff:
            raise ValueError("lower_freq_cutoff must be < higher_freq_cutoff")
        self.useLogFBank = use_log_fbank
        self.usePower = use_power
        self.eps = float(epsilon)
        self.melBank = None
        self.fftLength = None
        self.sampleAxis = -1

    def build(self, input_shape):
        M = input_shape[self.sampleAxis]
        self.fftLength, self.melBank = ops.mel_bank_dense(M, self.numBins, self.sampleFreq, self.lowerCutoff, self.upperCutoff)
        self._M = M
        self._dev_cache = {}
        self.built = True

    def nextPowerOf2(self, n):
        return ops.next_power_of_2(n)

    def compute_output_shape(self, input_shape):
        out = list(input_shape)
        out[self.sampleAxis] = self.numBins
        return out

    def get_config(self):
        c = super().get_config()
        c.update({"sample_frequency": self.sampleFreq, "num_bins": self.numBins, "lower_freq_cutoff": self.lowerCutoff,
                  "upper_freq_cutoff": self.upperCutoff, "use_log_fbank": self.useLogFBank, "use_power": self.usePower,
                  "epsilon": self.eps})
        return c

    def call(self, inputs):
        x = inputs.to(torch.float32).contiguous()
        M = x.shape[-1]
        if M != self._M:
            raise ValueError(f"layer was built for frames of {self._M} samples, got {M}")
        lead = x.shape[:-1]
        rows = int(np.prod(lead))
        tables = per_device(self, x.device, lambda: ops.FrontendTables(M, mel_bank=self.melBank, device=x.device))
        cfg = L.FrontendCfg(frame_size=M, frame_shift=M, nfft=max(64, self.fftLength), num_mels=self.numBins, num_ceps=1,
                            use_power=int(self.usePower), use_log=int(self.useLogFBank), eps=self.eps)
        out = ops.frontend(x.reshape(1, rows, M), L.IN_WINDOWED, cfg, tables, L.OUT_FBANK, rows, 1, rows)
        return out.reshape(*lead, self.numBins)


class DCT(Layer):
    """layers/dsp/dct.py:27 — orthonormal DCT-II as a matmul (column 0 = sqrt(1/N))."""

    def __init__(self, length, dct_type=2, norm="ortho", name=None, **kwargs):
        super().__init__(trainable=False, name=name, **kwargs)
        self.length = length
        if self.length <= 0:
            raise ValueError(f"DCT length must be > 0, got {length}")
        self.dctType = dct_type
        if self.dctType not in [2]:
            raise NotImplementedError(f"DCT-{dct_type} is not supported yet")
        self.norm = norm.lower()
        if self.norm not in ["ortho"]:
            raise NotImplementedError(f"{norm} normalization is not supported yet")
        self.dct = None
        self.featAxis = -1

    def build(self, input_shape):
        featDim = input_shape[self.featAxis]
        if featDim < self.length:
            raise ValueError("input feature length must be >= DCT length")
        self.dct = ops.dct_matrix(featDim, self.length)
        self._dev_cache = {}
        self.built = True

    def compute_output_shape(self, input_shape):
        batch, time, _ = input_shape
        return (batch, time, self.length)

    def get_config(self):
        c = super().get_config()
        c.update({"length": self.length, "dct_type": self.dctType, "norm": self.norm})
        return c

    def call(self, inputs):
        x = inputs.to(torch.float32).contiguous()
        dct_dev = per_device(self, x.device, lambda: ops.to_device_f32(self.dct, x.device))
        lead = x.shape[:-1]
        out = ops.dct(x.reshape(-1, x.shape[-1]), dct_dev, None, self.length)
        return out.reshape(*lead, self.length)


class MFCC(Layer):
    """layers/dsp/mfcc.py:28 — Windowing -> FilterBank -> DCT -> lifter -> C0 <- log-energy, as ONE fused kernel."""

    def __init__(self, num_mfccs=23, num_mels=23, cepstral_lifter=22, use_energy=True, sample_frequency=16000.0,
                 high_freq_cutoff=0.0, low_freq_cutoff=20.0, use_log_fbank=True, use_power=True, window_type="povey",
                 dither=0.0, remove_dc_offset=True, preemphasis_coefficient=0.97, raw_energy=True, energy_floor=0.0,
                 epsilon=1e-7, name=None, **kwargs):
        super().__init__(trainable=False, name=name)
        self.numMfccs = num_mfccs
        self.melBins = num_mels
        self.cepstralLifter = cepstral_lifter
        self.useEnergy = use_energy
        if self.numMfccs > self.melBins:
            raise ValueError("num_mfccs must be <= num_mels")
        self.eps = float(epsilon)
        self.batchAxis, self.frameAxis, self.sampleAxis = 0, -2, -1
        self.lifters = ops.lifter_coeffs(self.numMfccs, self.cepstralLifter) if (self.numMfccs > 1 and self.cepstralLifter > 1) else None
        self.windowing = Windowing(window_type=window_type, dither=dither, remove_dc_offset=remove_dc_offset,
                                   preemphasis_coefficient=preemphasis_coefficient, raw_energy=raw_energy,
                                   return_energy=use_energy, energy_floor=energy_floor, epsilon=epsilon)
        self.filterbank = FilterBank(num_bins=num_mels, sample_frequency=sample_frequency,
                                     high_freq_cutoff=high_freq_cutoff, low_freq_cutoff=low_freq_cutoff,
                                     use_log_fbank=use_log_fbank, use_power=use_power, epsilon=epsilon)
        self.dct = DCT(length=num_mfccs, dct_type=2, norm="ortho")
        self._seed = itertools.count(0xC0FFEE + 1)    # (next() of a count is atomic: concurrent callers never draw the same dither seed)
        self._tables = {}

    def build(self, input_shape):
        M = input_shape[self.sampleAxis]
        self._prepare(M)
        self.built = True

    def _prepare(self, M):
        """(frame width) -> (FrontendCfg, host tables); shared by the stand-alone call and the fused extractor."""
        self.windowing.build((None, None, M))
        self.filterbank.build((None, None, M))
        self.dct.build((None, None, self.melBins))
        w, f = self.windowing, self.filterbank
        cfg = L.FrontendCfg(frame_size=M, frame_shift=M, nfft=max(64, f.fftLength), num_mels=self.melBins,
                            num_ceps=self.numMfccs, remove_dc=int(w.removeDCOffset), raw_energy=int(w.rawEnergy),
                            use_energy=int(self.useEnergy), use_power=int(f.usePower), use_log=int(f.useLogFBank),
                            use_lifter=int(self.cepstralLifter > 1 and self.lifters is not None), preemph=w.preemphasisCoeff,
                            dither=w.dither, energy_floor=w.energyFloor, eps=self.eps)
        self._M = M
        self._cfg = cfg
        return cfg

    def tables(self, device):
        key = (str(device), self._M)
        if key not in self._tables:
            self._tables[key] = ops.FrontendTables(self._M, window=self.windowing.windowFunc, mel_bank=self.filterbank.melBank,
                                                   dct=self.dct.dct, lifter=self.lifters, device=device)
        return self._tables[key]

    def compute_output_shape(self, input_shape):
        out = list(input_shape)
        out[self.sampleAxis] = self.numMfccs
        return out

    def get_config(self):
        c = super().get_config()
        c.update(self.windowing.get_config())
        c.update(self.filterbank.get_config())
        c.update({"num_mfccs": self.numMfccs, "num_mels": self.melBins, "cepstral_lifter": self.cepstralLifter,
                  "use_energy": self.useEnergy, "epsilon": self.eps})
        return c

    def next_seed(self):
        return next(self._seed)

    def call(self, inputs):
        x = inputs.to(torch.float32).contiguous()
        M = x.shape[-1]
        if M != self._M:
            raise ValueError(f"layer was built for frames of {self._M} samples, got {M}")
        B, T = x.shape[0], x.shape[-2]
        rows = x.numel() // M
        out = ops.frontend(x.reshape(1, rows, M), L.IN_FRAMES, self._cfg, self.tables(x.device), L.OUT_MFCC, rows, 1, rows,
                           seed=self.next_seed())
        return out.reshape(B, T, self.numMfccs)


class VAD(Layer):
    """layers/dsp/vad.py:23 — Kaldi energy VAD."""

    def __init__(self, energy_mean_scale=0.5, energy_threshold=5, frames_context=0, proportion_threshold=0.6,
                 return_indexes=True, energy_coeff=0, name=None, **kwargs):
        super().__init__(trainable=False, name=name, **kwargs)
        if energy_mean_scale < 0:
            raise ValueError("`energy_mean_scale` must be >= 0")
        if frames_context < 0:
            raise ValueError("`frames_context` must be >= 0")
        if proportion_threshold <= 0 or proportion_threshold >= 1:
            raise ValueError("`proportion_threshold` must be between 0 and 1 (exlcusive)")
        self.energyThreshold = float(energy_threshold)
        self.energyMeanScale = float(energy_mean_scale)
        self.propThreshold = float(proportion_threshold)
        self.returnIndexes = return_indexes
        self.useEnergyMean = energy_mean_scale > 0
        self.framesContext = frames_context
        self.windowSize = self.framesContext * 2 + 1
        self.energyCoef = energy_coeff
        self.frameAxis = -2

    def cfg(self):
        return L.VadCfg(energy_threshold=self.energyThreshold, energy_mean_scale=self.energyMeanScale,
                        proportion_threshold=self.propThreshold, frames_context=self.framesContext,
                        energy_coeff=self.energyCoef)

    def get_config(self):
        c = super().get_config()
        c.update({"energy_mean_scale": self.energyMeanScale, "energy_threshold": self.energyThreshold,
                  "frames_context": self.framesContext, "proportion_threshold": self.propThreshold,
                  "return_indexes": self.returnIndexes, "energy_coeff": self.energyCoef})
        return c

    def call(self, inputs):
        x = inputs.to(torch.float32).contiguous()
        if x.dim() == 2:
            x = x.unsqueeze(0)
        B, T, D = x.shape
        if self.returnIndexes:
            idx, lens = ops.vad_index(x, self.cfg())
            # tf.where row order: [batch, frame] ascending. The (n,2) shape is data dependent -> one host sync.
            lens_h = lens.cpu().tolist()
            rows = [torch.stack([torch.full((n,), b, dtype=torch.int64, device=x.device), idx[b, :n].to(torch.int64)], 1)
                    for b, n in enumerate(lens_h)]
            return torch.cat(rows, 0) if rows else torch.zeros((0, 2), dtype=torch.int64, device=x.device)
        return ops.vad_mask(x, self.cfg()).reshape(B, T, 1)


# =============================================================================== normalization
class CMVN(Layer):
    """layers/normalization/cmvn.py:25 — sliding-window cepstral mean (and variance) normalisation."""

    def __init__(self, center=True, norm_vars=False, window=600, min_window=100, padding="SAME", name=None, **kwargs):
        super().__init__(trainable=False, name=name)
        self.center = center
        self.normVar = norm_vars
        self.N = window
        self.minN = min_window
        if not self.center:
            raise NotImplementedError("CMVN with center=False not supported yet")
        if self.N <= 0 or self.minN <= 0:
            raise ValueError("`window` and `min_window` must be > 0")
        self.padding = padding.upper()
        if self.padding not in ["SAME", "VALID"]:
            raise ValueError(f"`padding` should be either 'SAME' or 'VALID', got '{padding}'")
        self.batchAxis, self.frameAxis, self.featAxis = 0, -2, -1

    def cfg(self):
        return L.CmvnCfg(window=self.N, norm_vars=int(self.normVar), valid=int(self.padding == "VALID"), reserved=0)

    def compute_output_shape(self, input_shape):
        if self.padding == "SAME":
            return input_shape
        out = list(input_shape)
        T = input_shape[self.frameAxis]
        if T is None:
            out[self.frameAxis] = None
        elif T <= self.N:
            out[self.frameAxis] = T
        else:
            out[self.frameAxis] = T - (2 * self.N - 1) // 2
        return out

    def get_config(self):
        c = super().get_config()
        c.update({"center": self.center, "norm_vars": self.normVar, "window": self.N, "min_window": self.minN,
                  "padding": self.padding})
        return c

    def call(self, inputs):
        x = inputs.to(torch.float32).contiguous()
        if x.dim() == 2:
            x = x.unsqueeze(0)
        B, T, D = x.shape
        out = ops.cmvn(x, self.cfg())
        if self.padding == "VALID":         # (cmvn.py:238-243: an input no longer than the window leaves no valid frame -- one when exactly as long)
            a, b = self.N // 2, T - (self.N - 1) // 2
            return out[:, : max(b - a, 0), :].contiguous()
        return out


class AddDeltas(Layer):
    """Extension (the reference has no delta features): Kaldi's `add-deltas --delta-order=order --delta-window=window`
    (DeltaFeatures; the sid recipes pass order 2, window 3). (B, T, D) or (T, D) fp32 on a GPU -> (B, T, D * (order + 1)): the input,
    then its order-1 .. order-`order` regression coefficients, frames beyond an utterance's ends clamped to its first / last frame.
    `lengths` (optional, B values): utterance b has lengths[b] frames; rows at and beyond them are written as zeros."""

    def __init__(self, order=2, window=2, name=None, **kwargs):
        super().__init__(trainable=False, name=name, **kwargs)
        if int(order) != order or int(window) != window or order < 0 or window < 1 or order * window > L.ADD_DELTAS_MAX_CONTEXT:
            raise ValueError(f"AddDeltas needs integers order >= 0, window >= 1, order * window <= {L.ADD_DELTAS_MAX_CONTEXT}; "
                             f"got order={order}, window={window}")
        self.order, self.window = int(order), int(window)
        self._coeffs = self.coefficients(self.order, self.window)

    @staticmethod
    def coefficients(order, window):
        """DeltaFeatures' scales in fp32: s_0 = [1]; s_i[j + k] += j * s_{i-1}[k] for j in [-window, window], divided by sum j^2.
        -> (order + 1, 2 * order * window + 1) fp32, row i centred at column order * window and zero beyond +- i * window."""
        f = np.float32
        ow = order * window
        out = np.zeros((order + 1, 2 * ow + 1), f)
        prev = np.ones(1, f)
        out[0, ow] = 1
        for i in range(1, order + 1):
            po = (len(prev) - 1) // 2
            cur = np.zeros(len(prev) + 2 * window, f)
            norm = f(0)
            for j in range(-window, window + 1):
                norm = f(norm + f(j * j))
                for k in range(-po, po + 1):
                    cur[j + k + po + window] = f(cur[j + k + po + window] + f(f(j) * prev[k + po]))
            cur = (cur / norm).astype(f)
            out[i, ow - i * window:ow + i * window + 1] = cur
            prev = cur
        return out

    def compute_output_shape(self, input_shape):
        out = list(input_shape)
        out[-1] = None if out[-1] is None else out[-1] * (self.order + 1)
        return out

    def get_config(self):
        c = super().get_config()
        c.update({"order": self.order, "window": self.window})
        return c

    def call(self, inputs, lengths=None):
        if not inputs.is_cuda:
            raise ValueError("AddDeltas computes on a GPU: the input must be a tensor on one")
        x = inputs.to(torch.float32)
        squeeze = x.dim() == 2
        if squeeze:
            x = x.unsqueeze(0)
        if x.dim() != 3 or x.shape[2] < 1:
            raise ValueError(f"AddDeltas takes (B, T, D) or (T, D), got {tuple(inputs.shape)}")
        B, T, D = x.shape
        if x.stride(2) != 1 or x.stride(1) < D or (B > 1 and x.stride(0) < 0):
            x = x.contiguous()
        n = None
        if lengths is not None:
            h = host(lengths, np.int64).reshape(-1)
            if h.shape[0] != B or (h < 0).any() or (h > T).any():
                raise ValueError(f"lengths must hold {B} values in 0 .. {T}")
            n = torch.as_tensor(h.astype(np.int32), device=x.device)
        coeffs = per_device(self, x.device, lambda: torch.as_tensor(self._coeffs, device=x.device))
        out = ops.add_deltas(x, n, coeffs, self.order, self.window)
        return out[0] if squeeze else out


class ReLU(Layer):
    """keras ReLU as used by models/kaldi/sequential.py:72 (stand-alone elementwise kernel)."""

    def __init__(self, name=None, **kwargs):
        super().__init__(trainable=False, name=name, **kwargs)

    def call(self, inputs):
        return ops.affine_act(inputs.to(torch.float32).contiguous(), L.ACT_RELU)


class BatchNorm(Layer):
    """layers/normalization/batchnorm.py:27 — keras BatchNormalization(center=False, scale=True) at inference with
    Kaldi weight import: y = gamma * (x - moving_mean) / sqrt(moving_var + eps)."""

    def __init__(self, axis=-1, momentum=0.99, target_rms=1.0, epsilon=0.001, mean_initializer=None,
                 variance_initializer=None, name=None, **kwargs):
        super().__init__(trainable=True, name=name, **kwargs)
        self.axis = axis
        self.momentum = momentum
        self.targetRMS = target_rms
        self.epsilon = epsilon
        self.gamma = self.moving_mean = self.moving_variance = None
        self._dev = None
        self._version = 0          # bumped by set_weights: consumers that folded this layer's affine into their weights re-fold

    def build(self, input_shape):
        D = input_shape[-1]
        if self.gamma is None:
            self.gamma = np.full((D,), self.targetRMS, np.float32)
            self.moving_mean = np.zeros((D,), np.float32)
            self.moving_variance = np.ones((D,), np.float32)
        self.built = True

    def get_config(self):
        c = super().get_config()
        c.update({"axis": self.axis, "momentum": self.momentum, "epsilon": self.epsilon, "target_rms": self.targetRMS})
        return c

    def get_weights(self):
        return [self.gamma, self.moving_mean, self.moving_variance]

    def set_weights(self, weights, fmt="kaldi"):
        if fmt not in ["kaldi", "tensorflow"]:
            raise ValueError(f"expected 'fmt' to be either 'kaldi' or 'tensorflow', got {fmt}")
        if len(weights) != 3:
            raise ValueError(f"expected a weight list of length 3, got {len(weights)}")
        if fmt == "tensorflow":
            gamma, mean, var = [np.asarray(w, np.float32) for w in weights]
        else:
            targetRMS, mean, var = weights
            mean = np.asarray(mean, np.float32)
            var = np.asarray(var, np.float32)
            gamma = (np.float32(targetRMS) * np.ones_like(mean)).astype(np.float32)
        if not (gamma.shape == mean.shape == var.shape):
            raise ValueError("gamma / mean / variance shapes differ")
        self.gamma, self.moving_mean, self.moving_variance = gamma, mean, var
        self._dev = None
        self._version += 1
        WEIGHTS_EPOCH[0] += 1

    def affine64(self):
        """(scale, shift) of the inference transform y = scale * x + shift, float64."""
        g = self.gamma.astype(np.float64)
        scale = g / np.sqrt(self.moving_variance.astype(np.float64) + self.epsilon)
        return scale, -self.moving_mean.astype(np.float64) * scale

    def affine(self):
        """(scale, shift) of the inference transform, computed in float64 on the host."""
        scale, shift = self.affine64()
        return scale.astype(np.float32), shift.astype(np.float32)

    def affine_device(self, device):
        if self._dev is None or self._dev[0].device != torch.device(device):
            s, h = self.affine()
            self._dev = (ops.to_device_f32(s, device), ops.to_device_f32(h, device))
        return self._dev

    def call(self, inputs, training=False):
        if training:
            raise NotImplementedError("training-mode batch normalisation is not part of the inference path")
        x = inputs.to(torch.float32).contiguous()
        s, h = self.affine_device(x.device)
        return ops.affine_act(x, L.ACT_NONE, s, h)


# =============================================================================== tdnn
def reshapeKaldiTdnnWeights(weights, units, kernel_width):
    """layers/tdnn/utils.py:22-28: Kaldi (units, K*D) -> keras conv2d kernel (1, K, D, units)."""
    return weights.flatten().reshape((1, -1, kernel_width, units), order="F").transpose([0, 2, 1, 3])


WEIGHTS_EPOCH = [0]      # bumped by every set_weights / re-build in the process: a cheap "anything changed?" for captured graphs

# every name tf.keras.activations.get resolves in the reference's TensorFlow (2.8; layers/tdnn/tdnn.py:117-118). The GEMM epilogues
# fuse the first four; the others run as a second launch over the layer's output (ktf_tdnn does that itself, fp32 kernels only)
_ACTS = {None: L.ACT_NONE, "linear": L.ACT_NONE, "relu": L.ACT_RELU, "sigmoid": L.ACT_SIGMOID, "tanh": L.ACT_TANH,
         "elu": L.ACT_ELU, "selu": L.ACT_SELU, "softplus": L.ACT_SOFTPLUS, "softsign": L.ACT_SOFTSIGN, "swish": L.ACT_SWISH,
         "gelu": L.ACT_GELU, "exponential": L.ACT_EXPONENTIAL, "hard_sigmoid": L.ACT_HARD_SIGMOID, "softmax": L.ACT_SOFTMAX}
_GEMM = {"f32": L.GEMM_F32, "float32": L.GEMM_F32, "bf16": L.GEMM_BF16, "bfloat16": L.GEMM_BF16, "bf16x3": L.GEMM_BF16X3,
         "f16mx": L.GEMM_F16MX}


class TDNN(Layer):
    """layers/tdnn/tdnn.py:29 — irregular-context 1-D convolution as an implicit-im2col MFMA GEMM."""

    MAX_DEVICE_SETS = 4        # device operand sets kept per layer AND DEVICE (keyed by mode / layout): the oldest set of
                               # the same device is evicted; sets on other devices (other ranks' streams may be reading them) stay

    def __init__(self, units, context=[0], subsampling_factor=1, padding="SAME", use_bias=True, kernel_initializer=None,
                 bias_initializer=None, activation=None, name=None, gemm="f32", **kwargs):
        super().__init__(trainable=True, name=name, **kwargs)
        self.units = units
        self.useBias = use_bias
        self.subsamplingFactor = subsampling_factor
        if self.subsamplingFactor <= 0:
            raise ValueError("subsampling_factor should be > 0")
        self.padding = padding.upper()
        if self.padding not in ["VALID", "SAME"]:
            raise ValueError("padding should be either 'VALID' or 'SAME'")
        if context is None:
            self.context = [0]
        elif isinstance(context, int):
            self.context = [context]
        elif isinstance(context, list):
            self.context = context if len(context) > 0 else [0]
        else:
            raise ValueError("context should be None, a list or an integer")
        self.context.sort()
        self.kernelWidth = len(self.context)
        self.kernelInitializer = kernel_initializer
        self.biasInitializer = bias_initializer
        self.activation = activation
        if isinstance(activation, str) and activation.lower() not in _ACTS:
            raise ValueError(f"Unknown activation function: {activation}")
        if gemm not in _GEMM:
            raise ValueError(f"gemm must be one of {sorted(_GEMM)}")
        self.gemm = gemm
        self.batchAxis, self.timeAxis, self.featAxis = 0, 1, -1
        self.kernel = None     # keras layout (1, K, D, units), numpy fp32
        self.bias = None
        self.kernelFlags = 0   # KtfTdnnDesc.flags of this layer's launches (L.TDNN_REF_TILES: bitwise-reference fp32 tiles)
        self._dev = {}
        self._version = 0      # bumped whenever the weights change: models refuse stale captured graphs

    # ---- weights
    def build(self, input_shape):
        D = input_shape[self.featAxis]
        self.inputDim = D
        if self.kernel is None or self.kernel.shape != (1, self.kernelWidth, D, self.units):
            # Glorot-uniform like the reference's default initialisers (tdnn.py:40-41)
            # seeded from the layer NAME with a process-independent hash: every rank of a multi-GPU job draws the same
            # initial weights for a layer that is not found in the nnet3 file
            rng = np.random.default_rng(zlib.crc32(self.name.encode()))
            fan_in, fan_out = self.kernelWidth * D, self.kernelWidth * self.units
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            self.kernel = rng.uniform(-lim, lim, (1, self.kernelWidth, D, self.units)).astype(np.float32)
            if self.useBias:
                lb = np.sqrt(6.0 / (self.units + 1))
                self.bias = rng.uniform(-lb, lb, (self.units,)).astype(np.float32)
            self._version += 1
            WEIGHTS_EPOCH[0] += 1
        self._dev = {}
        self.built = True

    def get_weights(self):
        return [self.kernel, self.bias] if self.useBias else [self.kernel]

    def set_weights(self, weights, fmt="kaldi"):
        fmt = fmt.lower()
        if fmt not in ["kaldi", "tensorflow"]:
            raise ValueError(f"expected 'fmt' to be either 'kaldi' or 'tensorflow', got {fmt}")
        if len(weights) == 0:
            raise ValueError("expected a weight list of at least length 2, got 0")
        if self.useBias and len(weights) != 2:
            raise ValueError(f"expected a weight list of length 2, got {len(weights)}")
        kernel = np.asarray(weights[0], np.float32)
        if fmt == "kaldi":
            kernel = reshapeKaldiTdnnWeights(kernel, self.units, self.kernelWidth)
        if self.built and kernel.shape != (1, self.kernelWidth, self.inputDim, self.units):
            raise ValueError(f"Layer weight shape {(1, self.kernelWidth, self.inputDim, self.units)} not compatible with "
                             f"provided weight shape {kernel.shape}")
        if kernel.ndim != 4 or kernel.shape[0] != 1 or kernel.shape[1] != self.kernelWidth or kernel.shape[3] != self.units:
            raise ValueError(f"weight shape {kernel.shape} does not match (1, {self.kernelWidth}, D, {self.units})")
        self.kernel = np.ascontiguousarray(kernel)
        self.inputDim = kernel.shape[2]
        if self.useBias:
            bias = np.asarray(weights[1], np.float32).reshape(-1)
            if bias.shape != (self.units,):
                raise ValueError(f"bias shape {bias.shape} != ({self.units},)")
            self.bias = bias
        self._dev = {}
        self._version += 1
        WEIGHTS_EPOCH[0] += 1
        self._warned_fp32_fallback = set()       # (warn_fallback speaks again for the new weights)
        self.built = True

    def kaldi_matrix(self):
        """(units, K*D) Kaldi layout of the kernel."""
        K, D = self.kernelWidth, self.inputDim
        return np.ascontiguousarray(self.kernel[0].reshape(K * D, self.units).T)

    def device_weights(self, device, gemm, k_interleaved=False, w_tiled=False):
        """Padded GEMM operands on the device: W (units_pad, K*Dpad) in the GEMM's dtype (+ lo part for the split-bf16 mode),
        bias. `k_interleaved`: K axis ordered (32-feature chunk, context, feature) — KTF_TDNN_K_INTERLEAVED, `w_tiled`: the
        kernel's LDS stage images (KTF_TDNN_W_TILED); both for the split-plane kernel."""
        key = (str(device), gemm, bool(k_interleaved), bool(w_tiled))
        if key in self._dev:
            return self._dev[key]
        K, D = self.kernelWidth, self.inputDim
        Dp, Up = ops.round_up(D, 32), ops.round_up(self.units, 256)
        Wk = np.transpose(self.kernel[0], (2, 0, 1)).astype(np.float64)       # [u, k, d]
        bias64 = self.bias.astype(np.float64) if self.useBias else None
        W = np.zeros((Up, K, Dp), np.float64)
        W[: self.units, :, :D] = Wk
        if k_interleaved:
            W = np.ascontiguousarray(W.reshape(Up, K, Dp // 32, 32).transpose(0, 2, 1, 3))
        W = W.reshape(Up, K * Dp)
        if w_tiled:
            # KTF_TDNN_W_TILED: (N-tile, K-step) blocks in the kernel's LDS image order: row r keeps its four 16-byte chunks
            # at positions chunk ^ ((4 - (r >> 2)) & 3)
            nt, nks = Up // 256, K * Dp // 32
            r = np.arange(256)
            src = np.arange(4)[None, :] ^ ((4 - ((r >> 2) & 3)) & 3)[:, None]              # [row, position] -> chunk
            W5 = W.reshape(nt, 256, nks, 4, 8)
            W = np.ascontiguousarray(W5[:, r[:, None], :, src, :].transpose(2, 3, 0, 1, 4)).reshape(Up, K * Dp)
        W = torch.as_tensor(W, device=device)
        w_lo = None
        if gemm == L.GEMM_F32:
            w = W.to(torch.float32)
        elif gemm == L.GEMM_BF16X4:
            w = ops.pair_encode(W.to(torch.float32))
        else:
            W = W.to(torch.float32)
            w = W.to(torch.bfloat16)
            if gemm == L.GEMM_BF16X3:
                w_lo = (W - w.to(torch.float32)).to(torch.bfloat16)
        bias = ops.to_device_f32(bias64, device) if bias64 is not None else None
        mine = [k for k in self._dev if k[0] == str(device)]
        while len(mine) >= self.MAX_DEVICE_SETS:             # mode changes replace operand sets: evict this device's oldest
            self._dev.pop(mine.pop(0))
        self._dev[key] = (w, w_lo, bias)
        return self._dev[key]

    def device_weights_mx(self, device, fold=None, loader=True, kernel=None):
        """KTF_GEMM_F16MX operands on the device: (wh, wq, bias) -- the half plane and the block-scaled e2m1 / e2m3 planes of
        the weights as the LDS images of the kernel that will read them (include/ktf_hip.h, ktf_tdnn_mx). `kernel`: "tile" = the
        256 x 256 kernel (mx.weight_images), "loader" = the loader-wave kernel (KTF_TDNN_MX_LOADER: mx.weight_images_loader);
        None: "loader" / "tile" by `loader`. K ordered (32-feature chunk, context, feature) and zero-padded to
        whole super-steps. `fold`: the BatchNorm whose affine y = s*x + h precedes this layer, folded INTO it so that the stored
        activations are the ReLU outputs themselves: W'[u,k,d] = W[u,k,d] * s[d], b'[u] = b[u] + sum_kd W[u,k,d] * h[d] (float64 on
        the host; exact for replicate padding, every context row carries the same per-feature affine)."""
        from . import mx
        kernel = kernel or ("loader" if loader else "tile")
        if kernel not in ("loader", "tile"):
            raise ValueError(f"unknown f16mx kernel {kernel!r}")
        key = ("mx", str(device), None if fold is None else (id(fold), fold._version), kernel)
        if key in self._dev:
            return self._dev[key]
        K, D = self.kernelWidth, self.inputDim
        Dp, Up = ops.round_up(D, 32), ops.round_up(self.units, 256)
        Wk = np.transpose(self.kernel[0], (2, 0, 1)).astype(np.float64)       # [u, k, d]
        bias64 = self.bias.astype(np.float64) if self.useBias else None
        if fold is not None:
            s64, h64 = fold.affine64()
            if s64.shape != (D,):
                raise ValueError(f"cannot fold a {s64.shape[0]}-wide BatchNorm into a layer with input dim {D}")
            extra = np.einsum("ukd,d->u", Wk, h64)
            bias64 = extra if bias64 is None else bias64 + extra
            Wk = Wk * s64[None, None, :]
        W = np.zeros((Up, K, Dp), np.float64)
        W[: self.units, :, :D] = Wk
        W = np.ascontiguousarray(W.reshape(Up, K, Dp // 32, 32).transpose(0, 2, 1, 3)).reshape(Up, (Dp // 32) * K, 32)
        wh, wq, _ = mx.weight_images_loader(W) if kernel == "loader" else mx.weight_images(W)
        out = (torch.as_tensor(wh, device=device), torch.as_tensor(wq, device=device),
               ops.to_device_f32(bias64, device) if bias64 is not None else None)
        # one MX image set per (layer, device, kernel): a re-fold replaces the set of its own device and kernel only
        self._dev = {k: v for k, v in self._dev.items() if not (k[0] == "mx" and k[1] == key[1] and k[3] == key[3])}
        self._dev[key] = out
        return out

    def desc(self, gemm, x_dtype, y_dtype, act=None, flags=0):
        d = L.TdnnDesc()
        d.flags = flags
        d.units, d.din, d.din_pad, d.nctx = self.units, self.inputDim, ops.round_up(self.inputDim, 32), self.kernelWidth
        for i, c in enumerate(self.context):
            d.ctx[i] = int(c)
        d.subsampling, d.valid = self.subsamplingFactor, int(self.padding == "VALID")
        a = self.activation if act is None else act
        d.act = _ACTS[a.lower() if isinstance(a, str) else a]
        d.gemm = gemm
        d.x_dtype = L.ktf_dtype(x_dtype)
        d.w_dtype = {L.GEMM_F32: L.KTF_F32, L.GEMM_BF16X4: L.KTF_BF16P}.get(gemm, L.KTF_BF16)
        d.y_dtype = L.ktf_dtype(y_dtype)
        return d

    def getStartEndSteps(self, T):
        start, end = 0, T
        if self.padding == "VALID":
            if self.context[0] < 0:
                start = -1 * self.context[0]
            if self.context[-1] > 0:
                end = T - self.context[-1]
        return start, end

    def outputTimesteps(self, T):
        start, end = self.getStartEndSteps(T)
        n = end - start
        return 0 if n <= 0 else (n + self.subsamplingFactor - 1) // self.subsamplingFactor

    def compute_output_shape(self, input_shape):
        B, T = input_shape[self.batchAxis], input_shape[self.timeAxis]
        return (B, None if T is None else self.outputTimesteps(T), self.units)

    def get_config(self):
        c = super().get_config()
        c.update({"units": self.units, "context": self.context, "subsampling_factor": self.subsamplingFactor,
                  "padding": self.padding, "use_bias": self.useBias, "activation": self.activation})
        return c

    def forward(self, x, lens=None, relu=False, bn=None, gemm=None, out_dtype=torch.float32, ldy=None, out=None,
                out_lens=None, flags=0, pair_in=False, pair_out=False):
        """Low-level launch used by call() and by the fused Sequential runner.
        x: (B, T, ldx) fp32/bf16 with ldx >= round_up(D,32) (pad columns finite). Returns y (B, Tout, ldy).
        `pair_in` (gemm GEMM_BF16X4) / `pair_out` (GEMM_F32 or GEMM_BF16X4): the float32 tensor x / y holds KTF_BF16P pairs."""
        gemm = _GEMM[self.gemm] if gemm is None else gemm
        if pair_in != (gemm == L.GEMM_BF16X4):
            raise ValueError("KTF_GEMM_BF16X4 reads pairs, and only it does")
        w, w_lo, bias = self.device_weights(x.device, gemm)
        act = "relu" if relu else None
        if relu and self.activation not in (None, "linear"):
            raise ValueError("cannot fuse a ReLU after a TDNN that already has an activation")
        d = self.desc(gemm, L.PAIR if pair_in else x.dtype, L.PAIR if pair_out else out_dtype, act=act if relu else None,
                      flags=0 if pair_in else flags | self.kernelFlags)
        B, T = x.shape[0], x.shape[1]
        Tout = self.outputTimesteps(T)
        ldy = self.units if ldy is None else ldy
        if out is None:
            alloc = torch.zeros if ldy != self.units else torch.empty
            out = alloc((B, Tout, ldy), dtype=out_dtype, device=x.device)
        scale, shift = bn if bn is not None else (None, None)
        if Tout > 0 and B > 0:
            ops.tdnn(x, lens, d, w, w_lo, bias, scale, shift, out, out_lens)
        elif out_lens is not None:                  # no output row (VALID padding of inputs shorter than the context): every utterance is empty
            out_lens.zero_()
        return out

    def effective_gemm(self, gemm, relu=False):
        """The f16mx mode runs on the MX kernels only (units > 128, ReLU or no activation); any other layer of
        such a model is evaluated by the exact fp32 kernel instead. A pure query (the fused runner's planner asks it for every
        layer, and for the layer behind it): `warn_fallback` is what tells the user."""
        return L.GEMM_F32 if self.fallback_reason(gemm, relu) else gemm

    def fallback_reason(self, gemm, relu=False):
        """Why this layer runs on the exact fp32 kernels in a model of mode `gemm` (None: it does not)."""
        a = self.activation.lower() if isinstance(self.activation, str) else self.activation
        if gemm == L.GEMM_F32:
            return None
        if _ACTS[a] > L.ACT_TANH:            # activations no epilogue fuses: the fp32 kernels + an activation pass, in every mode
            return f"activation {self.activation!r} is not fused by any reduced-precision epilogue"
        if gemm != L.GEMM_F16MX:
            return None
        if self.units <= 128:
            return f"units = {self.units} (these kernels tile 256 units: layers of up to 128 stay on fp32)"
        if not (a in (None, "linear") or (a == "relu" and not relu)):
            return (f"activation {self.activation!r}" + (" followed by a ReLU" if relu else "") + " (these kernels fuse ReLU or no activation)")
        return None

    def warn_fallback(self, gemm, relu=False):
        """One RuntimeWarning per (layer, mode) naming the condition that keeps the layer off the mode's kernels; called where the
        layer is about to run (TDNN.call, the fused runner), re-armed by set_weights."""
        why = self.fallback_reason(gemm, relu)
        if why is None or gemm in self.__dict__.setdefault("_warned_fp32_fallback", set()):
            return
        import warnings
        self._warned_fp32_fallback.add(gemm)
        mode = {v: k for k, v in _GEMM.items()}.get(gemm, str(gemm))
        warnings.warn(f"TDNN layer '{self.name}' runs on the exact fp32 kernels in this '{mode}' model: {why} "
                      f"(several times slower per flop; its results are the more accurate ones)", RuntimeWarning, stacklevel=3)

    def prepare_input(self, x, gemm):
        """Dense user tensor (B,T,D) -> operand the GEMM can read (padded to a multiple of 32 columns, right dtype)."""
        D = x.shape[-1]
        Dp = ops.round_up(D, 32)
        want = L.act_torch_dtype(gemm)
        if D == Dp and x.dtype == want and x.is_contiguous():
            return x
        if x.dtype not in (torch.float32, torch.bfloat16) or (x.dtype != torch.float32 and x.dtype != want):
            x = x.to(torch.float32)
        dst = torch.empty((*x.shape[:-1], Dp), dtype=want, device=x.device)
        return ops.convert_pad(x.contiguous(), D, dst)

    def call(self, inputs):
        x = inputs
        if x.dim() != 3:
            raise ValueError(f"expected a (batch, time, feat) input, got shape {tuple(x.shape)}")
        if x.shape[-1] != self.inputDim:
            raise ValueError(f"expected input feature dim {self.inputDim}, got {x.shape[-1]}")
        self.warn_fallback(_GEMM[self.gemm])
        gemm = self.effective_gemm(_GEMM[self.gemm])
        B, T, D = x.shape
        if gemm == L.GEMM_F16MX:
            return self._call_mx(x)
        # the 16-bit ring kernels want an output row stride that is a multiple of 8 (16-byte stores); the pad columns
        # are sliced off again
        ldy = ops.round_up(self.units, 8) if gemm == L.GEMM_BF16 else self.units
        if T == 1 and list(self.context) == [0] and self.subsamplingFactor == 1 and B > 1:
            # one row per utterance (e.g. the affine after stats pooling): run as ONE B-row GEMM (context [0] only: another offset
            # would clamp to the neighbouring UTTERANCES' rows there, not to the utterance's single frame)
            y = self.forward(self.prepare_input(x.reshape(1, B, D), gemm), gemm=gemm, ldy=ldy)
            return y[:, :, : self.units].reshape(B, 1, self.units)
        return self.forward(self.prepare_input(x, gemm), gemm=gemm, ldy=ldy)[:, :, : self.units]


    def _call_mx(self, x):
        """A stand-alone call of an "f16mx" layer (inside a Sequential the planes travel from layer to layer instead): fp32 rows ->
        the four MX planes -> csrc/tdnn_mx.hip -> fp32 rows."""
        from . import mx
        B, T, D = x.shape
        planes = mx.Planes.empty(B, T, D, x.device)
        ops.mx_planes(_f32_rows(x), D, None, planes)
        wh, wq, bias = self.device_weights_mx(x.device, loader=False)
        d = self.desc(L.GEMM_F16MX, torch.float32, torch.float32)
        if self.outputTimesteps(T) <= 0:               # VALID padding of an input shorter than the context: no output row
            return torch.empty((B, 0, self.units), dtype=torch.float32, device=x.device)
        y = torch.empty((B, self.outputTimesteps(T), ops.round_up(self.units, 4)), dtype=torch.float32, device=x.device)
        ops.tdnn_mx(planes, None, d, wh, wq, bias, None, None, y)
        return y[:, :, : self.units]


def _f32_rows(x):
    """(B, T, D) x as fp32 rows of one stride per utterance: x itself if it is that already, else a contiguous copy."""
    if x.dtype == torch.float32 and x.stride(2) == 1 and x.stride(0) == x.shape[1] * x.stride(1):
        return x
    return x.to(torch.float32).contiguous()


# =============================================================================== stats
class StatsPooling(Layer):
    """layers/stats/stats_pooling.py:26 — mean (+ std) pooling over the whole utterance or sliding windows."""

    def __init__(self, left_context, right_context, input_period=1, output_period=1, include_std=True, padding="SAME",
                 epsilon=1e-10, reduce_time_axis=False, name=None, **kwargs):
        super().__init__(trainable=False, name=name)
        self.leftContext = left_context
        self.rightContext = right_context
        self.inputPeriod = input_period
        self.outputPeriod = output_period
        self.includeStd = include_std
        self.reduce = reduce_time_axis
        if self.leftContext > 0 or self.rightContext < 0:
            raise ValueError("'left_context' must be <= 0 and 'right_context' must be >= 0")
        if self.inputPeriod <= 0 or self.outputPeriod <= 0:
            raise ValueError("'input_period' and 'output_period' must be > 0")
        if self.outputPeriod % self.inputPeriod != 0 and not self.reduce:
            raise ValueError("'output_period' must be a multiple of 'input_period'")
        self.padding = padding.upper()
        if self.padding not in ["VALID", "SAME"]:
            raise ValueError("padding should be either 'VALID' or 'SAME'")
        self.epsilon = float(epsilon)
        self.maxWindowWidth = right_context - left_context + 1
        self.batchAxis, self.timeAxis, self.featAxis = 0, 1, -1

    def getStartEndSteps(self, T):
        start, end = 0, T
        if self.padding == "SAME":
            return start, end
        if self.leftContext < 0:
            start = -1 * self.leftContext
        if self.rightContext > 0 and self.maxWindowWidth < T:
            end = T - self.rightContext
        return start, end + 1

    def numOutputSteps(self, T):
        start, end = self.getStartEndSteps(T)
        n = end - start
        return 0 if n <= 0 else (n + self.outputPeriod - 1) // self.outputPeriod

    def compute_output_shape(self, input_shape):
        B, T, D = input_shape[self.batchAxis], input_shape[self.timeAxis], input_shape[self.featAxis]
        if self.includeStd:
            D = D * 2
        if self.reduce:
            return (B, 1, D)
        if self.padding == "SAME" or T is None:          # (a model built for any number of frames: the time axis stays unknown)
            return (B, T, D)
        return (B, self.numOutputSteps(T), D)

    def get_config(self):
        c = super().get_config()
        c.update({"left_context": self.leftContext, "right_context": self.rightContext, "input_period": self.inputPeriod,
                  "output_period": self.outputPeriod, "include_std": self.includeStd, "padding": self.padding,
                  "epsilon": self.epsilon, "reduce_time_axis": self.reduce})
        return c

    def reduce_all(self, x, D, lens=None, out=None):
        """(B,T,ld) -> (B, 1, D or 2D) over the valid rows of each utterance."""
        od = 2 * D if self.includeStd else D
        if out is None:
            out = torch.empty((x.shape[0], od), dtype=torch.float32, device=x.device)
        ops.stats_pool(x, D, lens, self.inputPeriod, self.includeStd, self.epsilon, out)
        return out

    def call(self, inputs):
        x = inputs if inputs.dtype in (torch.float32, torch.bfloat16) else inputs.to(torch.float32)
        x = x.contiguous()
        B, T, D = x.shape
        od = 2 * D if self.includeStd else D
        if self.reduce:
            return self.reduce_all(x, D).reshape(B, 1, od)
        if T == 0 and self.padding == "SAME":        # no frame, no window (a VALID-padded layer in front left nothing); with VALID
            return torch.empty((B, 0, od), dtype=torch.float32, device=x.device)      # padding the reference pools "all" frames: one NaN row, below
        x = x.to(torch.float32)
        if self.padding == "SAME":
            n = self.numOutputSteps(T)
            s = ops.stats_pool_windowed(x, self.leftContext, self.rightContext, self.inputPeriod, self.outputPeriod, 0, n,
                                        self.includeStd, self.epsilon)
            if self.outputPeriod > 1:
                # tf.repeat(stats, output_period, axis=time): row j -> rows j*p .. j*p+p-1 (pure data movement)
                s = s.repeat_interleave(self.outputPeriod, dim=1)
            return s
        if T > self.maxWindowWidth:
            start, _ = self.getStartEndSteps(T)
            return ops.stats_pool_windowed(x, self.leftContext, self.rightContext, self.inputPeriod, self.outputPeriod,
                                           start, self.numOutputSteps(T), self.includeStd, self.epsilon)
        return self.reduce_all(x, D).reshape(B, 1, od)


class AttentiveStatsPooling(Layer):
    """Attentive statistics pooling (Okabe et al. 2018): e = W2^T act(W1^T h + b1) + b2 per frame, a softmax of e over the frames of
    the utterance, and the weighted mean (+ standard deviation) of h under it (include/ktf_attn.h). `heads` = 1: one weight per frame;
    1 < heads < D: channel c is weighted by head c // (D / heads); heads = D: one weight per frame and channel. The two affines are
    context-[0] TDNN layers held by this layer; the weights in keras order are [W1 (D, A), b1 (A,), W2 (A, H), b2 (H,)]."""

    def __init__(self, attention_units, heads=1, include_std=True, epsilon=1e-10, attention_activation="tanh", name=None, **kwargs):
        super().__init__(trainable=True, name=name, **kwargs)
        self.attentionUnits, self.heads = int(attention_units), int(heads)
        if self.attentionUnits < 1 or self.heads < 1:
            raise ValueError("'attention_units' and 'heads' must be >= 1")
        if float(epsilon) < 0 or not np.isfinite(float(epsilon)):
            raise ValueError("'epsilon' must be finite and >= 0")
        self.includeStd = bool(include_std)
        self.epsilon = float(epsilon)
        self.attentionActivation = attention_activation
        self.reduce = True             # the whole utterance, as a StatsPooling(reduce_time_axis=True): the fused runner's tail treats it alike
        self.hidden = TDNN(self.attentionUnits, [0], activation=attention_activation, name=self.name + ".hidden")
        self.logits = TDNN(self.heads, [0], name=self.name + ".logits")
        self.gemm = "f32"
        self.batchAxis, self.timeAxis, self.featAxis = 0, 1, -1

    @property
    def _version(self):
        return self.hidden._version + self.logits._version

    def build(self, input_shape):
        D = input_shape[self.featAxis]
        if D % self.heads:
            raise ValueError(f"'heads' = {self.heads} does not divide the {D} input channels")
        self.inputDim = D
        if not self.hidden.built or self.hidden.inputDim != D:
            self.hidden.build((None, None, D))
        if not self.logits.built:
            self.logits.build((None, None, self.attentionUnits))
        self.built = True

    def compute_output_shape(self, input_shape):
        D = input_shape[self.featAxis]
        return (input_shape[self.batchAxis], 1, 2 * D if self.includeStd else D)

    def get_config(self):
        c = super().get_config()
        c.update({"attention_units": self.attentionUnits, "heads": self.heads, "include_std": self.includeStd, "epsilon": self.epsilon,
                  "attention_activation": self.attentionActivation})
        return c

    def get_weights(self):
        if not (self.hidden.built and self.logits.built):
            return []
        return [self.hidden.kernel[0, 0], self.hidden.bias, self.logits.kernel[0, 0], self.logits.bias]

    def set_weights(self, weights, fmt="tensorflow"):
        """[W1, b1, W2, b2]; fmt "tensorflow": W1 (D, A), W2 (A, H) as get_weights() gives them, "kaldi": (A, D) and (H, A)."""
        fmt = fmt.lower()
        if fmt not in ["kaldi", "tensorflow"]:
            raise ValueError(f"expected 'fmt' to be either 'kaldi' or 'tensorflow', got {fmt}")
        if len(weights) != 4:
            raise ValueError(f"expected a weight list of length 4, got {len(weights)}")
        w1, b1, w2, b2 = (np.asarray(w, np.float32) for w in weights)
        if fmt == "kaldi":
            w1, w2 = w1.T, w2.T
        A, H = self.attentionUnits, self.heads
        D = self.inputDim if self.built else (w1.shape[0] if w1.ndim == 2 else -1)
        for name, w, shape in (("W1", w1, (D, A)), ("b1", b1.reshape(-1), (A,)), ("W2", w2, (A, H)), ("b2", b2.reshape(-1), (H,))):
            if w.shape != shape:
                raise ValueError(f"{name}: expected shape {shape}, got {w.shape}")
        if D % H:
            raise ValueError(f"'heads' = {H} does not divide the {D} input channels")
        self.hidden.set_weights([w1[None, None], b1], fmt="tensorflow")
        self.logits.set_weights([w2[None, None], b2], fmt="tensorflow")
        self.inputDim = D
        self.built = True

    @staticmethod
    def attention_gemm(gemm):
        """The arithmetic of the two attention affines in a call of mode `gemm`: their output goes through exp, so they never run in
        one-pass bf16 or f16mx -- fp32 for an fp32 call, split-bf16 for every other."""
        return L.GEMM_F32 if gemm == L.GEMM_F32 else L.GEMM_BF16X3

    def attend(self, x, lens=None, gemm=L.GEMM_F32, scratch=None):
        """x (B, T, D) fp32 rows the GEMM can read (TDNN.forward) -> the logits e (B, T, H), a view of a buffer whose pad columns are
        finite. `scratch(role, shape, dtype)`: where the two outputs go (default: fresh zeroed tensors)."""
        B, T, _ = x.shape
        A, H = self.attentionUnits, self.heads
        lda, lde = ops.round_up(A, 32), ops.round_up(H, 8)
        new = scratch or (lambda role, shape, dtype: torch.zeros(shape, dtype=dtype, device=x.device))
        g = self.attention_gemm(gemm)
        h = self.hidden.forward(x, lens=lens, gemm=g, ldy=lda, out=new("attn_hidden", (B, T, lda), torch.float32))
        e = self.logits.forward(h[:, :, :A], lens=lens, gemm=g, ldy=lde, out=new("attn_logits", (B, T, lde), torch.float32))
        return e[:, :, :H]

    def pool(self, x, lens=None, gemm=L.GEMM_F32, out=None, scratch=None):
        """x as in attend() -> (B, D or 2 D) fp32 in `out` (B, ld_out) if given. No host synchronisation."""
        B, T, D = x.shape
        if D != self.inputDim:
            raise ValueError(f"expected input feature dim {self.inputDim}, got {D}")
        od = 2 * D if self.includeStd else D
        if out is None:
            out = torch.empty((B, od), dtype=torch.float32, device=x.device)
        e = self.attend(x, lens, gemm, scratch)
        new = scratch or (lambda role, shape, dtype: torch.empty(shape, dtype=dtype, device=x.device))
        norm = new("attn_norm", (B, self.heads, 2), torch.float64)
        ops.attn_pool(x, e, lens, self.includeStd, self.epsilon, out, norm, None, D=D, H=self.heads)
        return out

    def call(self, inputs):
        x = inputs
        if x.dim() != 3:
            raise ValueError(f"expected a (batch, time, feat) input, got shape {tuple(x.shape)}")
        B, T, D = x.shape
        gemm = _GEMM[self.gemm]
        rows = self.hidden.prepare_input(x.to(torch.float32), self.attention_gemm(gemm))
        return self.pool(rows[:, :, :D], None, gemm).reshape(B, 1, -1)


# =============================================================================== plda
class PLDA(Layer):
    """layers/plda/plda.py:24 — PLDA transform + pairwise log-likelihood-ratio scoring."""

    def __init__(self, dim, plda_mean, plda_transform, plda_psi, normalize_length=True, simple_length_norm=False,
                 dtype=torch.float64, return_transformed=True, name=None):
        super().__init__(trainable=False, name=name)
        self.dim = dim
        self.normalizeLength = normalize_length
        self.simpleLengthNorm = simple_length_norm
        self.paramDtype = self._torch_dtype(dtype)
        self.returnTransformed = return_transformed
        self.inputRank = 3
        npdt = np.float64 if self.paramDtype == torch.float64 else np.float32
        self.mean = np.asarray(plda_mean, dtype=npdt)
        self.transformMat = np.asarray(plda_transform, dtype=npdt)
        self.psi = np.asarray(plda_psi, dtype=npdt)
        self.assertParamShapes()
        self.offset = (-1.0 * (self.transformMat @ self.mean.reshape(self.dim, 1))).reshape(-1).astype(npdt)
        self._dev = None
        self._dense_dev = self._dense_ws = None
        self.last_dense_dims = None               # score_dense: retained PCA dimension per recording (device int32)

    @staticmethod
    def _torch_dtype(dt):
        if dt in (torch.float64, np.float64, "float64", float):
            return torch.float64
        if dt in (torch.float32, np.float32, "float32"):
            return torch.float32
        name = getattr(dt, "name", None)
        if name in ("float64", "float32"):
            return torch.float64 if name == "float64" else torch.float32
        raise ValueError(f"unsupported PLDA dtype {dt}")

    def build(self, input_shape):
        vecDim = input_shape[-1]
        if vecDim != self.dim:
            raise ValueError(f"expected input vector dimension to be {self.dim}, got {vecDim}")
        self.inputRank = len(input_shape)
        if self.inputRank not in [2, 3]:
            raise ValueError(f"expected input tensor rank to be 2 or 3, got {len(input_shape)}")
        self.built = True

    def assertParamShapes(self):
        assert self.mean.ndim == 1, f"plda_mean must be a vector, got dimension={self.mean.ndim}"
        assert self.psi.ndim == 1, f"plda_psi must be a vector, got dimension={self.psi.ndim}"
        assert self.transformMat.ndim == 2, f"plda_transform_mat must be a matrix, got dimension={self.transformMat.ndim}"
        assert self.mean.shape[0] == self.dim, f"plda_mean dimension size ({self.mean.shape[0]}) != input dim ({self.dim})"
        assert self.psi.shape[0] == self.dim, f"plda_psi dimension size ({self.psi.shape[0]}) != input dim ({self.dim})"
        r, c = self.transformMat.shape
        assert r == self.dim, f"plda_transform_mat dimension size ({r}) != input dim ({self.dim})"
        assert r == c, f"plda_transform_mat ({r} x {c}) is not a square matrix"

    def _prepare(self, inputs):
        x = inputs
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(np.ascontiguousarray(x), device=ops.default_device())
        if x.dim() == 3:
            if x.shape[1] != 1:
                raise ValueError(f"expected (batch, 1, dim) input, got {tuple(x.shape)}")
            x = x.reshape(x.shape[0], x.shape[2])
        elif x.dim() != 2:
            raise ValueError(f"expected input tensor rank to be 2 or 3, got {x.dim()}")
        x = x.to(self.paramDtype).contiguous()
        if self._dev is None or self._dev[0].device != x.device:
            f = lambda a: torch.as_tensor(np.ascontiguousarray(a).copy(), device=x.device)  # noqa: E731
            self._dev = (f(self.transformMat), f(self.offset), f(self.psi))
        return x

    def transform(self, inputs, num_examples=None):
        """Extension: transformVector alone (plda.py:163-196) -> (B, dim) transformed vectors. num_examples: the number of
        examples each vector averages (Kaldi's TransformIvector(num_examples); the speaker model of verification.speaker_means):
        None (1, the plain path), a scalar, a host array of B or a device tensor of B. Counts must be > 0: checked directly on the
        host, or on the device with one reduction and one read. With every count 1 the result is the plain path's, bit for bit."""
        x = self._prepare(inputs)
        A, off, psi = self._dev
        if num_examples is None:
            return ops.plda(x, A, off, psi, self.normalizeLength, self.simpleLengthNorm, want_scores=False)[1]
        n = self._counts(num_examples, x.shape[0], x.device, "num_examples")
        return ops.plda_transform_n(x, A, off, psi, n, self.normalizeLength, self.simpleLengthNorm)

    def _counts(self, n, rows, device, what):
        """num_examples as a (rows,) device tensor of the layer's dtype, every value checked > 0 (NaN refused)."""
        if isinstance(n, torch.Tensor) and n.is_cuda:
            if n.device != device:
                raise ValueError(f"{what} is on {n.device}, the vectors on {device}")
            if n.dim() == 0:
                n = n.reshape(1).expand(rows)
            if n.dim() != 1 or n.shape[0] != rows:
                raise ValueError(f"{what} must be a scalar or hold {rows} counts, got shape {tuple(n.shape)}")
            c = n.to(self.paramDtype).contiguous()
            if rows and bool((~(c > 0)).any().item()):                      # the one device -> host read
                raise ValueError(f"{what} must all be > 0")
            return c
        a = np.asarray(n.numpy() if isinstance(n, torch.Tensor) else n, dtype=np.float64)
        if a.ndim == 0:
            a = np.full((rows,), float(a))
        if a.ndim != 1 or a.shape[0] != rows:
            raise ValueError(f"{what} must be a scalar or hold {rows} counts, got shape {a.shape}")
        if not np.all(a > 0):
            raise ValueError(f"{what} must all be > 0, got {a[~(a > 0)][:4].tolist()}")
        return torch.as_tensor(a, dtype=self.paramDtype).to(device)

    def _scoring_inputs(self, test_transformed, enroll_transformed):
        t = test_transformed.reshape(test_transformed.shape[0], -1).to(self.paramDtype).contiguous()
        e = enroll_transformed.reshape(enroll_transformed.shape[0], -1).to(self.paramDtype).contiguous()
        if e.device != t.device:
            raise ValueError(f"test vectors on {t.device}, enrollment vectors on {e.device}")
        if self._dev is None or self._dev[0].device != t.device:
            self._prepare(t)
        return t, e

    def score(self, test_transformed, enroll_transformed, enroll_num_examples=None):
        """Extension: rectangular trial block, scores[i, j] = LLR(test_i | class of enroll_j) on TRANSFORMED vectors
        (the reference scores a batch against itself only); row blocks of a large trial matrix shard across GPUs
        (parallel.plda_trials). enroll_num_examples: examples per class j (Kaldi's LogLikelihoodRatio(n), ivector-plda-scoring
        --num-utts), checked as transform's num_examples; None keeps the count-free path (every count 1 gives its bits)."""
        t, e = self._scoring_inputs(test_transformed, enroll_transformed)
        if enroll_num_examples is None:
            return ops.plda_score(t, e, self._dev[2])
        n = self._counts(enroll_num_examples, e.shape[0], t.device, "enroll_num_examples")
        return ops.plda_score_n(t, e, self._dev[2], n)

    def score_trials(self, test_transformed, enroll_transformed, trials_enroll, trials_test, enroll_num_examples=None):
        """Extension: ivector-plda-scoring over a trial list. scores[t] = LLR(test_{trials_test[t]} | class enroll_{trials_enroll[t]})
        with the class's count (enroll_num_examples, as in score; None: 1 each) -> (T,) in the layer's dtype. Only the listed pairs
        are scored: a trial's bits depend on its two vectors and the count, not on the list's order. The indices are host arrays
        (checked there) or device integer tensors (checked with one reduction and one read); either way every index must lie in
        range (a pair outside the arrays that reached the kernel would score NaN, nothing outside them is read)."""
        t, e = self._scoring_inputs(test_transformed, enroll_transformed)
        N, M = t.shape[0], e.shape[0]
        pairs = self._trial_pairs(trials_enroll, trials_test, M, N, t.device)
        n = self._counts(1.0 if enroll_num_examples is None else enroll_num_examples, M, t.device, "enroll_num_examples")
        return ops.plda_trials(t, e, self._dev[2], n, pairs)

    def cohort_stats(self, vectors_tr, cohort_tr, top_n=None, role="test", num_examples=None, workspace_limit=1 << 30):
        """Extension: the statistics of score normalisation against a cohort (S-norm; adaptive S-norm with top_n, Matejka et al.
        2017) on TRANSFORMED vectors -> (mean, std), each (R,) float64 on the device: the mean and the centred population standard
        deviation of the top_n largest of row r's C cohort scores (None or >= C: all of them, plain S-norm; ties at the threshold
        fill the selection up to top_n, so it does not depend on how ties are broken).
        role "test" (T-norm side): row r is a test vector scored against every cohort vector as a class; num_examples are the
        cohort's counts (transform the cohort with them): row r is score(vectors_tr, cohort_tr, num_examples)[r].
        role "enroll" (Z-norm side): row r is a class with count num_examples[r], every cohort vector (transformed without counts)
        is scored against it as a test: row r is score(cohort_tr, vectors_tr, num_examples)[:, r].
        Every ranked score has score's bits for its pair. num_examples is checked as transform's. The (R, C) scores are never held
        at once: rows go through one workspace of at most workspace_limit bytes, chunk * C * itemsize <= workspace_limit with at
        least one row per chunk (above 64 rows a multiple of 64, the score tile); the result does not depend on the chunking."""
        if role not in ("test", "enroll"):
            raise ValueError(f"role must be 'test' or 'enroll', got {role!r}")
        if top_n is not None:
            if not is_int(top_n) or int(top_n) < 2:
                raise ValueError(f"top_n must be None or an integer >= 2, got {top_n!r}")
        if not is_int(workspace_limit) or int(workspace_limit) < 1:
            raise ValueError(f"workspace_limit must be a positive number of bytes, got {workspace_limit!r}")
        for t, what in ((vectors_tr, "vectors_tr"), (cohort_tr, "cohort_tr")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError(f"{what} must be a device tensor of transformed vectors")
            if t.dim() != 2 or t.shape[1] != self.dim:
                raise ValueError(f"{what} must be (rows, {self.dim}), got {tuple(t.shape)}")
        if cohort_tr.device != vectors_tr.device:
            raise ValueError(f"vectors on {vectors_tr.device}, the cohort on {cohort_tr.device}")
        if cohort_tr.shape[0] < 1:
            raise ValueError("the cohort is empty")
        v, c = vectors_tr.to(self.paramDtype).contiguous(), cohort_tr.to(self.paramDtype).contiguous()
        if self._dev is None or self._dev[0].device != v.device:
            self._prepare(c)
        R, Cn = v.shape[0], c.shape[0]
        n = None
        if num_examples is not None:
            n = self._counts(num_examples, Cn if role == "test" else R, v.device, "num_examples")
        mean = torch.empty((R,), dtype=torch.float64, device=v.device)
        std = torch.empty((R,), dtype=torch.float64, device=v.device)
        if R == 0:
            return mean, std
        chunk = min(max(1, int(workspace_limit) // (Cn * v.element_size())), 64 * 65535)
        if chunk < R and chunk > 64:
            chunk -= chunk % 64                                             # whole 64-row score tiles (a ragged tile only at the end)
        chunk = min(chunk, R)
        ws = torch.empty((ops.plda_cohort_workspace_bytes(chunk, Cn, self.dim, v.element_size()),), dtype=torch.uint8, device=v.device)
        with L.launch_scope(v.device):
            for r0, r1 in chunks(R, chunk):
                ops.plda_cohort_stats(v[r0:r1], c, self._dev[2], n if n is None or role == "test" else n[r0:r1],
                                      1 if role == "enroll" else 0, top_n, mean[r0:r1], std[r0:r1], ws)
        return mean, std

    @staticmethod
    def _trial_pairs(trials_enroll, trials_test, M, N, device):
        """(T, 2) device int32 rows (class j, test i), every index checked in range."""
        dev_in = [isinstance(a, torch.Tensor) and a.is_cuda for a in (trials_enroll, trials_test)]
        if all(dev_in):
            je, it = trials_enroll, trials_test
            for a in (je, it):
                if a.device != device:
                    raise ValueError(f"trial indices on {a.device}, the vectors on {device}")
                if a.dim() != 1 or a.dtype.is_floating_point or a.dtype == torch.bool or a.is_complex():
                    raise ValueError(f"trial indices must be 1-D integer tensors, got {a.dtype} {tuple(a.shape)}")
            if je.shape[0] != it.shape[0]:
                raise ValueError(f"{je.shape[0]} enrollment indices, {it.shape[0]} test indices")
            if je.shape[0] and bool(((je < 0) | (je >= M) | (it < 0) | (it >= N)).any().item()):     # the one device -> host read
                raise ValueError(f"a trial index is out of range (classes 0..{M - 1}, tests 0..{N - 1})")
            return torch.stack((je.to(torch.int32), it.to(torch.int32)), dim=1).contiguous()
        if any(dev_in):
            raise ValueError("trials_enroll and trials_test must both be on the host or both on the device")
        arrs = []
        for a, hi, what in ((trials_enroll, M, "trials_enroll"), (trials_test, N, "trials_test")):
            a = np.asarray(a.numpy() if isinstance(a, torch.Tensor) else a)
            if a.size == 0:
                a = a.reshape(0).astype(np.int64)
            if a.ndim != 1 or a.dtype.kind not in "iu":
                raise ValueError(f"{what} must be a 1-D sequence of integers, got {a.dtype} {a.shape}")
            if a.size and (a.min() < 0 or a.max() >= hi):
                raise ValueError(f"{what} has an index outside 0..{hi - 1}")
            arrs.append(a.astype(np.int32))
        if arrs[0].shape != arrs[1].shape:
            raise ValueError(f"{arrs[0].size} enrollment indices, {arrs[1].size} test indices")
        return torch.as_tensor(np.ascontiguousarray(np.stack(arrs, axis=1).reshape(-1, 2))).to(device)

    def score_dense(self, inputs, lengths=None, target_energy=0.1):
        """Extension: Kaldi's `ivector-plda-scoring-dense`, the scoring stage of diarization. `inputs` (S, dim) or (S, 1, dim), the
        vectors `call` takes, are the rows of R recordings laid end to end, `lengths[r]` rows each (None: one recording). Each
        recording gets its own PCA (retaining `target_energy` of its variance as Kaldi's EstPca counts it, clamped to the
        numerical rank), the model is projected into that subspace, and every pair of its rows is scored.
        target_energy None: no PCA, every block is `call`'s scores of that recording's rows, bit for bit.
        -> a list of R (n_r, n_r) tensors in the layer's dtype, views of one allocation; a single (S, S) tensor when lengths is None.
        `last_dense_dims` then holds the retained dimension per recording (device int32; 0 = scored without PCA)."""
        shape = tuple(inputs.shape)
        if len(shape) not in (2, 3) or (len(shape) == 3 and shape[1] != 1):
            raise ValueError(f"expected (rows, dim) or (rows, 1, dim) input, got {shape}")
        if shape[-1] != self.dim:
            raise ValueError(f"expected input vector dimension to be {self.dim}, got {shape[-1]}")
        if self.dim > L.PLDA_DENSE_MAX_DIM:
            raise ValueError(f"dense scoring needs dim <= {L.PLDA_DENSE_MAX_DIM}, got {self.dim} (PLDA.call serves any dim)")
        if target_energy is not None:
            if isinstance(target_energy, bool) or not isinstance(target_energy, (int, float, np.floating, np.integer)):
                raise ValueError(f"target_energy must be a number in [0, 1) or None, got {target_energy!r}")
            if not 0.0 <= float(target_energy) < 1.0:
                raise ValueError(f"target_energy must be in [0, 1) (None: no PCA), got {target_energy}")
        S = shape[0]
        single = lengths is None
        if single:
            lens = [S]
        else:
            arr = np.asarray(lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)
            if arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iu"):
                raise ValueError(f"lengths must be a 1-D sequence of integers, got {lengths!r}")
            lens = [int(n) for n in arr]
        if not lens or min(lens) < 1:
            raise ValueError(f"every recording needs at least one row, got lengths {lens}")
        if sum(lens) != S:
            raise ValueError(f"lengths add up to {sum(lens)} rows, the input has {S}")
        x = self._prepare(inputs)
        A, off, psi = self._dev
        if getattr(self, "_dense_dev", None) is None or self._dense_dev[0].device != x.device:
            T = np.asarray(self.transformMat, np.float64)
            f = lambda a: torch.as_tensor(np.array(a, np.float64), device=x.device)  # noqa: E731
            self._dense_dev = (f(self.mean), f(np.linalg.inv(T)), f(self.psi))
        if getattr(self, "_dense_ws", None) is None:
            from .models import _Workspace
            self._dense_ws = _Workspace()
        ws = self._dense_ws
        scores, dims, status = ops.plda_dense(x, lens, target_energy, A, off, psi, *self._dense_dev, self.normalizeLength,
                                              self.simpleLengthNorm,
                                              scratch=lambda role, shp, dt: ws.get(role, shp, dt, x.device, padded=False))
        self.last_dense_dims = dims
        bad = int(status.item())                   # the call's one device -> host read
        if bad:
            raise L.KtfBackendError(f"PLDA.score_dense: {bad} per-recording eigenproblem(s) did not converge within "
                                    f"{L.PLDA_DENSE_MAX_SWEEPS} Jacobi sweeps or gave a singular subspace model")
        if single:
            return scores.view(S, S)
        out, o = [], 0
        for n in lens:
            out.append(scores[o:o + n * n].view(n, n))
            o += n * n
        return out

    def call(self, inputs):
        x = self._prepare(inputs)
        A, off, psi = self._dev
        scores, tr = ops.plda(x, A, off, psi, self.normalizeLength, self.simpleLengthNorm)
        if self.returnTransformed:
            return scores, tr.reshape(tr.shape[0], tr.shape[1], 1)
        return scores


# =============================================================================== i-vectors
def select_frames(feats, D, lengths, mask):
    """(B, T, D) device fp32 -> (frames (F, D) in utterance order, offsets (B + 1) host int64): the first lengths[b] frames of
    utterance b, or the frames with a nonzero mask (B, T) / (B, T, 1), or every frame."""
    if not isinstance(feats, torch.Tensor) or not feats.is_cuda:
        raise ValueError("feats must be a (B, T, D) tensor on a GPU")
    if feats.dim() != 3 or feats.shape[2] != D:
        raise ValueError(f"feats must be (B, T, {D}), got {tuple(feats.shape)}")
    if feats.dtype != torch.float32:
        raise ValueError(f"feats must be float32, got {feats.dtype}")
    B, T, D = feats.shape
    if lengths is not None and mask is not None:
        raise ValueError("pass lengths or mask, not both")
    if mask is not None:
        m = mask.reshape(mask.shape[0], -1) if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask))
        if m.dim() != 2 or tuple(m.shape) != (B, T):
            raise ValueError(f"mask must be (B, T) or (B, T, 1) = ({B}, {T}), got {tuple(mask.shape)}")
        m = m.to(feats.device) != 0
    elif lengths is not None:
        n = host(lengths, np.int64).reshape(-1)
        if n.shape[0] != B or (n < 0).any() or (n > T).any():
            raise ValueError(f"lengths must hold {B} values in 0 .. {T}")
        m = torch.arange(T, device=feats.device)[None, :] < torch.as_tensor(n, device=feats.device)[:, None]
    else:
        return feats.reshape(B * T, D) if feats.is_contiguous() else feats.contiguous().reshape(B * T, D), np.arange(B + 1) * T
    counts = m.sum(1).cpu().numpy().astype(np.int64)
    return feats[m].contiguous(), np.concatenate([[0], np.cumsum(counts)])


class IvectorExtractor(Layer):
    """Extension (the reference reads `final.ie` and extracts nothing): Kaldi's sid/extract_ivectors.sh core on the GPU,

        gmm-global-get-post --n=num_gselect --min-post=min_post final.dubm feats ark:- | scale-post ark:- posterior_scale ark:- |
        ivector-extract --acoustic-weight=acoustic_weight --max-count=max_count final.ie feats ark:- ivectors.ark

    or, with `full_ubm`, the posterior stage of the recipes themselves (every sid/extract_ivectors.sh):

        gmm-gselect --n=num_gselect final.dubm feats ark:- |
        fgmm-global-gselect-to-post --min-post=min_post final.ubm feats ark:- ark:- | scale-post ... | ivector-extract ...

    `extractor`: a path to a Kaldi binary `final.ie` or an io.KaldiIvecExtractorReader; `diag_ubm`: a path to `final.dubm` or an
    io.KaldiDiagGmmReader; `full_ubm`: a path to `final.ubm` or an io.KaldiFullGmmReader. With a full UBM the diagonal one only
    preselects num_gselect Gaussians per frame and the posteriors come from the full one; `diag_ubm=None` then stands for
    `full_ubm.toDiag()` (fgmm-global-to-gmm). The defaults are those of the recipe's extract_ivectors.sh (num_gselect 20, min_post
    0.025); gmm-global-get-post's own defaults are --n=50 --min-post=0.0. An extractor with ivector-dependent weights (a non-empty
    `w`) raises NotImplementedError. Calls run on the device of `feats` and its current stream; the utterances, and with a full UBM
    the frames, are processed in chunks whose workspace stays under `workspace_limit` bytes, and no output bit depends on the chunks."""

    def __init__(self, extractor, diag_ubm=None, num_gselect=20, min_post=0.025, posterior_scale=1.0, acoustic_weight=1.0, max_count=0.0,
                 workspace_limit=1 << 30, name=None, full_ubm=None):
        super().__init__(trainable=False, name=name)
        from . import io as kio
        ie = extractor if isinstance(extractor, kio.KaldiIvecExtractorReader) else kio.KaldiIvecExtractorReader(extractor, binary=True)
        if diag_ubm is None and full_ubm is None:
            raise ValueError("IvectorExtractor needs diag_ubm, full_ubm or both")
        full = None
        if full_ubm is not None:
            full = full_ubm if isinstance(full_ubm, kio.KaldiFullGmmReader) else kio.KaldiFullGmmReader(full_ubm, binary=True)
            if full.numGauss != ie.numGauss or full.featDim != ie.featDim:
                raise ValueError(f"full UBM ({full.numGauss} Gaussians, dim {full.featDim}) does not match the extractor "
                                 f"({ie.numGauss} Gaussians, dim {ie.featDim})")
        if diag_ubm is None:
            ubm = full.toDiag()
        else:
            ubm = diag_ubm if isinstance(diag_ubm, kio.KaldiDiagGmmReader) else kio.KaldiDiagGmmReader(diag_ubm, binary=True)
        if ie.w is not None and ie.w.size:
            raise NotImplementedError("ivector-dependent weights (a non-empty <w>) are not supported")
        if ubm.numGauss != ie.numGauss or ubm.featDim != ie.featDim:
            raise ValueError(f"UBM ({ubm.numGauss} Gaussians, dim {ubm.featDim}) does not match the extractor "
                             f"({ie.numGauss} Gaussians, dim {ie.featDim})")
        I, D, S = ie.numGauss, ie.featDim, ie.ivecDim
        if not (1 <= I <= L.IVECTOR_MAX_GAUSS and 1 <= D <= L.IVECTOR_MAX_FEAT_DIM and 1 <= S <= L.IVECTOR_MAX_DIM):
            raise ValueError(f"extractor shape (I={I}, D={D}, S={S}) outside I <= {L.IVECTOR_MAX_GAUSS}, D <= "
                             f"{L.IVECTOR_MAX_FEAT_DIM}, S <= {L.IVECTOR_MAX_DIM}")
        if not 1 <= int(num_gselect) <= L.IVECTOR_MAX_GSELECT:
            raise ValueError(f"num_gselect {num_gselect} outside 1 .. {L.IVECTOR_MAX_GSELECT}")
        if not 0.0 <= float(min_post) < 1.0:
            raise ValueError(f"min_post {min_post} outside [0, 1)")
        if min(float(posterior_scale), float(acoustic_weight), float(max_count)) < 0:
            raise ValueError("posterior_scale, acoustic_weight and max_count must be >= 0")
        self.numGauss, self.featDim, self.ivecDim = I, D, S
        self.numGselect, self.minPost = int(num_gselect), float(min_post)
        self.posteriorScale, self.acousticWeight, self.maxCount = float(posterior_scale), float(acoustic_weight), float(max_count)
        self.priorOffset = float(ie.priorOffset)
        self.workspaceLimit = int(workspace_limit)
        # host copies of the device constants: W = [means_invvars; -inv_vars / 2] (2D, I), gconst (I), sigmaInvM (I*D, S), U (I, P)
        self._W = np.ascontiguousarray(np.concatenate([ubm.means_invvars.astype(np.float32).T,
                                                       (np.float32(-0.5) * ubm.inv_vars.astype(np.float32)).T]))
        self._gconst = np.ascontiguousarray(ubm.gconsts, dtype=np.float32)
        self._sigmaInvM = np.ascontiguousarray(np.asarray(ie.sigmaInvM, dtype=np.float64).reshape(I * D, S))
        self._U = np.ascontiguousarray(ie.U, dtype=np.float64)
        # the full UBM as ktf_fgmm_post_f32 takes it: means_invcovars (I, D), inv_covars (I, D, D) full, gconst (I)
        self._full = None if full is None else tuple(np.ascontiguousarray(a, dtype=np.float32)
                                                     for a in (full.means_invcovars, full.inv_covars, full.gconsts))
        # the most frames whose ktf_fgmm_post_f32 workspace stays under workspace_limit (at least one)
        self._frameStep = None if full is None else self._frame_step()

    def get_config(self):
        raise NotImplementedError("IvectorExtractor holds model files, not a config")

    def _consts(self, device):
        def make():
            f = lambda a: torch.as_tensor(a, device=device)  # noqa: E731
            full = None if self._full is None else tuple(f(a) for a in self._full)
            return f(self._W), f(self._gconst), f(self._sigmaInvM), f(self._U), full
        return per_device(self, device, make)

    def _frame_step(self):
        I, D, n = self.numGauss, self.featDim, self.numGselect
        return max_under(lambda f: ops.fgmm_workspace_bytes(f, I, D, n), self.workspaceLimit, ((1 << 31) - 1) // n)

    def _post(self, x):
        """Posteriors of the frames x (F, D): gmm-global-get-post, or with a full UBM gmm-gselect | fgmm-global-gselect-to-post."""
        W, gc, _, _, full = self._consts(x.device)
        if full is None:
            return ops.ivector_post(x, W, gc, self.numGselect, self.minPost)
        mic, icov, fgc = full
        F, step = x.shape[0], self._frameStep
        if F <= step:
            sel, _ = ops.ivector_post(x, W, gc, self.numGselect, 0.0)
            return ops.fgmm_post(x, sel, mic, icov, fgc, self.minPost)
        g = torch.empty((F, self.numGselect), dtype=torch.int32, device=x.device)
        p = torch.empty((F, self.numGselect), dtype=torch.float32, device=x.device)
        for lo, hi in chunks(F, step):
            sel, _ = ops.ivector_post(x[lo:hi], W, gc, self.numGselect, 0.0)
            g[lo:hi], p[lo:hi] = ops.fgmm_post(x[lo:hi], sel, mic, icov, fgc, self.minPost)
        return g, p

    def _frames(self, feats, lengths, mask):
        """(B, T, D) device fp32 -> (frames (F, D) in utterance order, offsets (B + 1) host int64)."""
        return select_frames(feats, self.featDim, lengths, mask)

    def _chunks(self, B):
        per = ops.ivector_workspace_bytes(1, self.numGauss, self.featDim, self.ivecDim)
        return chunks(B, int(max(1, min(B, 65535, self.workspaceLimit // max(per, 1)))))

    def posteriors(self, feats, lengths=None, mask=None):
        """The posterior stage alone (gmm-global-get-post, or the full-UBM pair) -> (gauss (F, num_gselect) int32, post (F, num_gselect) fp32, offsets (B + 1) int64): the selected
        frames of all utterances end to end, utterance b's rows [offsets[b], offsets[b + 1]); unused slots (-1, 0)."""
        x, off = self._frames(feats, lengths, mask)
        with L.on_device(x.device):
            g, p = self._post(x)
        return g, p, torch.as_tensor(off, device=x.device)

    def from_posteriors(self, feats, gauss, post, lengths=None, mask=None, dtype=torch.float32):
        """scale-post | ivector-extract on posteriors the caller supplies: gauss / post (F, n) rows aligned with the selected frames
        of feats (as `posteriors` returns them; an index outside [0, I) is skipped) -> (B, S) i-vectors of dtype."""
        x, off = self._frames(feats, lengths, mask)
        if gauss.shape != post.shape or gauss.dim() != 2 or gauss.shape[0] != x.shape[0]:
            raise ValueError(f"gauss / post must both be ({x.shape[0]}, n), got {tuple(gauss.shape)} / {tuple(post.shape)}")
        if not 1 <= gauss.shape[1] <= L.IVECTOR_MAX_GSELECT:
            raise ValueError(f"{gauss.shape[1]} slots per frame outside 1 .. {L.IVECTOR_MAX_GSELECT}")
        g = gauss.to(device=x.device, dtype=torch.int32).contiguous()
        p = post.to(device=x.device, dtype=torch.float32).contiguous()
        return self._extract(x, off, lambda lo, hi: (g[lo:hi], p[lo:hi]), dtype)

    def _extract(self, x, off, posts, dtype):
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype}")
        B = len(off) - 1
        _, _, sim, U, _ = self._consts(x.device)
        out = torch.empty((B, self.ivecDim), dtype=dtype, device=x.device)
        with L.on_device(x.device):
            for b0, b1 in self._chunks(B):
                lo, hi = int(off[b0]), int(off[b1])
                g, p = posts(lo, hi)
                o = torch.as_tensor((off[b0:b1 + 1] - lo).astype(np.int32), device=x.device)
                out[b0:b1] = ops.ivector_extract(x[lo:hi], o, g, p, self.posteriorScale, self.acousticWeight, self.maxCount, sim, U,
                                                 self.priorOffset, dtype)
        return out

    def _train_chunks(self, B):
        per = ops.ivector_train_workspace_bytes(1, self.numGauss, self.featDim, self.ivecDim)
        return chunks(B, int(max(1, min(B, 65535, self.workspaceLimit // max(per, 1)))))

    def _accumulate(self, stats, x, off, posts):
        if self.acousticWeight != 1.0 or self.maxCount != 0.0:
            raise ValueError("ivector-extractor-acc-stats has no acoustic_weight and no max_count: the layer must keep their defaults")
        if tuple(stats.shape) != (self.numGauss, self.featDim, self.ivecDim):
            raise ValueError(f"statistics of shape {tuple(stats.shape)} do not match the extractor "
                             f"{(self.numGauss, self.featDim, self.ivecDim)}")
        stats._alloc(x.device)
        B = len(off) - 1
        _, _, sim, U, _ = self._consts(x.device)
        chunks = self._train_chunks(B)
        with L.on_device(x.device):
            for b0, b1 in chunks:
                lo, hi = int(off[b0]), int(off[b1])
                g, p = posts(lo, hi)
                o = torch.as_tensor((off[b0:b1 + 1] - lo).astype(np.int32), device=x.device)
                ops.ivector_acc_stats(x[lo:hi], o, g, p, self.posteriorScale, sim, U, self.priorOffset, stats.gamma, stats.Y, stats.R,
                                      stats.ivector_sum, stats.ivector_scatter, stats.totals)
                if stats.updateVariances:
                    ops.ivector_acc_second_order(x[lo:hi], g, p, self.posteriorScale, stats.Ssec)
        return len(chunks)

    def accumulate(self, stats, feats, lengths=None, mask=None):
        """Extension: ivector-extractor-acc-stats on the batch `__call__` would extract from, posterior stage included (with or
        without full_ubm), added to `stats` (training.IvectorStats) in place. The utterances run in chunks whose workspace stays
        under workspace_limit; for the same sequence of calls and the same limit every accumulator is bit-identical run to run.
        ValueError if the layer's acoustic_weight != 1 or max_count != 0, or if stats was made for another extractor shape.
        -> the number of chunks."""
        x, off = self._frames(feats, lengths, mask)
        return self._accumulate(stats, x, off, lambda lo, hi: self._post(x[lo:hi]))

    def accumulate_from_posteriors(self, stats, feats, gauss, post, lengths=None, mask=None):
        """`accumulate` on posteriors the caller supplies, laid out as `from_posteriors` takes them."""
        x, off = self._frames(feats, lengths, mask)
        if gauss.shape != post.shape or gauss.dim() != 2 or gauss.shape[0] != x.shape[0]:
            raise ValueError(f"gauss / post must both be ({x.shape[0]}, n), got {tuple(gauss.shape)} / {tuple(post.shape)}")
        if not 1 <= gauss.shape[1] <= L.IVECTOR_MAX_GSELECT:
            raise ValueError(f"{gauss.shape[1]} slots per frame outside 1 .. {L.IVECTOR_MAX_GSELECT}")
        g = gauss.to(device=x.device, dtype=torch.int32).contiguous()
        p = post.to(device=x.device, dtype=torch.float32).contiguous()
        return self._accumulate(stats, x, off, lambda lo, hi: (g[lo:hi], p[lo:hi]))

    def __call__(self, feats, lengths=None, mask=None, dtype=torch.float32):
        """feats (B, T, D) fp32 on a GPU; lengths: the first lengths[b] frames of utterance b; mask: (B, T) or (B, T, 1), nonzero =
        voiced (select-voiced-frames, e.g. VAD(return_indexes=False)); neither: every frame. -> (B, S) i-vectors (fp32, Kaldi's
        Vector<BaseFloat>; dtype=torch.float64 keeps the solve's precision)."""
        x, off = self._frames(feats, lengths, mask)
        return self._extract(x, off, lambda lo, hi: self._post(x[lo:hi]), dtype)
