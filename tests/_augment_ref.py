"""The augmentation's rules (include/ktf_augment.h, steps 1 to 5) restated in fp64 NumPy with a direct np.convolve, and the
arithmetic a Kaldi-style CPU tool does for the same convolution restated in fp32 (block overlap-add with one FFT of the next power
of two >= 4 L per block, torch.fft on the CPU): the latter only measures what fp32 costs against the fp64 oracle, which sizes the
GPU tests' tolerance."""

import numpy as np
import torch


def early_window(h, fs):
    """(k, s0, s1): the lowest index of the signed maximum of h, and the early window about it."""
    k = int(np.argmax(np.asarray(h)))
    s0 = max(0, k - int(round(0.001 * fs)))
    s1 = min(len(h), k + int(round(0.05 * fs)))
    return k, s0, s1


def gain(snr_db, p_sig, p_nu):
    return float(np.sqrt(10.0 ** (-snr_db / 10.0) * p_sig / p_nu)) if p_nu > 0 else 0.0


def noise_piece(nu, d):
    """e[t] = nu[t mod m] for t < d' = d or m."""
    nu = np.asarray(nu, np.float64)
    d = int(d) or nu.size
    return nu[np.arange(d) % nu.size]


def augment_ref(x, h=None, additives=(), noises=(), fs=16000, shift_output=True, normalize_output=True, volume=0.0, int16=False):
    """One utterance. x: samples (fp32 values, or int16), h: the RIR or None, additives: [(noise id, snr_db, start o, duration d)] in
    samples -> dict(out, y (unshifted, unscaled), p_before, p_sig, p_after, scale, k, gains)."""
    x = np.asarray(x).astype(np.float32).astype(np.float64)
    n = x.size
    if n == 0:
        return dict(out=np.zeros(0, np.int16 if int16 else np.float64), y=np.zeros(0), p_before=0.0, p_sig=0.0, p_after=0.0,
                    scale=volume if volume > 0 else 1.0, k=0, gains=[0.0 for _ in additives])
    p_before = float(np.mean(x * x))
    if h is None:
        y, p_sig, k = x.copy(), p_before, 0
    else:
        h = np.asarray(h).astype(np.float32).astype(np.float64)
        k, s0, s1 = early_window(h, fs)
        e = np.convolve(x, h[s0:s1])
        p_sig = float(np.mean(e * e))
        y = np.convolve(x, h)
    gains = []
    for nid, snr_db, o, d in additives:
        e = noise_piece(np.asarray(noises[nid]).astype(np.float32), d)
        g = gain(np.float64(np.float32(snr_db)), p_sig, float(np.mean(e * e)))
        gains.append(g)
        m = min(e.size, y.size - o)
        if m > 0:
            y[o:o + m] += g * e[:m]
    p_after = float(np.mean(y * y))
    scale = float(volume) if volume > 0 else (float(np.sqrt(p_before / p_after)) if normalize_output and p_after > 0 else 1.0)
    out = (y * scale)[k:k + n] if shift_output else y * scale
    if int16:
        out = np.clip(np.rint(out), -32768, 32767).astype(np.int16)
    return dict(out=out, y=y, p_before=p_before, p_sig=p_sig, p_after=p_after, scale=scale, k=k, gains=gains)


def to_int16(v):
    """Round to nearest even and saturate, as the int16 output does, of fp32 values."""
    return np.clip(np.rint(np.asarray(v, np.float32)), -32768, 32767).astype(np.int16)


def blockwise_fft_convolve_f32(x, h):
    """x * h in fp32 the way a CPU tool with one FFT size does it: blocks of nfft - L + 1 samples, nfft the next power of two
    >= 4 L, each block's rfft times the filter's, irfft, overlap-add."""
    x = torch.as_tensor(np.asarray(x, np.float32))
    h = torch.as_tensor(np.asarray(h, np.float32))
    n, L = x.numel(), h.numel()
    nfft = 1
    while nfft < 4 * L:
        nfft *= 2
    block = nfft - L + 1
    H = torch.fft.rfft(h, n=nfft)
    y = torch.zeros(n + L - 1, dtype=torch.float32)
    for s in range(0, n, block):
        seg = x[s:s + block]
        piece = torch.fft.irfft(torch.fft.rfft(seg, n=nfft) * H, n=nfft)
        m = seg.numel() + L - 1
        y[s:s + m] += piece[:m]
    return y.numpy()


def rel_err(y, y64):
    """max |y - y64| / max |y64|."""
    y64 = np.asarray(y64, np.float64)
    return float(np.abs(np.asarray(y, np.float64) - y64).max() / np.abs(y64).max())


def decaying_rir(rng, L, peak):
    """An exponentially decaying random RIR of L taps whose signed maximum sits at `peak`."""
    h = rng.standard_normal(L) * np.exp(-6.0 * np.arange(L) / max(L, 1))
    h[peak] = np.abs(h).max() * 1.5 + 1.0
    return h.astype(np.float32)
