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


# ----------------------------------------------------------------------------- what csrc/augment.hip's launcher and kernels choose
# Internal constants of the kernels, mirrored here because the library does not export them (test_augment_paths_cpu.py checks
# the shapes of test_gpu_augment_paths.py against them: a changed constant moves the edge, and that module then fails).
AUG_J = 4                          # augment.hip:28, output blocks per workgroup of aug_conv_kernel
DIRECT_TAPS = 64                   # include/ktf_augment.h:37 (augment.hip:29), the longest filter applied in the time domain
AUG_THREADS = 256                  # augment_fft.h:14, threads per workgroup (aug_rir_peak_kernel: thread i % 256 reads tap i)
WAVE = 64


def blocks_of(samples, P):
    """augment.hip:37."""
    return (samples + P - 1) // P


def early_taps(fs):
    """augment.hip:38-39 -> (pre, post): the early window reaches pre taps before the peak and post taps from it on (nearbyint:
    to nearest, ties to even, as Python's round)."""
    return int(round(0.001 * fs)), int(round(0.05 * fs))


def early_partitions(fs, P):
    """augment.hip:40: the partitions the bank reserves per RIR for the spectra of h[s0:s1]."""
    return blocks_of(sum(early_taps(fs)), P)


def spectra_slots(lengths, fs, P):
    """augment.hip:120-121 -> [(full0, early0)] per RIR of a bank: its first partition among the full spectra and among the early
    ones, which lie behind all the full ones, npe = early_partitions(fs) per RIR."""
    off = np.concatenate([[0], np.cumsum(lengths)])
    R, npe = len(lengths), early_partitions(fs, P)
    return [(int(off[r]) // P + r, int(off[R]) // P + R + r * npe) for r in range(R)]


def conv_path(Lh):
    """augment.hip:237: "direct" (time domain) or "transform" for a filter of Lh taps."""
    return "direct" if Lh <= DIRECT_TAPS else "transform"


def conv_groups(n, Lh, P):
    """The workgroups of aug_conv_kernel that work on a row of n samples and a filter of Lh > DIRECT_TAPS taps (augment.hip:229-236,
    :269, :289-290) -> [dict(j0, np, pend, slides)]: the workgroup owns output blocks j0 .. j0 + AUG_J - 1, runs partitions
    0 .. pend - 1 and moves its register window of input spectra down `slides` = pend - 1 times."""
    ny, npart = blocks_of(n + Lh - 1, P), blocks_of(Lh, P)
    return [dict(j0=j0, np=npart, pend=min(npart, j0 + AUG_J), slides=min(npart, j0 + AUG_J) - 1) for j0 in range(0, ny, AUG_J)]


def early_grid(max_n, max_L, fs, P):
    """augment.hip:585-591 -> (ny, nye, the x-extent of aug_conv_kernel<true>'s grid = cdiv(min(ny, nye), AUG_J))."""
    ny, nye = blocks_of(max_n + max_L - 1, P), blocks_of(max_n + sum(early_taps(fs)) - 1, P)
    return ny, nye, -(-min(ny, nye) // AUG_J)


def peak_owner(i):
    """aug_rir_peak_kernel (augment.hip:103): -> (thread, wave) that reads tap i."""
    t = i % AUG_THREADS
    return t, t // WAVE


# The shapes of test_gpu_augment_paths.py, from P = ktf_aug_partition(). Pure data; the CPU module proves what each reaches.
def long_shapes(P):
    """-> (signal lengths, RIR lengths): RIRs of 5, 5, 10 and 13 partitions, more than the AUG_J blocks a workgroup owns."""
    return (1, P + 1, 2 * P + 17, 6 * P + 3), (4 * P + 1, 5 * P, 9 * P + 3, 13 * P - 1)


EARLY_RATES = (48000, 44100)       # pre + post = 2448 and 2249 taps: three early partitions (16000 and 8000 have one)


def wide_early_bank(P):
    """[(L, peak)] of one bank for EARLY_RATES, in the bank's order. At 48000: a clipped window of 148 taps (one partition); 2448
    taps (three partitions), twice, behind it; a peak on the last tap (49 taps: the early filter in the time domain, the full one
    transformed); a RIR of exactly DIRECT_TAPS taps (all of it in the time domain)."""
    return [(1500, 1400), (3 * P + 5, 100), (5000, 2500), (P + 200, P + 199), (DIRECT_TAPS, 20)]


def edge_early_bank(P):
    """[(L, peak)] of one bank at 16000 Hz (pre 16, post 800), every early window clipped by the RIR's end or its start: exactly
    DIRECT_TAPS and DIRECT_TAPS + 1 early taps under a full RIR beyond a partition (one row takes the time-domain path in one
    launch of aug_conv_kernel and the transform path in the other, or the transform path in both); 116 taps; an early window
    that is the whole RIR, transformed (300 taps) and in the time domain (DIRECT_TAPS taps)."""
    L = P + 100
    return [(L, L + 16 - DIRECT_TAPS), (L, L + 16 - DIRECT_TAPS - 1), (1500, 1400), (300, 5), (DIRECT_TAPS, 7)]


def early_ns(P):
    return (1, P, 2 * P + 17)


# aug_rir_peak_kernel's ties: (taps, the indices that hold the maximum). 45 / 300 and 45 / 290: threads 45 and 44 (34) of wave 0,
# the lower index in the higher lane; 70 / 260 and 100 / 260: the lower index in wave 1, the higher in wave 0; 10 / 266 / 522:
# one thread; 3 / 40 / 699 (299): three lanes, the lowest index in the lowest
TIE_CASES = [(700, (45, 300)), (300, (45, 290)), (700, (70, 260)), (300, (100, 260)), (700, (10, 266, 522)), (700, (3, 40, 699)),
             (300, (3, 40, 299))]


def rir_with_peaks(rng, L, peaks):
    """L random taps in (-1, 0.9) with the same maximum, 1.5, at every index of `peaks`."""
    h = rng.uniform(-1.0, 0.9, L)
    h[list(peaks)] = 1.5
    return h.astype(np.float32)
