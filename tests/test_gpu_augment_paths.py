"""The branches of csrc/augment.hip that test_gpu_augment.py does not reach with a value check, against the fp64 restatement of
tests/_augment_ref.py: RIRs of more partitions than the AUG_J blocks a workgroup owns, banks at 48000 and 44100 Hz whose early
window takes three partitions, early windows clipped onto the time-domain limit, int16 input on the time-domain path, and ties of
the RIR's maximum across lanes and waves. tests/test_augment_paths_cpu.py proves that each shape selects its branch.

Bounds (the project's own): per row max|y - y64| / max|y64| within 4 x the same figure of the fp32
block-FFT restatement on the same inputs; the powers within 1e-6 (relative); rows alone, chunked and as int16 bit for bit.
Measured on an MI355X: the worst e_gpu / e_ref is 3.58 and 2.56 (one sample through 13 P - 1 and 5 P taps with the peak last: the
restatement's transform of one sample is exact, e_ref 2e-8), 2.21 on the other long rows; p_sig on three early partitions deviates 5.5e-11 .. 1.84e-7, as the fp32
restatement's own does (7.3e-9 .. 1.53e-7). The figures per group are in INTEGRATION.md §2m and DESIGN.md §7."""

import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "kaldi-tflite_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import ops  # noqa: E402
import _augment_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
aug = ktf.augment
P = ops.aug_partition()
WHERE = ("first", "middle", "last")


def peak_at(where, Lh):
    return {"first": 0, "middle": Lh // 2, "last": Lh - 1}[where]


def parity(got, want, ref):
    """-> (e_gpu, e_ref, e_gpu / e_ref) of one row against the fp64 convolution `want`."""
    e_gpu, e_ref = R.rel_err(got, want), R.rel_err(ref, want)
    return e_gpu, e_ref, (e_gpu / e_ref if e_ref > 0 else (0.0 if e_gpu == 0 else np.inf))


# ----------------------------------------------------------------------------- 1: more partitions than blocks per workgroup
@functools.lru_cache(maxsize=None)
def long_set(where):
    """Every (n, L) of long_shapes(P) with the RIR's peak at `where`: signals, RIRs, the fp64 convolutions and the fp32 restatement's."""
    rng = np.random.default_rng({"first": 110, "middle": 111, "last": 112}[where])
    ns, Ls = R.long_shapes(P)
    xs, hs, y64, yref = [], [], [], []
    for n in ns:
        for Lh in Ls:
            x = (rng.standard_normal(n) * 3000).astype(np.float32)
            h = R.decaying_rir(rng, Lh, peak_at(where, Lh))
            xs.append(x)
            hs.append(h)
            y64.append(np.convolve(x.astype(np.float64), h.astype(np.float64)))
            yref.append(R.blockwise_fft_convolve_f32(x, h))
    return xs, hs, y64, yref


@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("where", WHERE)
def test_long_rir_parity(where, shift):
    xs, hs, y64, yref = long_set(where)
    bank = aug.RirBank(hs, 16000)
    assert bank.lengths.tolist() == [h.size for h in hs] and bank.peak.tolist() == [peak_at(where, h.size) for h in hs]
    out, lens = aug.augment(xs, rirs=bank, rir_ids=np.arange(len(xs)), shift_output=shift, normalize_output=False)
    out = out.cpu().numpy()
    worst, bad = 0.0, []
    for b, (x, h) in enumerate(zip(xs, hs)):
        k = peak_at(where, h.size)
        lo, hi = (k, k + x.size) if shift else (0, x.size + h.size - 1)
        assert lens[b] == hi - lo and not out[b, lens[b]:].any()
        e_gpu, e_ref, ratio = parity(out[b, :lens[b]], y64[b][lo:hi], yref[b][lo:hi])
        worst = max(worst, ratio)
        print(f"long peak={where} shift={shift} n={x.size} L={h.size}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} ratio {ratio:.2f}")
        if not e_gpu <= 4.0 * e_ref:
            bad.append((x.size, h.size, e_gpu, e_ref))
    print(f"long peak={where} shift={shift}: worst e_gpu / e_ref = {worst:.2f} (limit 4)")
    assert not bad, bad


def test_long_rir_int16_input_is_the_fp32_input():
    xs, hs, _, _ = long_set("middle")
    n = R.long_shapes(P)[0][2]
    rows = [b for b, x in enumerate(xs) if x.size == n]
    assert n == 2 * P + 17 and len(rows) == len(R.long_shapes(P)[1])
    bank = aug.RirBank(hs, 16000)
    x16 = [np.clip(np.rint(xs[b]), -32768, 32767).astype(np.int16) for b in rows]
    for shift in (True, False):
        kw = dict(rirs=bank, rir_ids=rows, shift_output=shift, normalize_output=False, return_stats=True)
        a, la, sa = aug.augment(x16, **kw)
        f, lf, sf = aug.augment([x.astype(np.float32) for x in x16], **kw)
        assert a.dtype == torch.float32 and la == lf and torch.equal(a, f) and torch.equal(sa, sf) and bool(a.any())


# ----------------------------------------------------------------------------- 2 / 3: the early window
def _bank_case(fs):
    return R.wide_early_bank(P) if fs in R.EARLY_RATES else R.edge_early_bank(P)


@functools.lru_cache(maxsize=None)
def early_set(fs):
    """One bank and every (RIR, n) row of it, integer-valued samples (so that the same rows go in as int16) -> (hs, xs, ids,
    [augment_ref per row], [fp32 restatement of the full convolution], [p_sig of the fp32 restatement of the early one])."""
    rng = np.random.default_rng(fs)
    hs = [R.decaying_rir(rng, L, k) for L, k in _bank_case(fs)]
    xs, ids, refs, yref, psig_ref = [], [], [], [], []
    for r, h in enumerate(hs):
        k, s0, s1 = R.early_window(h, fs)
        for n in R.early_ns(P):
            x = np.rint(rng.standard_normal(n) * 3000).clip(-32768, 32767).astype(np.float32)
            xs.append(x)
            ids.append(r)
            refs.append(R.augment_ref(x, h, fs=fs, shift_output=False, normalize_output=False))
            yref.append(R.blockwise_fft_convolve_f32(x, h))
            e = R.blockwise_fft_convolve_f32(x, h[s0:s1]).astype(np.float64)
            psig_ref.append(float(np.mean(e * e)))
    return hs, xs, tuple(ids), refs, yref, tuple(psig_ref)


def check_early(fs, out, lens, stats, tag):
    hs, xs, ids, refs, yref, psig_ref = early_set(fs)
    worst = {"p_before": 0.0, "p_sig": 0.0, "parity": 0.0}
    bad = []
    for b, (x, r) in enumerate(zip(xs, refs)):
        h = hs[ids[b]]
        k, s0, s1 = R.early_window(h, fs)
        assert lens[b] == r["y"].size and not out[b, lens[b]:].any()
        e_gpu, e_ref, ratio = parity(out[b, :lens[b]], r["y"], yref[b])
        dev = {name: abs(stats[b, i] - r[name]) / r[name] for i, name in enumerate(("p_before", "p_sig"))}
        dev_ref = abs(psig_ref[b] - r["p_sig"]) / r["p_sig"]
        print(f"{tag} fs={fs} rir={ids[b]} L={h.size} early={s1 - s0} n={x.size}: p_before rel {dev['p_before']:.2e} p_sig rel "
              f"{dev['p_sig']:.2e} (fp32 restatement {dev_ref:.2e}; bound 1e-6) e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} ratio {ratio:.2f}")
        worst = {"p_before": max(worst["p_before"], dev["p_before"]), "p_sig": max(worst["p_sig"], dev["p_sig"]),
                 "parity": max(worst["parity"], ratio)}
        if not (dev["p_before"] <= 1e-6 and dev["p_sig"] <= 1e-6 and e_gpu <= 4.0 * e_ref):
            bad.append((ids[b], x.size, dev, e_gpu, e_ref))
        assert stats[b, 3] == 1.0
    print(f"{tag} fs={fs}: worst p_before rel {worst['p_before']:.2e}, p_sig rel {worst['p_sig']:.2e} (bound 1e-6), "
          f"e_gpu / e_ref {worst['parity']:.2f} (limit 4)")
    assert not bad, bad


@pytest.mark.parametrize("fs", R.EARLY_RATES + (16000,))
def test_early_window_powers_and_output(fs):
    hs, xs, ids, refs, _, _ = early_set(fs)
    bank = aug.RirBank(hs, fs)
    want = [R.early_window(h, fs) for h in hs]
    meta = bank.meta.cpu().numpy()
    assert bank.peak.tolist() == [k for k, _, _ in want] == [k for _, k in _bank_case(fs)]
    assert meta[:, 1:4].tolist() == [[s0, s1, h.size] for (_, s0, s1), h in zip(want, hs)]
    assert meta[:, 4:6].tolist() == [list(v) for v in R.spectra_slots([h.size for h in hs], fs, P)]
    kw = dict(rirs=bank, rir_ids=ids, shift_output=False, normalize_output=False, sample_rate=fs, return_stats=True)
    out, lens, stats = aug.augment(xs, **kw)
    check_early(fs, out.cpu().numpy(), lens, stats.cpu().numpy(), "f32 in")
    # the same values as int16: the same bits, on the transform path and in the time domain
    x16 = [x.astype(np.int16) for x in xs]
    assert all(np.array_equal(a.astype(np.float32), x) for a, x in zip(x16, xs))
    out16, lens16, stats16 = aug.augment(x16, **kw)
    assert out16.dtype == torch.float32 and lens16 == lens and torch.equal(out16, out) and torch.equal(stats16, stats)
    # int16 out: the rounded fp32 output, whichever the input type
    for src in (xs, x16):
        i16, li, si = aug.augment(src, out_dtype=torch.int16, **kw)
        assert i16.dtype == torch.int16 and li == lens and torch.equal(si, stats)
        assert np.array_equal(i16.cpu().numpy(), R.to_int16(out.cpu().numpy()))
    # shifted: the window y[k : k + n] of the same y
    sh, ls = aug.augment(xs, **dict(kw, shift_output=True, return_stats=False))
    for b, x in enumerate(xs):
        k = want[ids[b]][0]
        assert ls[b] == x.size and torch.equal(sh[b, :x.size], out[b, k:k + x.size]) and not bool(sh[b, x.size:].any())


# ----------------------------------------------------------------------------- 4: ties of the maximum
@functools.lru_cache(maxsize=None)
def tie_rirs():
    rng = np.random.default_rng(44)
    hs = [R.rir_with_peaks(rng, L, peaks) for L, peaks in R.TIE_CASES]
    hs.append(-(rng.uniform(0.1, 1.0, 700)).astype(np.float32))          # every tap negative: the maximum is the smallest magnitude
    hs.append(-(rng.uniform(0.1, 1.0, 300)).astype(np.float32))
    hs[-1][[7, 200, 290]] = np.float32(-0.05)                              # ... and held three times
    hs.append(np.full(700, 0.25, np.float32))                            # constant taps: every thread and every wave ties
    hs.append(np.full(300, -0.25, np.float32))
    return hs


def test_peak_ties_take_the_lowest_index():
    hs = tie_rirs()
    want = [int(np.argmax(h)) for h in hs]
    assert want[:len(R.TIE_CASES)] == [min(p) for _, p in R.TIE_CASES] and want[-4:] == [want[-4], 7, 0, 0] and max(hs[-4]) < 0
    bank = aug.RirBank(hs, 16000)
    print(f"peaks {bank.peak.tolist()} (np.argmax: {want})")
    assert bank.peak.tolist() == want
    assert bank.meta.cpu().numpy()[:, 1:3].tolist() == [list(R.early_window(h, 16000)[1:]) for h in hs]
    # a unit impulse: y = h, so the shifted output is h[k:] and starts on the peak. Three transforms of log2(2 P) = 11 stages round
    # once per stage: 33 x 2^-24 = 2e-6 of the largest tap; 1e-5 leaves a factor 5. Another index of the same maximum gives another
    # window: its distance from h[k:] is printed and is four orders of magnitude above the bound.
    n = 64
    x = np.zeros(n, np.float32)
    x[0] = 1.0
    out, lens = aug.augment([x] * len(hs), rirs=bank, rir_ids=np.arange(len(hs)), shift_output=True, normalize_output=False)
    out = out.cpu().numpy()
    for r, h in enumerate(hs):
        k = want[r]
        win = np.zeros(n)
        win[:min(n, h.size - k)] = h[k:k + n]
        tol = 1e-5 * float(np.abs(h).max())
        err = float(np.abs(out[r] - win).max())
        others = [i for i in np.flatnonzero(h == h.max()) if i != k and i + n <= h.size and not np.array_equal(h[i:i + n], win)]
        gap = min((float(np.abs(h[i:i + n] - win).max()) for i in others), default=float("nan"))
        print(f"impulse through RIR {r} (L={h.size}, peak {k}): max abs err {err:.3e} (bound {tol:.3e}); the next tie's window is {gap:.3e} away")
        assert lens[r] == n and err <= tol and not gap <= 1e3 * tol
        assert abs(out[r, 0] - h.max()) <= tol


# ----------------------------------------------------------------------------- 5: rows alone and chunked
def _isolation(xs, bank, ids, fs, shift):
    kw = dict(rirs=bank, shift_output=shift, normalize_output=True, sample_rate=fs, return_stats=True)
    out, lens, stats = aug.augment(xs, rir_ids=ids, **kw)
    chunked, lens2, stats2 = aug.augment(xs, rir_ids=ids, workspace_limit=1, **kw)
    assert lens2 == lens and torch.equal(chunked, out) and torch.equal(stats2, stats)
    for b, x in enumerate(xs):
        one, l1, s1 = aug.augment([x], rir_ids=[ids[b]], **kw)
        assert l1 == [lens[b]] and torch.equal(one[0, :l1[0]], out[b, :lens[b]]) and torch.equal(s1[0], stats[b]), (b, x.size, ids[b])
        assert not bool(out[b, lens[b]:].any()) and bool(out[b, :lens[b]].any())


@pytest.mark.parametrize("shift", [True, False])
def test_long_rir_rows_are_isolated(shift):
    xs, hs, _, _ = long_set("middle")
    _isolation(xs, aug.RirBank(hs, 16000), list(range(len(xs))), 16000, shift)


@pytest.mark.parametrize("fs", R.EARLY_RATES)
def test_wide_early_rows_are_isolated(fs):
    hs, xs, ids, _, _, _ = early_set(fs)
    _isolation(xs, aug.RirBank(hs, fs), list(ids), fs, False)
