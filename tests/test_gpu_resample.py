"""ktf.augment.Resampler / resample / speed_perturb on the GPU against the fp64 restatement of tests/_resample_ref.py. Shapes are
built from T = ktf_rs_tile() so that they sit on the kernel's boundaries (one output, a tile less one, a tile, a tile and one, more
than two tiles, a row shorter than the filter).

Parity: |out - ref| <= 2^-24 |ref| + 2^-45 sum|w x| per sample, ref = resample64 with the library's fp32 table: the first term is the
single fp32 rounding, the second covers the fp64 summation (at most 2^8 taps, unit roundoff 2^-53). Measured on an MI355X: the worst
error / bound per rate pair is 0.963 to 0.991 (16000 -> 17600, int16), what a correctly rounded fp32 of the fp64 sum gives; the
figures and tools/bench_resample.py's timings (1024 x 10 s, 48000 -> 8000 int16: 0.99 ms against 8.2 ms for a strided conv1d per
phase in torch) are in DESIGN.md §7 (sample-rate conversion)."""

import functools
import math
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
import _augment_ref as A  # noqa: E402
import _resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
aug = ktf.augment
T = ops.rs_tile()
PAIRS = [(16000, 8000), (8000, 16000), (44100, 16000), (48000, 8000), (16000, 17600), (16000, 14400)]
TARGETS = (0, 1, 2, T - 1, T, T + 1, 2 * T + 17)


def n_for(m, fi, fo):
    """The fewest input samples that give at least m outputs (exactly m whenever some n gives m: always when fi > fo)."""
    if m == 0:
        return 0
    g = math.gcd(fi, fo)
    n = max(1, (m - 1) * (fi // g) // (fo // g))
    while R.num_out(n, fi, fo) < m:
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def batch(fi, fo):
    """The ragged batch of a rate pair: rows for every target length, and one shorter than the filter; fp32 samples."""
    rng = np.random.default_rng(fi + fo)
    ns = [n_for(m, fi, fo) for m in TARGETS] + [5]
    if fi > fo:
        assert [R.num_out(n, fi, fo) for n in ns[:-1]] == list(TARGETS)
    return ns, [(rng.standard_normal(n) * 3000).astype(np.float32) for n in ns]


@functools.lru_cache(maxsize=None)
def reference(fi, fo, i16):
    """(rows, [(fp64 sums, sum |w x|)]) of the batch through resample64 with the library's table."""
    ns, xs = batch(fi, fo)
    if i16:
        xs = [np.clip(np.rint(x), -32768, 32767).astype(np.int16) for x in xs]
    iu, ou, first, taps, w = ops.rs_plan(fi, fo, R.default_cutoff(fi, fo), 6)
    refs = [R.resample64(x.astype(np.float32), first, taps, w, iu, ou, R.num_out(x.size, fi, fo)) for x in xs]
    return xs, refs


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("fi,fo", PAIRS)
def test_parity(fi, fo, i16):
    xs, refs = reference(fi, fo, i16)
    rs = aug.Resampler(fi, fo)
    assert min(x.size for x in xs if x.size) < int(rs.taps.min())
    out, lens = rs(xs, out_dtype=torch.float32)
    assert out.dtype == torch.float32 and out.shape == (len(xs), max(lens))
    assert lens == [R.num_out(x.size, fi, fo) for x in xs] == [rs.num_out(x.size) for x in xs]
    out = out.cpu().numpy()
    worst = 0.0
    for b, (y, mag) in enumerate(refs):
        assert not out[b, lens[b]:].any()
        if not lens[b]:
            continue
        err = np.abs(out[b, :lens[b]].astype(np.float64) - y)
        bound = 2.0 ** -24 * np.abs(y) + 2.0 ** -45 * mag
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, ratio)
        print(f"parity {fi} -> {fo} {'i16' if i16 else 'f32'} n={xs[b].size} m={lens[b]}: worst err / bound {ratio:.3f}")
        assert (err <= bound).all()
    print(f"parity {fi} -> {fo} {'i16' if i16 else 'f32'}: worst err / bound = {worst:.3f} (limit 1)")


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("fi,fo", [(44100, 16000), (48000, 8000), (16000, 17600)])
def test_rows_are_isolated(fi, fo, i16):
    xs, _ = reference(fi, fo, i16)
    rs = aug.Resampler(fi, fo)
    out, lens = rs(xs)
    again, lens2 = rs(xs)
    assert lens == lens2 and torch.equal(out, again)
    # the same rows in a wider tensor whose padding past n must never be read, in another order
    order = list(reversed(range(len(xs))))
    ldx = max(x.size for x in xs) + 37
    pad = 32767 if i16 else float("nan")
    wide = torch.full((len(xs), ldx), pad, dtype=torch.int16 if i16 else torch.float32, device="cuda")
    for r, b in enumerate(order):
        wide[r, :xs[b].size] = torch.as_tensor(xs[b], device="cuda")
    got, glens = rs(wide[:, :ldx - 3], lengths=[xs[b].size for b in order])
    assert glens == [lens[b] for b in order]
    for r, b in enumerate(order):
        one, l1 = rs(xs[b])
        assert l1 == [lens[b]] and one.shape == (1, lens[b])
        assert torch.equal(one[0], out[b, :lens[b]]) and torch.equal(got[r, :lens[b]], one[0])
        assert not got[r, lens[b]:].any() and not out[b, lens[b]:].any()


def test_int16_output_rounds_and_saturates():
    fi, fo = 16000, 8000
    rs = aug.Resampler(fi, fo)
    rng = np.random.default_rng(5)
    square = (32767 * np.where((np.arange(3 * T) // 40) % 2 == 0, 1, -1)).astype(np.int16)      # full scale, 200 Hz
    xs = [square, (rng.standard_normal(2 * T + 3) * 9000).clip(-32768, 32767).astype(np.int16), square[:T - 5].copy()]
    f32, lens = rs(xs, out_dtype=torch.float32)
    i16, lens16 = rs(xs)
    assert i16.dtype == torch.int16 and lens16 == lens
    want = R.to_int16(f32.cpu().numpy())
    assert np.array_equal(i16.cpu().numpy(), want)
    y, _ = R.resample64(square.astype(np.float32), rs.first, rs.taps, rs.weights, rs.iu, rs.ou, lens[0])
    assert y.max() > 32767 and y.min() < -32768                   # the filter overshoots at the edges: the case is real
    assert (want[0] == 32767).any() and (want[0] == -32768).any()
    from_f32, _ = rs([x.astype(np.float32) for x in xs], out_dtype=torch.int16)
    assert torch.equal(from_f32, i16)
    halves = aug.Resampler(1, 2, lowpass_cutoff=0.5, num_zeros=1)  # phase 0 of this plan: weight 1 at the sample itself, 0 beside it
    assert halves.first[0] == -1 and halves.weights[0].tolist() == [0.0, 1.0, 0.0]
    tie, _ = halves(torch.tensor([[0.5, 1.5, 2.5, -0.5, -1.5, 40000.0, -40000.0]], device="cuda"), out_dtype=torch.int16)
    assert tie.cpu()[0, ::2].tolist() == [0, 2, 2, 0, -2, 32767, -32768]


def test_speed_perturb():
    rng = np.random.default_rng(6)
    x = torch.as_tensor((rng.standard_normal((3, 16000)) * 3000).astype(np.float32), device="cuda")
    lengths = [16000, 12345, 1]
    for factor, p, q, big, m_full in ((1.1, 11, 10, (17600, 16000), 14546), (0.9, 9, 10, (14400, 16000), 17778)):
        out, lens = aug.speed_perturb(x, factor, lengths=lengths)
        assert lens == [R.num_out(n, p, q) for n in lengths] and lens[0] == m_full
        small, l2 = aug.Resampler(p, q)(x, lengths=lengths)
        scaled, l3 = aug.Resampler(*big)(x, lengths=lengths)       # the plan depends on the ratio only: the same table, the same bits
        assert np.array_equal(aug.Resampler(p, q).weights, aug.Resampler(*big).weights)
        assert l2 == lens == l3 and torch.equal(small, out) and torch.equal(scaled, out)
    same, lens = aug.speed_perturb(x, 1.0, lengths=lengths)
    assert same is x and lens == lengths


def test_resampled_banks_run_through_augment():
    """16 kHz RIRs and noises taken to 8 kHz, banks built at 8000 Hz, augment at sample_rate=8000: against tests/_augment_ref.py on
    the same resampled arrays, under the bounds of test_gpu_augment.py (§2m)."""
    rng = np.random.default_rng(7)
    rirs16 = [A.decaying_rir(rng, 3000, 40), A.decaying_rir(rng, 90, 6)]
    noises16 = [(rng.standard_normal(5000) * 300).astype(np.float32), (rng.standard_normal(1500) * 100).astype(np.float32)]
    r8, rl = aug.resample(rirs16, 16000, 8000)
    n8, nl = aug.resample(noises16, 16000, 8000)
    assert rl == [1500, 45] and nl == [2500, 750]
    rirs8 = [r8[b, :l].cpu().numpy() for b, l in enumerate(rl)]
    noises8 = [n8[b, :l].cpu().numpy() for b, l in enumerate(nl)]
    with pytest.raises(ValueError, match="resampling"):
        aug.augment(np.zeros((1, 100), np.float32), rirs=aug.RirBank(rirs16, 16000), rir_ids=[0], sample_rate=8000)
    bank, nb = aug.RirBank(rirs8, sample_rate=8000), aug.NoiseBank(noises8, sample_rate=8000)
    xs = [(rng.standard_normal(n) * 2500).astype(np.float32) for n in (4000, 2100, 800)]
    ids = [0, 1, -1]
    adds = [[(0, 10.0, 0, 0)], [(1, 5.0, 100, 1200), (0, 15.0, 0, 0)], [(1, 8.0, 10, 0)]]
    secs = [[(nid, snr, o / 8000, d / 8000) for nid, snr, o, d in row] for row in adds]
    out, lens, stats = aug.augment(xs, rirs=bank, rir_ids=ids, noises=nb, additives=secs, shift_output=False, normalize_output=False,
                                   sample_rate=8000, return_stats=True)
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    EPS = 2.0 ** -24
    for b, x in enumerate(xs):
        h = rirs8[ids[b]] if ids[b] >= 0 else None
        r = A.augment_ref(x, h, adds[b], noises8, 8000, shift_output=False, normalize_output=False)
        assert lens[b] == r["y"].size
        for name, got in (("p_before", stats[b, 0]), ("p_sig", stats[b, 1]), ("p_after", stats[b, 2])):
            assert abs(got - r[name]) <= 1e-6 * r[name]
        e_ref, ymax = 0.0, 0.0
        if h is not None:
            y64 = np.convolve(x.astype(np.float64), h.astype(np.float64))
            e_ref, ymax = A.rel_err(A.blockwise_fft_convolve_f32(x, h), y64), float(np.abs(y64).max())
        mags = [g * float(np.abs(A.noise_piece(noises8[a[0]], a[3])).max()) for a, g in zip(adds[b], r["gains"])]
        tol = 4.0 * e_ref * ymax + 3 * EPS * len(mags) * (float(np.abs(r["y"]).max()) + sum(mags)) + 0.5e-6 * sum(mags)
        err = float(np.abs(out[b, :lens[b]] - r["y"]).max())
        print(f"row {b}: max abs err {err:.3e} (bound {tol:.3e})")
        assert err <= tol
