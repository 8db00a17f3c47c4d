"""ktf.augment on the GPU against the fp64 restatement of tests/_augment_ref.py. Shapes are built from P = ktf_aug_partition() so
that they sit on the kernels' boundaries (a partition, the time-domain path's tap limit, the blocks a workgroup owns).

Convolution parity: per utterance max|y - y64| / max|y64| against 4 x the same figure of the fp32 block-FFT restatement on the same
inputs (measured on an MI355X: the worst ratio on the transform path was 2.58; the figures are in DESIGN.md's augmentation section)."""

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
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
aug = ktf.augment
P = ops.aug_partition()
DIRECT = 64                                     # KTF_AUG_DIRECT_TAPS: up to it a filter is applied in the time domain
NS = (1, P - 1, P, P + 1, 2 * P + 17)
LS = (1, 2, DIRECT, DIRECT + 1, P - 1, P, P + 1, 3 * P + 5)
FS = 16000
EPS = 2.0 ** -24


def peak_at(where, Lh):
    return {"first": 0, "middle": Lh // 2, "last": Lh - 1}[where]


@functools.lru_cache(maxsize=None)
def parity_set(where):
    """Every (n, L) of NS x LS with the RIR's peak at `where`: signals, RIRs, the fp64 convolutions and the fp32 restatement's."""
    rng = np.random.default_rng({"first": 10, "middle": 11, "last": 12}[where])
    xs, hs, y64, yref = [], [], [], []
    for n in NS:
        for Lh in LS:
            x = (rng.standard_normal(n) * 3000).astype(np.float32)
            h = R.decaying_rir(rng, Lh, peak_at(where, Lh))
            xs.append(x)
            hs.append(h)
            y64.append(np.convolve(x.astype(np.float64), h.astype(np.float64)))
            yref.append(R.blockwise_fft_convolve_f32(x, h))
    return xs, hs, y64, yref


@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_convolution_parity(where, shift):
    xs, hs, y64, yref = parity_set(where)
    bank = aug.RirBank(hs, FS)
    assert bank.lengths.tolist() == [h.size for h in hs]
    assert bank.peak.tolist() == [peak_at(where, h.size) for h in hs]
    out, lens = aug.augment(xs, rirs=bank, rir_ids=np.arange(len(xs)), shift_output=shift, normalize_output=False)
    out = out.cpu().numpy()
    worst = 0.0
    bad = []
    for b, (x, h) in enumerate(zip(xs, hs)):
        k = peak_at(where, h.size)
        lo, hi = (k, k + x.size) if shift else (0, x.size + h.size - 1)
        assert lens[b] == hi - lo and not out[b, lens[b]:].any()
        e_gpu, e_ref = R.rel_err(out[b, :lens[b]], y64[b][lo:hi]), R.rel_err(yref[b][lo:hi], y64[b][lo:hi])
        ratio = e_gpu / e_ref if e_ref > 0 else (0.0 if e_gpu == 0 else np.inf)
        worst = max(worst, ratio)
        print(f"parity peak={where} shift={shift} n={x.size} L={h.size}: e_gpu {e_gpu:.3e} e_ref {e_ref:.3e} ratio {ratio:.2f}")
        if not e_gpu <= 4.0 * e_ref:
            bad.append((x.size, h.size, e_gpu, e_ref))
    print(f"parity peak={where} shift={shift}: worst e_gpu / e_ref = {worst:.2f} (limit 4)")
    assert not bad, bad


def _mixed_batch():
    """A ragged batch: n = 0, rows without an RIR, shared and distinct RIRs, empty and overlapping additive lists."""
    rng = np.random.default_rng(20)
    hs = [R.decaying_rir(rng, P + 300, 40), R.decaying_rir(rng, 2 * P + 1, 700), R.decaying_rir(rng, 30, 3)]
    noises = [(rng.standard_normal(700) * 80).astype(np.float32), (rng.standard_normal(3 * P) * 500).astype(np.float32),
              np.zeros(50, np.float32)]
    ns = [2 * P + 17, 0, P, 5000, 333, 4 * P + 1, 0, 1]
    ids = [0, 1, -1, 1, 2, 0, -1, 2]
    xs = [(rng.standard_normal(n) * 2500).astype(np.float32) for n in ns]
    adds = [
        [(0, 10.0, 0, 0), (1, 5.0, 100, 2000)],                  # start at 0; two overlapping
        [(0, 10.0, 0, 0)],                                       # on an empty row: nothing
        [(0, 3.0, 10, 1800)],                                    # d > m: the noise wraps; no RIR
        [],
        [(1, 15.0, 300, 0), (2, 0.0, 0, 0)],                     # cut by the end of y; a silent noise
        [(1, 8.0, 0, 100), (0, 12.0, 10 ** 6, 0), (0, 0.0, 5 * P + 299, 0)],   # d < m; beyond the end; the last sample only
        [],
        [(0, 20.0, 0, 5)],
    ]
    return xs, hs, ids, noises, adds


def _seconds(adds):
    return [[(nid, snr, o / FS, d / FS) for nid, snr, o, d in row] for row in adds]


def _conv_ref_err(x, h):
    """The fp32 restatement's error on this row's convolution, and max|y64|."""
    y64 = np.convolve(x.astype(np.float64), h.astype(np.float64))
    return R.rel_err(R.blockwise_fft_convolve_f32(x, h), y64), float(np.abs(y64).max())


def test_additives_and_powers():
    xs, hs, ids, noises, adds = _mixed_batch()
    bank, nb = aug.RirBank(hs, FS), aug.NoiseBank(noises, FS)
    out, lens, stats = aug.augment(xs, rirs=bank, rir_ids=ids, noises=nb, additives=_seconds(adds), shift_output=False,
                                   normalize_output=False, return_stats=True)
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    for b, x in enumerate(xs):
        h = hs[ids[b]] if ids[b] >= 0 else None
        r = R.augment_ref(x, h, adds[b], noises, FS, shift_output=False, normalize_output=False)
        assert lens[b] == r["y"].size
        for name, got in (("p_before", stats[b, 0]), ("p_sig", stats[b, 1]), ("p_after", stats[b, 2])):
            err = abs(got - r[name]) / r[name] if r[name] > 0 else abs(got)
            print(f"row {b} {name}: {got:.9e} oracle {r[name]:.9e} rel {err:.2e} (bound 1e-6)")
            assert err <= 1e-6
        assert stats[b, 3] == 1.0
        if x.size == 0:
            continue
        # the convolution within 4 x the fp32 restatement's error; each add rounds the gain, the product and the sum once, and its
        # gain follows p_sig, which may sit 1e-6 (relative) from the oracle's: 0.5e-6 on the gain
        e_ref, ymax = _conv_ref_err(x, h) if h is not None else (0.0, 0.0)
        mags = [g * float(np.abs(R.noise_piece(noises[a[0]], a[3])).max()) for a, g in zip(adds[b], r["gains"])]
        tol = 4.0 * e_ref * ymax + 3 * EPS * len(mags) * (float(np.abs(r["y"]).max()) + sum(mags)) + 0.5e-6 * sum(mags)
        err = float(np.abs(out[b, :lens[b]] - r["y"]).max())
        print(f"row {b} n={x.size} rir={ids[b]} additives={len(adds[b])}: max abs err {err:.3e} (bound {tol:.3e})")
        assert err <= tol
    # the silent noise and the additive beyond the end changed nothing: the same rows without them are bit-equal
    trimmed = [list(row) for row in adds]
    trimmed[4], trimmed[5] = trimmed[4][:1], [trimmed[5][0], trimmed[5][2]]
    again, _ = aug.augment(xs, rirs=bank, rir_ids=ids, noises=nb, additives=_seconds(trimmed), shift_output=False, normalize_output=False)
    assert np.array_equal(again.cpu().numpy(), out)
    base, _ = aug.augment(xs, rirs=bank, rir_ids=ids, shift_output=False, normalize_output=False)
    base = base.cpu().numpy()
    end = lens[5] - 1                                             # row 5: 100 samples from 0, and the last sample of y
    assert not np.array_equal(base[5, :100], out[5, :100]) and np.array_equal(base[5, 100:end], out[5, 100:end])
    assert base[5, end] != out[5, end]


def test_normalisation_and_volume():
    xs, hs, ids, noises, adds = _mixed_batch()
    bank, nb = aug.RirBank(hs, FS), aug.NoiseBank(noises, FS)
    kw = dict(rirs=bank, rir_ids=ids, noises=nb, additives=_seconds(adds), shift_output=False)
    raw, lens = aug.augment(xs, normalize_output=False, **kw)
    out, _, stats = aug.augment(xs, normalize_output=True, return_stats=True, **kw)
    vol, _, vstats = aug.augment(xs, normalize_output=True, volume=0.25, return_stats=True, **kw)
    raw, out, vol, stats, vstats = (v.cpu().numpy() for v in (raw, out, vol, stats, vstats))
    for b, x in enumerate(xs):
        if x.size == 0:
            assert lens[b] == 0 and stats[b].tolist() == [0.0, 0.0, 0.0, 1.0]
            continue
        y = out[b, :lens[b]].astype(np.float64)
        dev = abs(np.mean(y * y) / stats[b, 0] - 1.0)
        print(f"row {b}: mean(y^2) / p_before - 1 = {dev:.2e} (bound 1e-5)")
        assert dev <= 1e-5
        assert abs(stats[b, 3] - np.sqrt(stats[b, 0] / stats[b, 2])) <= 1e-12 * stats[b, 3]
        assert np.array_equal(out[b, :lens[b]], raw[b, :lens[b]] * np.float32(stats[b, 3]))
        assert vstats[b, 3] == 0.25 and np.array_equal(vol[b, :lens[b]], raw[b, :lens[b]] * np.float32(0.25))


def test_ragged_batch_is_bit_exact_per_row_run_and_chunking():
    xs, hs, ids, noises, adds = _mixed_batch()
    bank, nb = aug.RirBank(hs, FS), aug.NoiseBank(noises, FS)
    for shift in (True, False):
        kw = dict(noises=nb, shift_output=shift, normalize_output=True, return_stats=True)
        out, lens, stats = aug.augment(xs, rirs=bank, rir_ids=ids, additives=_seconds(adds), **kw)
        again, lens2, stats2 = aug.augment(xs, rirs=bank, rir_ids=ids, additives=_seconds(adds), **kw)
        assert lens == lens2 and torch.equal(out, again) and torch.equal(stats, stats2)
        assert lens == [(x.size if shift or ids[b] < 0 or x.size == 0 else x.size + hs[ids[b]].size - 1) for b, x in enumerate(xs)]
        for limit in (1, 300000):                               # one row per chunk; a few rows per chunk
            chunked, lens3, stats3 = aug.augment(xs, rirs=bank, rir_ids=ids, additives=_seconds(adds), workspace_limit=limit, **kw)
            assert lens3 == lens and torch.equal(out, chunked) and torch.equal(stats, stats3)
        for b, x in enumerate(xs):
            one, l1, s1 = aug.augment([x], rirs=bank, rir_ids=[ids[b]], additives=_seconds([adds[b]]), **kw)
            assert l1 == [lens[b]] and torch.equal(one[0, :l1[0]], out[b, :lens[b]]) and torch.equal(s1[0], stats[b])
            assert not out[b, lens[b]:].any()
    # the CSR form of the additives, and a (B, T) tensor with lengths, are the list forms
    T = max(x.size for x in xs)
    dense = np.zeros((len(xs), T), np.float32)
    for b, x in enumerate(xs):
        dense[b, :x.size] = x
    off = np.cumsum([0] + [len(r) for r in adds]).astype(np.int32)
    table = np.array([a for r in _seconds(adds) for a in r], np.float64)
    csr = (torch.as_tensor(off, device="cuda"), torch.as_tensor(table, device="cuda"))
    got, lens4 = aug.augment(torch.as_tensor(dense, device="cuda"), lengths=[x.size for x in xs], rirs=bank, rir_ids=ids, noises=nb,
                             additives=csr, shift_output=False)
    assert lens4 == lens and torch.equal(got, out)


def test_int16_output_and_input():
    rng = np.random.default_rng(30)
    hs = [R.decaying_rir(rng, P + 7, 20)]
    noises = [(rng.standard_normal(900) * 300).astype(np.float32)]
    xs16 = [(rng.standard_normal(n) * 6000).clip(-32768, 32767).astype(np.int16) for n in (2 * P + 5, 700, P)]
    bank, nb = aug.RirBank(hs, FS), aug.NoiseBank(noises, FS)
    adds = [[(0, 5.0, 0.0, 0.1)], [], [(0, 10.0, 0.01, 0.0)]]
    for volume in (0.0, 6.5):                                     # 6.5: a good part of the samples saturates
        kw = dict(rirs=bank, rir_ids=[0, -1, 0], noises=nb, additives=adds, volume=volume)
        f32, lens = aug.augment(xs16, **kw)
        i16, lens16 = aug.augment(xs16, out_dtype=torch.int16, **kw)
        assert i16.dtype == torch.int16 and lens16 == lens == [x.size for x in xs16]
        want = R.to_int16(f32.cpu().numpy())
        assert np.array_equal(i16.cpu().numpy(), want)
        if volume:
            assert (want == 32767).any() and (want == -32768).any()
        from_f32, _ = aug.augment([x.astype(np.float32) for x in xs16], **kw)
        assert torch.equal(from_f32, f32)
    halves = torch.tensor([[0.5, 1.5, 2.5, -0.5, -1.5, 40000.0, -40000.0]], device="cuda")
    tie, _ = aug.augment(halves, normalize_output=False, out_dtype=torch.int16)
    assert tie.cpu().tolist() == [[0, 2, 2, 0, -2, 32767, -32768]]


def test_hand_over_to_the_extractor():
    ext = synth.build_extractor(ktf, synth.extractor_cfg(), synth.make_weights(seed=4321, narrow=True), gemm="f32")
    wav = synth.make_wav(3, 2 * FS, seed=77)
    rng = np.random.default_rng(40)
    bank = aug.RirBank([R.decaying_rir(rng, 4000, 60), R.decaying_rir(rng, 1500, 10)], FS)
    nb = aug.NoiseBank([(rng.standard_normal(FS) * 200).astype(np.float32), (rng.standard_normal(3 * FS) * 200).astype(np.float32)], FS)
    plan = aug.plan_additives("babble", [2.0] * 3, nb.lengths_s, seed=3)
    out, lens = aug.augment(torch.as_tensor(wav, device="cuda"), rirs=bank, rir_ids=[0, 1, -1], noises=nb, additives=plan)
    assert out.shape == (3, 2 * FS) and out.dtype == torch.float32 and lens == [2 * FS] * 3
    units = ext.ldaMat.shape[0]
    emb = ext.embeddings(out)
    assert emb.shape == (3, units) and bool(torch.isfinite(emb).all())
    assert ext(out).shape == (3, ext.ldaMat.shape[1])
    ragged, rl = aug.augment([wav[0], wav[1][:FS + 123]], rirs=bank, rir_ids=[1, 0], noises=nb,
                             additives=aug.plan_additives("noise", [2.0, (FS + 123) / FS], nb.lengths_s, seed=4))
    assert rl == [2 * FS, FS + 123]
    win = ext.extract_windows([ragged[b, :n] for b, n in enumerate(rl)])
    assert len(win.lengths) == 2 and win.xvectors.shape[0] == sum(win.lengths) and bool(torch.isfinite(win.xvectors).all())
