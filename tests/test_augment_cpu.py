"""Waveform augmentation without a GPU: the fp64 restatement (tests/_augment_ref.py) against scipy and hand cases, plan_additives,
the C-ABI of include/ktf_augment.h (symbols, argument checks before any launch) and the ops.aug_* wrappers' library calls, pinned
in tests/golden/augment_calls.txt in the manner of test_ops_calls_cpu.py (on tests/_recorder.Recorder, with a recorder of its own).

    python tests/test_augment_cpu.py --write      # regenerate the golden file (only for a deliberate change of behaviour)
"""

import contextlib
import ctypes as C
import difflib
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "kaldi-tflite_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import _lib as L, ops  # noqa: E402
import _augment_ref as R  # noqa: E402
from _recorder import STREAM, Recorder  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "augment_calls.txt")
HOST_HELPERS = re.compile(r"ktf_aug_(partition|tables_floats|rir_spectra_floats|workspace_bytes)")
F32, F64, I32, I16, U8 = torch.float32, torch.float64, torch.int32, torch.int16, torch.uint8


# ----------------------------------------------------------------------------- the oracle
def test_oracle_matches_scipy_fftconvolve():
    import scipy.signal as sig
    rng = np.random.default_rng(0)
    for n, Lh, peak in ((1000, 1, 0), (777, 300, 20), (50, 400, 399)):
        x = (rng.standard_normal(n) * 3000).astype(np.float32)
        h = R.decaying_rir(rng, Lh, peak)
        r = R.augment_ref(x, h, shift_output=False, normalize_output=False)
        want = sig.fftconvolve(x.astype(np.float64), h.astype(np.float64))
        assert r["y"].shape == (n + Lh - 1,) and r["k"] == peak
        assert np.abs(r["out"] - want).max() <= 1e-9 * np.abs(want).max()
        k, s0, s1 = R.early_window(h, 16000)
        e = sig.fftconvolve(x.astype(np.float64), h[s0:s1].astype(np.float64))
        assert (s0, s1) == (max(0, peak - 16), min(Lh, peak + 800))
        assert abs(r["p_sig"] - np.mean(e * e)) <= 1e-9 * r["p_sig"]


def test_oracle_peak_is_the_lowest_index_of_the_signed_maximum():
    h = np.array([0.1, -5.0, 2.0, 0.3, 2.0], np.float32)
    assert R.early_window(h, 16000) == (2, 0, 5)
    assert R.early_window(h, 1000) == (2, 1, 5)          # round(0.001 * 1000) = 1, round(0.05 * 1000) = 50


def test_oracle_delta_rir_with_shift_returns_the_signal():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(321) * 1000).astype(np.float32)
    for Lh, k in ((1, 0), (40, 17), (40, 39)):
        h = np.zeros(Lh, np.float32)
        h[k] = 1.0
        r = R.augment_ref(x, h, shift_output=True, normalize_output=False)
        assert r["k"] == k and np.array_equal(r["out"], x.astype(np.float64))
        assert abs(r["p_sig"] * (x.size + min(Lh, k + 800) - max(0, k - 16) - 1) / x.size - r["p_before"]) <= 1e-12 * r["p_before"]


def test_oracle_additive_inside_y_realises_its_snr():
    rng = np.random.default_rng(2)
    x = (rng.standard_normal(4000) * 2000).astype(np.float32)
    h = R.decaying_rir(rng, 500, 30)
    noises = [(rng.standard_normal(700) * 50).astype(np.float32), (rng.standard_normal(5000) * 900).astype(np.float32)]
    for nid, snr, o, d in ((0, 10.0, 100, 0), (0, 0.0, 0, 2500), (1, -5.0, 400, 300), (1, 20.0, 0, 4499)):
        r = R.augment_ref(x, h, [(nid, snr, o, d)], noises, normalize_output=False)
        e = R.noise_piece(noises[nid], d)
        assert o + e.size <= r["y"].size
        got = 10.0 * np.log10(r["p_sig"] / np.mean((r["gains"][0] * e) ** 2))
        assert abs(got - snr) <= 1e-12
    silent = R.augment_ref(x, h, [(0, 10.0, 0, 0)], [np.zeros(10, np.float32)], normalize_output=False)
    assert silent["gains"] == [0.0] and np.array_equal(silent["y"], R.augment_ref(x, h, normalize_output=False)["y"])


def test_oracle_normalisation_restores_the_power_and_volume_overrides():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(3000) * 2000).astype(np.float32)
    h = R.decaying_rir(rng, 900, 100)
    noises = [(rng.standard_normal(1234) * 300).astype(np.float32)]
    adds = [(0, 5.0, 0, 3899), (0, 8.0, 3000, 0)]
    r = R.augment_ref(x, h, adds, noises, shift_output=False, normalize_output=True)
    assert abs(np.mean(r["out"] ** 2) / r["p_before"] - 1.0) <= 1e-12
    v = R.augment_ref(x, h, adds, noises, shift_output=False, normalize_output=True, volume=0.25)
    assert v["scale"] == 0.25 and np.allclose(v["out"], 0.25 * v["y"], rtol=0, atol=0)
    cut = R.augment_ref(x, h, [(0, 5.0, 3898, 0), (0, 5.0, 3899, 0), (0, 5.0, 10 ** 6, 0)], noises, shift_output=False, normalize_output=False)
    base = R.augment_ref(x, h, shift_output=False, normalize_output=False)["y"]
    assert np.array_equal(cut["y"][:3898], base[:3898]) and cut["y"][3898] != base[3898]       # one sample of the first, none of the others


def test_oracle_int16_rounds_to_even_and_saturates():
    assert R.to_int16([0.5, 1.5, 2.5, -0.5, -1.5, 40000.0, -40000.0, 32767.4, -32768.5]).tolist() == \
        [0, 2, 2, 0, -2, 32767, -32768, 32767, -32768]


def test_blockwise_restatement_is_the_convolution():
    rng = np.random.default_rng(4)
    for n, Lh in ((1, 1), (300, 2), (2000, 257), (100, 600)):
        x = rng.standard_normal(n).astype(np.float32)
        h = R.decaying_rir(rng, Lh, 0)
        y64 = np.convolve(x.astype(np.float64), h.astype(np.float64))
        assert R.rel_err(R.blockwise_fft_convolve_f32(x, h), y64) < 2e-6


# ----------------------------------------------------------------------------- plan_additives
@pytest.mark.parametrize("kind,snrs", [("noise", {15, 10, 5, 0}), ("music", {15, 10, 8, 5}), ("babble", {20, 17, 15, 13})])
def test_plan_additives(kind, snrs):
    lengths = [0.4, 3.0, 7.25, 12.0]
    pool = [0.3, 1.7, 5.0, 30.0]
    plan = ktf.augment.plan_additives(kind, lengths, pool, seed=7)
    assert plan == ktf.augment.plan_additives(kind, lengths, pool, seed=7)
    assert plan != ktf.augment.plan_additives(kind, lengths, pool, seed=8)
    assert len(plan) == len(lengths)
    for dur, row in zip(lengths, plan):
        for nid, snr, start, d in row:
            assert 0 <= nid < len(pool) and snr in snrs
            assert 0.0 <= start < dur and 0.0 < d and start + d <= dur + 1e-12
        if kind == "noise":
            assert [a[2] for a in row] == [float(i) for i in range(int(np.ceil(dur)))]
            assert all(a[3] == min(pool[a[0]], dur - a[2]) for a in row)
        else:
            assert all(a[2] == 0.0 and a[3] == dur for a in row)
            assert len(row) == 1 if kind == "music" else 3 <= len(row) <= 7
    if kind == "babble":
        counts = {len(r) for r in ktf.augment.plan_additives(kind, [5.0] * 200, pool, seed=1)}
        assert counts == {3, 4, 5, 6, 7}
    with pytest.raises(ValueError):
        ktf.augment.plan_additives("speech", lengths, pool, seed=0)
    with pytest.raises(ValueError):
        ktf.augment.plan_additives(kind, lengths, [], seed=0)


# ----------------------------------------------------------------------------- the C-ABI
def test_header_symbols_are_the_augment_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_augment.h")).read()
    declared = set(re.findall(r"\b(ktf_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.AUGMENT_PROTOTYPES), declared ^ set(L.AUGMENT_PROTOTYPES)
    lib = L.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert len(L.PROTOTYPES) == 120
    assert not set(L.PROTOTYPES) & set(L.AUGMENT_PROTOTYPES)
    core = open(os.path.join(ROOT, "include", "ktf_hip.h")).read()
    assert "ktf_aug_" not in core
    assert lib.ktf_aug_partition() == 1024 and lib.ktf_aug_tables_floats() == 4096


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


def _refused(rc, text):
    assert rc == -1, rc
    assert text in L.last_error(), L.last_error()
    with pytest.raises(ValueError):
        L.check(rc, "x")


def test_argument_checks_without_gpu():
    lib = L.load()
    buf = (C.c_float * 64)()                 # stands for any non-null device pointer: every refusal below comes before a launch
    n, ids, lens, off = _i32(100, 50), _i32(0, -1), _i32(300), _i32(0, 300)
    add_off = _i32(0, 1, 1)
    noise_off = (C.c_int64 * 2)(0, 500)

    def adds(noise=0, snr=10.0, start=0, dur=0):
        a = _i32(noise, 0, start, dur)
        C.cast(a, C.POINTER(C.c_float))[1] = snr
        return a

    def convolve(x=buf, ldx=100, n=n, n_dev=buf, ids=ids, ids_dev=buf, B=2, lens=lens, R=1, fs=16000, h=buf, off_dev=buf, meta=buf,
                 spectra=buf, tables=buf, A=0, stats=buf, ws=buf, ws_bytes=1 << 30):
        return lib.ktf_aug_convolve(x, 0, ldx, n, n_dev, ids, ids_dev, B, lens, R, fs, h, off_dev, meta, spectra, tables, A, stats, ws,
                                    ws_bytes, None)

    def mix(n=n, n_dev=buf, ids=ids, ids_dev=buf, B=2, lens=lens, R=1, fs=16000, meta=buf, add_off=add_off, add_off_dev=buf, a=None,
            a_dev=buf, noise=buf, noise_off=noise_off, noise_off_dev=buf, M=1, volume=0.0, out=buf, ldo=100, T_out=100, stats=buf, ws=buf):
        return lib.ktf_aug_mix(n, n_dev, ids, ids_dev, B, lens, R, fs, meta, add_off, add_off_dev, a if a is not None else adds(), a_dev,
                               noise, noise_off, noise_off_dev, M, 1, 1, volume, out, 0, ldo, T_out, stats, ws, 1 << 30, None)

    # null pointers
    _refused(lib.ktf_aug_tables(None, None), "null")
    _refused(lib.ktf_aug_rir_spectra_floats(None, 1, 16000), "null")
    _refused(lib.ktf_aug_rir_prepare(None, off, buf, 1, 16000, buf, buf, buf, None), "null")
    _refused(lib.ktf_aug_rir_prepare(buf, off, buf, 1, 16000, buf, None, buf, None), "null")
    _refused(lib.ktf_aug_workspace_bytes(None, ids, 2, lens, 1, 16000, 0), "null")
    _refused(convolve(x=None), "null")
    _refused(convolve(n=None), "null")
    _refused(convolve(stats=None), "null")
    _refused(convolve(spectra=None), "null")
    _refused(mix(out=None), "null")
    _refused(mix(add_off=None), "null")
    _refused(mix(a_dev=None), "null")
    # negative sizes
    _refused(lib.ktf_aug_rir_spectra_floats(off, -1, 16000), "negative size")
    _refused(lib.ktf_aug_rir_prepare(buf, off, buf, -1, 16000, buf, buf, buf, None), "negative size")
    _refused(lib.ktf_aug_workspace_bytes(n, ids, -2, lens, 1, 16000, 0), "negative size")
    _refused(lib.ktf_aug_workspace_bytes(n, ids, 2, lens, 1, 16000, -1), "negative size")
    _refused(lib.ktf_aug_workspace_bytes(_i32(100, -5), ids, 2, lens, 1, 16000, 0), "negative size")
    _refused(convolve(B=-1), "negative size")
    _refused(convolve(ldx=-1), "negative size")
    _refused(mix(R=-1), "negative size")
    _refused(mix(T_out=-1), "negative size")
    _refused(mix(a=adds(dur=-3)), "negative size")
    # ids out of range
    _refused(lib.ktf_aug_workspace_bytes(n, _i32(0, 1), 2, lens, 1, 16000, 0), "out of range")
    _refused(lib.ktf_aug_workspace_bytes(n, _i32(-2, 0), 2, lens, 1, 16000, 0), "out of range")
    _refused(convolve(ids=_i32(1, 0)), "out of range")
    _refused(mix(ids=_i32(0, 5)), "out of range")
    _refused(mix(a=adds(noise=1)), "out of range")
    _refused(mix(a=adds(noise=-1)), "out of range")
    # o < 0, a non-finite snr_db, fs <= 0
    _refused(mix(a=adds(start=-1)), "< 0")
    _refused(mix(a=adds(snr=float("nan"))), "not finite")
    _refused(mix(a=adds(snr=float("inf"))), "not finite")
    _refused(mix(volume=float("nan")), "not finite")
    for fs in (0, -16000):
        _refused(lib.ktf_aug_rir_spectra_floats(off, 1, fs), "fs")
        _refused(lib.ktf_aug_rir_prepare(buf, off, buf, 1, fs, buf, buf, buf, None), "fs")
        _refused(lib.ktf_aug_workspace_bytes(n, ids, 2, lens, 1, fs, 0), "fs")
        _refused(convolve(fs=fs), "fs")
        _refused(mix(fs=fs), "fs")
    # the bank's and the batch's shapes
    _refused(lib.ktf_aug_rir_spectra_floats(_i32(0, 0), 1, 16000), "no taps")
    _refused(lib.ktf_aug_rir_spectra_floats(_i32(4, 9), 1, 16000), "must be 0")
    _refused(mix(noise_off=(C.c_int64 * 2)(0, 0)), "no samples")
    _refused(mix(add_off=_i32(0, 1, 0)), "descend")
    _refused(convolve(ldx=99), "row stride")
    _refused(mix(T_out=99), "longest output row")
    _refused(mix(ldo=99), "longest output row")
    _refused(convolve(ws_bytes=1024), "workspace")
    _refused(convolve(ws=C.cast(C.addressof(buf) + 4, C.c_void_p)), "aligned")


def test_host_sizes():
    P = ops.aug_partition()
    assert P == 1024
    # spectra: a slot per RIR beyond offsets[R] / P full partitions, then ceil((round(0.001 fs) + round(0.05 fs)) / P) early ones each
    assert ops._size("ktf_aug_rir_spectra_floats", ops._host_ptr(np.array([0, 300, 300 + 3 * P + 5], np.int32)), 2, 16000) == (3 + 2 + 2) * 2 * P
    assert ops._size("ktf_aug_rir_spectra_floats", ops._host_ptr(np.array([0, 10], np.int32)), 1, 48000) == (0 + 1 + 3) * 2 * P
    n, ids, lens = [2 * P + 17, 0, 5], [1, -1, 0], [P + 1, 3 * P + 5]
    S = 3 + 4 + 1
    al = lambda b: (b + 255) & ~255  # noqa: E731
    want = al(3 * S * P * 4) + al(3 * 4 * 2 * P * 4) + al(3 * 3 * S * 8) + al(5 * 8)
    assert ops.aug_workspace_bytes(n, ids, lens, 16000, 5) == want
    assert ops.aug_workspace_bytes(n, [-1, -1, -1], lens, 16000, 0) == al(3 * 5 * P * 4) + al(3 * 3 * 5 * 8)
    assert ops.aug_workspace_bytes([], [], lens, 16000, 0) == 0
    with pytest.raises(ValueError, match="out of range"):
        ops.aug_workspace_bytes(n, [2, 0, 0], lens, 16000, 0)


def test_python_refusals_without_gpu(monkeypatch):
    aug = ktf.augment
    monkeypatch.setattr(L, "require_gpu", lambda: None)
    with pytest.raises(ValueError, match="multi-channel"):
        aug.RirBank([np.zeros((2, 100), np.float32)])
    with pytest.raises(ValueError, match="multi-channel"):
        aug.NoiseBank([np.zeros((100, 2), np.float32)])
    with pytest.raises(ValueError, match="multi-channel"):
        aug.augment(np.zeros((2, 3, 100), np.float32))
    with pytest.raises(ValueError, match="multi-channel"):
        aug.augment([np.zeros((2, 100), np.float32)])
    with pytest.raises(ValueError, match="duration"):
        aug.augment(np.zeros((2, 100), np.float32), duration=3.0)
    with pytest.raises(ValueError, match="sample_rate"):
        aug.augment(np.zeros((2, 100), np.float32), sample_rate=0)

    class Bank:
        sample_rate = 8000
    with pytest.raises(ValueError, match="resampling"):
        aug.augment(np.zeros((2, 100), np.float32), rirs=Bank(), rir_ids=[0, 0])
    with pytest.raises(ValueError, match="resampling"):
        aug.augment(np.zeros((2, 100), np.float32), noises=Bank())
    with pytest.raises(ValueError, match="out_dtype"):
        aug.augment(np.zeros((2, 100), np.float32), out_dtype=torch.float64)


# ----------------------------------------------------------------------------- the ops wrappers' library calls
class _Ptr(C.c_void_p):
    """What the test makes L.ptr return: the pointer, and the tensor it came from."""


class _AugRecorder(Recorder):
    """tests/_recorder.Recorder with the pointer arguments named after the tensors they came from: an argument of the wrapper by
    name, `out[k]` of what it returns, `tmp...` for any other tensor of the wrapper's own, `host` for a host array."""

    def __init__(self, real):
        super().__init__(real, HOST_HELPERS, names=lambda addr: "host", log_host=True)
        self.seen = []          # the tensors of the pointer arguments, in order: a line holds "@k@" until `resolve` names them

    def ptr(self, tensor):
        if tensor is None:
            return None
        p = _Ptr(tensor.data_ptr())
        p.tensor = tensor
        return p

    def arg(self, a):
        if isinstance(a, _Ptr):
            self.seen.append(a.tensor)
            return f"@{len(self.seen) - 1}@"
        return super().arg(a)

    def resolve(self, named, outs):
        def offset(a, b):
            """b is a, or a view into a's memory: -> the byte offset, else None."""
            if a is b:
                return 0
            if a.numel() and b.numel() and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr():
                return b.data_ptr() - a.data_ptr()
            return None

        def name(tensor):
            for tag, cand in list(named.items()) + [(f"out[{i}]", o) for i, o in enumerate(outs)]:
                off = offset(cand, tensor)
                if off is not None:
                    return tag + (f"+{off}" if off else "")
            return f"tmp{list(tensor.shape)}{str(tensor.dtype)[6:]}"
        names = [name(v) for v in self.seen]
        self.lines = [re.sub(r"@(\d+)@", lambda m: names[int(m.group(1))], line) for line in self.lines]


def _flat(res):
    if isinstance(res, (tuple, list)):
        return [o for r in res for o in _flat(r)]
    return [res]


def _show(v):
    if isinstance(v, torch.Tensor):
        return f"{list(v.shape)}{list(v.stride())}{str(v.dtype)[6:]}"
    return repr(v)


def t(*shape, dt=F32):
    return torch.zeros(shape, dtype=dt)


def cases():
    out = []
    add = lambda label, fn, **kw: out.append((label, fn, kw))  # noqa: E731
    P = 1024
    n, ids, lens = np.array([P + 1, 0, 7], np.int32), np.array([1, -1, 0], np.int32), np.array([5, 2 * P], np.int32)
    off = np.array([0, 5, 5 + 2 * P], np.int32)
    add("aug_partition", "aug_partition")
    add("aug_tables", "aug_tables", device="cpu")
    add("aug_rir_prepare", "aug_rir_prepare", h=t(5 + 2 * P), offsets=off, offsets_dev=t(3, dt=I32), fs=16000, tables=t(4096))
    add("aug_rir_prepare_8k", "aug_rir_prepare", h=t(5 + 2 * P), offsets=off, offsets_dev=t(3, dt=I32), fs=8000, tables=t(4096))
    add("aug_workspace_bytes", "aug_workspace_bytes", n=n, rir_ids=ids, rir_lengths=lens, fs=16000, num_additives=3)
    add("aug_workspace_bytes_no_rows", "aug_workspace_bytes", n=n[:0], rir_ids=ids[:0], rir_lengths=lens, fs=16000, num_additives=0)
    bank = dict(h=t(5 + 2 * P), offsets_dev=t(3, dt=I32), meta=t(2, 8, dt=I32), spectra=t(7 * 2 * P), tables=t(4096))
    none = dict(h=None, offsets_dev=None, meta=None, spectra=None, tables=None)
    for tag, x in (("f32", t(3, P + 1)), ("i16", t(3, P + 1, dt=I16)), ("strided", torch.zeros((3, P + 9))[:, 2:P + 3])):
        add(f"aug_convolve_{tag}", "aug_convolve", x=x, n=n, n_dev=t(3, dt=I32), rir_ids=ids, rir_ids_dev=t(3, dt=I32), rir_lengths=lens,
            fs=16000, **bank, num_additives=3, stats=t(3, 4, dt=F64), workspace=t(1 << 16, dt=U8))
    add("aug_convolve_no_rir", "aug_convolve", x=t(3, P + 1), n=n, n_dev=t(3, dt=I32), rir_ids=np.full(3, -1, np.int32),
        rir_ids_dev=t(3, dt=I32), rir_lengths=lens[:0], fs=16000, **none, num_additives=0, stats=t(3, 4, dt=F64), workspace=t(1 << 16, dt=U8))
    adds = np.array([[0, 0, 0, 0], [1, 0, 5, 100], [0, 0, 9, 0]], np.int32)
    rows = dict(n=n, n_dev=t(3, dt=I32), rir_ids=ids, rir_ids_dev=t(3, dt=I32), rir_lengths=lens, fs=16000, meta=t(2, 8, dt=I32))
    mixed = dict(add_offsets=np.array([0, 2, 2, 3], np.int32), add_offsets_dev=t(4, dt=I32), adds=adds, adds_dev=t(3, 4, dt=I32), noise=t(50),
                 noise_offsets=np.array([0, 20, 50], np.int64), noise_offsets_dev=t(3, dt=torch.int64))
    clean = dict(add_offsets=np.zeros(4, np.int32), add_offsets_dev=t(4, dt=I32), adds=adds[:0], adds_dev=t(0, 4, dt=I32), noise=None,
                 noise_offsets=np.zeros(1, np.int64), noise_offsets_dev=None)
    for tag, o, shift in (("f32", t(3, P + 1), True), ("i16", t(3, P + 1, dt=I16), True), ("unshifted", t(3, 3 * P), False),
                          ("strided", torch.zeros((3, P + 9))[:, 2:P + 3], True)):
        add(f"aug_mix_{tag}", "aug_mix", **rows, **mixed, shift_output=shift, normalize_output=True, volume=0.0, out=o, stats=t(3, 4, dt=F64),
            workspace=t(1 << 16, dt=U8))
    add("aug_mix_no_additives_volume", "aug_mix", **rows, **clean, shift_output=True, normalize_output=False, volume=0.5, out=t(3, P + 1),
        stats=t(3, 4, dt=F64), workspace=t(1 << 16, dt=U8))
    return out


def _shown(v):
    return f"np{list(v.shape)}{v.dtype}" if isinstance(v, np.ndarray) else _show(v)


def run_case(monkeypatch, case):
    label, fn, kw = case
    rec = _AugRecorder(L.load())
    named = {k: v for k, v in kw.items() if isinstance(v, torch.Tensor)}
    with monkeypatch.context() as m:
        m.setattr(L, "_lib", rec)
        m.setattr(L, "load", lambda: rec)
        m.setattr(L, "require_gpu", lambda: None)
        m.setattr(L, "stream_ptr", lambda: STREAM)
        m.setattr(L, "on_device", lambda device: contextlib.nullcontext())
        m.setattr(L, "ptr", rec.ptr)
        res = getattr(ops, fn)(**kw)
    outs = _flat(res)
    rec.resolve(named, [o for o in outs if isinstance(o, torch.Tensor)])
    k, shown = 0, []
    for o in outs:
        if isinstance(o, torch.Tensor):
            given = next((tag for tag, cand in named.items() if cand is o), None)
            shown.append(f"{given or f'out[{k}]'}={_show(o)}")
            k += 1
        else:
            shown.append(repr(o))
    head = f"== {label}: {fn}({', '.join(f'{k}={_shown(v)}' for k, v in kw.items())})"
    return [head] + rec.lines + ["-> " + ", ".join(shown)], rec.called


def record(monkeypatch):
    lines, called = [], set()
    for case in cases():
        ls, c = run_case(monkeypatch, case)
        lines += ls
        called |= c
    return lines, called


def test_ops_calls_match_golden(monkeypatch):
    lines, called = record(monkeypatch)
    assert called == set(L.AUGMENT_PROTOTYPES), called ^ set(L.AUGMENT_PROTOTYPES)
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    if lines != want:
        diff = list(difflib.unified_diff(want, lines, "golden", "ops", lineterm="", n=2))
        raise AssertionError("the augmentation wrappers' library calls changed:\n" + "\n".join(diff[:80]))


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit(__doc__)
    mp = pytest.MonkeyPatch()
    try:
        lines, called = record(mp)
    finally:
        mp.undo()
    if called != set(L.AUGMENT_PROTOTYPES):
        sys.exit(f"the cases do not reach {sorted(set(L.AUGMENT_PROTOTYPES) - called)}")
    with open(GOLDEN, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{GOLDEN}: {len(lines)} lines, {len(cases())} cases")
