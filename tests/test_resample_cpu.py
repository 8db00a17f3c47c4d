"""Sample-rate conversion without a GPU: the fp64 restatement (tests/_resample_ref.py) against pinned lengths, plan shapes and
signals, the library's host plan against it, the C-ABI of include/ktf_resample.h (symbols, argument checks before any launch), the
Python refusals, and the ops.rs_* wrappers' library calls, pinned in tests/golden/resample_calls.txt in the manner of
test_augment_cpu.py (on tests/_recorder.Recorder).

    python tests/test_resample_cpu.py --write      # regenerate the golden file (only for a deliberate change of behaviour)
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
import _resample_ref as R  # noqa: E402
from _recorder import STREAM, Recorder  # noqa: E402
from test_augment_cpu import _AugRecorder, _flat, _show, _shown  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "resample_calls.txt")
HOST_HELPERS = re.compile(r"ktf_rs_(tile|plan_sizes|plan|num_out)")
F32, I32, I16 = torch.float32, torch.int32, torch.int16

# fi, fo, m for n = 1000, m for n = 1 (rule 3)
LENGTHS = [(16000, 8000, 500, 1), (8000, 16000, 2000, 2), (44100, 16000, 363, 1), (48000, 8000, 167, 1), (17600, 16000, 910, 1),
           (16000, 17600, 1100, 2), (14400, 16000, 1112, 2), (22050, 16000, 726, 1)]
# fi, fo, iu, ou, min taps, max taps, first[0] (rules 1 and 2, default cutoff, 6 zeros)
SHAPES = [(16000, 8000, 2, 1, 25, 25, -12), (8000, 16000, 1, 2, 12, 13, -6), (44100, 16000, 441, 160, 33, 34, -16),
          (48000, 8000, 6, 1, 73, 73, -36), (17600, 16000, 11, 10, 13, 14, -6), (22050, 16000, 441, 320, 16, 17, -8)]
PAIRS = sorted({(fi, fo) for fi, fo, *_ in LENGTHS})


# ----------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("fi,fo,m1000,m1", LENGTHS)
def test_lengths(fi, fo, m1000, m1, monkeypatch):
    assert (R.num_out(1000, fi, fo), R.num_out(1, fi, fo), R.num_out(0, fi, fo)) == (m1000, m1, 0)
    lib = L.load()
    assert (lib.ktf_rs_num_out(1000, fi, fo), lib.ktf_rs_num_out(1, fi, fo), lib.ktf_rs_num_out(0, fi, fo)) == (m1000, m1, 0)
    monkeypatch.setattr(L, "require_gpu", lambda: None)
    rs = ktf.augment.Resampler(fi, fo)
    assert (rs.num_out(1000), rs.num_out(1), rs.num_out(0)) == (m1000, m1, 0)
    for n in (2, 3, 160, 441, 999, 16000, 1 << 30):
        assert lib.ktf_rs_num_out(n, fi, fo) == R.num_out(n, fi, fo)


@pytest.mark.parametrize("fi,fo,iu,ou,tmin,tmax,first0", SHAPES)
def test_plan_shape(fi, fo, iu, ou, tmin, tmax, first0):
    got = R.plan(fi, fo)
    assert (got[0], got[1], min(got[3]), max(got[3]), got[2][0]) == (iu, ou, tmin, tmax, first0)
    liu, lou, first, taps, w = ops.rs_plan(fi, fo, R.default_cutoff(fi, fo), 6)
    assert (liu, lou, int(taps.min()), int(taps.max()), int(first[0])) == (iu, ou, tmin, tmax, first0)
    assert w.shape == (ou, tmax) and w.dtype == np.float32


def _oracle(x, fi, fo):
    iu, ou, first, taps, w = R.plan(fi, fo)
    w32 = [r.astype(np.float32) for r in w]
    m = R.num_out(len(x), fi, fo)
    return R.resample64(x, first, taps, w32, iu, ou, m)[0]


def test_oracle_is_a_resampler():
    n, fi, fo = 4000, 16000, 8000
    t = np.arange(n) / fi
    y = _oracle((1000 * np.sin(2 * np.pi * 440 * t)).astype(np.float32), fi, fo)
    want = 1000 * np.sin(2 * np.pi * 440 * np.arange(y.size) / fo)
    assert y.size == 2000
    err = np.abs(y - want)[50:-50].max()
    print(f"440 Hz sine 16 kHz -> 8 kHz: max error {err:.3f} of amplitude 1000 (bound 1.0; 0.277 when written)")
    assert err <= 1e-3 * 1000
    # DC passes with the filter's gain, sum(w) = 1.00046: within 1e-3 of the level
    dc = _oracle(np.full(n, 1000, np.float32), fi, fo)
    assert np.abs(dc[50:-50] - 1000).max() <= 1e-3 * 1000
    # 6 kHz lies above the new Nyquist frequency (4 kHz) and past the window's transition band: the oracle leaves 1.82 of 1000,
    # 54.8 dB down; asserted with a 4.8 dB margin
    tone = _oracle((1000 * np.sin(2 * np.pi * 6000 * t)).astype(np.float32), fi, fo)
    db = 20 * np.log10(1000 / np.abs(tone[50:-50]).max())
    print(f"6 kHz tone: {db:.1f} dB down (bound 50)")
    assert db >= 50.0
    # and up: 8 kHz -> 16 kHz keeps the sine
    up = _oracle((1000 * np.sin(2 * np.pi * 440 * np.arange(2000) / 8000)).astype(np.float32), 8000, 16000)
    assert up.size == 4000
    assert np.abs(up - 1000 * np.sin(2 * np.pi * 440 * np.arange(4000) / 16000))[50:-50].max() <= 1.0


@pytest.mark.parametrize("fi,fo", PAIRS)
def test_library_table_against_the_oracle(fi, fo):
    iu, ou, first, taps, w64 = R.plan(fi, fo)
    liu, lou, lfirst, ltaps, w32 = ops.rs_plan(fi, fo, R.default_cutoff(fi, fo), 6)
    assert (liu, lou) == (iu, ou)
    for i in range(ou):
        assert not w32[i, ltaps[i]:].any()                      # zero-padded
    lo = min(min(first), int(lfirst.min()))
    width = max(max(f + t for f, t in zip(first, taps)), int((lfirst + ltaps).max())) - lo

    def scatter(fs, ts, ws):
        out = np.zeros((ou, width), np.float64)
        for i in range(ou):
            out[i, fs[i] - lo:fs[i] - lo + ts[i]] = np.asarray(ws[i], np.float64)[:ts[i]]
        return out
    want, got = scatter(first, taps, w64), scatter(lfirst, ltaps, w32)
    bound = 2.0 ** -24 * np.abs(want) + 2.0 ** -50
    worst = float((np.abs(got - want) / bound).max())
    print(f"{fi} -> {fo}: worst |w32 - w64| / bound = {worst:.3f}")
    assert (np.abs(got - want) <= bound).all()
    assert np.abs(want).max() <= 1.0


def test_plan_is_scale_invariant():
    a = ops.rs_plan(11, 10, 0.99 * 0.5 * 10, 6)
    b = ops.rs_plan(17600, 16000, 0.99 * 0.5 * 16000, 6)
    assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert np.abs(a[4].astype(np.float64) - b[4]).max() <= 2.0 ** -23 * np.abs(b[4]).max()


# ----------------------------------------------------------------------------- the C-ABI
def test_header_symbols_are_the_resample_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_resample.h")).read()
    declared = set(re.findall(r"\b(ktf_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.RESAMPLE_PROTOTYPES), declared ^ set(L.RESAMPLE_PROTOTYPES)
    lib = L.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert not set(L.RESAMPLE_PROTOTYPES) & (set(L.PROTOTYPES) | set(L.AUGMENT_PROTOTYPES))
    for other in ("ktf_hip.h", "ktf_augment.h"):
        assert "ktf_rs_" not in open(os.path.join(ROOT, "include", other)).read()
    assert lib.ktf_rs_tile() == ops.rs_tile() > 0


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
    o = _i32(0, 0, 0)
    at = lambda k: C.c_void_p(C.addressof(o) + 4 * k)  # noqa: E731
    sizes = lambda fi, fo, cutoff=3960.0, zeros=6: lib.ktf_rs_plan_sizes(fi, fo, cutoff, zeros, at(0), at(1), at(2))  # noqa: E731
    plan = lambda fi, fo, cutoff=3960.0, zeros=6, ldw=64: lib.ktf_rs_plan(fi, fo, cutoff, zeros, buf, buf, buf, ldw)  # noqa: E731
    for fn in (sizes, plan):
        _refused(fn(0, 8000), "positive")
        _refused(fn(16000, -8000), "positive")
        _refused(fn(8000, 8000), "equal rates")
        _refused(fn(16000, 8000, cutoff=0.0), "cutoff")
        _refused(fn(16000, 8000, cutoff=-1.0), "cutoff")
        _refused(fn(16000, 8000, cutoff=4000.5), "cutoff")
        _refused(fn(16000, 8000, cutoff=float("nan")), "cutoff")
        _refused(fn(16000, 8000, zeros=0), "zeros")
        _refused(fn(16000, 8000, zeros=200), "taps")                       # 801 taps
        _refused(fn(16000, 15999, cutoff=7900.0), "table")                 # 15999 phases of 13 taps
        _refused(fn(16000, 1000, cutoff=495.0), "spans")                   # 16 input samples per output: a tile spans 16 k
    assert sizes(44100, 16000, 7920.0) == 0 and list(o) == [160, 441, 34] and 160 * 34 <= 1 << 16
    assert sizes(48000, 8000) == 0 and list(o) == [1, 6, 73]
    _refused(lib.ktf_rs_plan_sizes(16000, 8000, 3960.0, 6, None, o, o), "null")
    _refused(lib.ktf_rs_plan(16000, 8000, 3960.0, 6, None, buf, buf, 64), "null")
    _refused(plan(16000, 8000, ldw=24), "ldw")
    _refused(lib.ktf_rs_num_out(-1, 16000, 8000), "samples")
    _refused(lib.ktf_rs_num_out((1 << 30) + 1, 16000, 8000), "samples")
    _refused(lib.ktf_rs_num_out(10, 0, 8000), "positive")

    first, taps, n = _i32(-12), _i32(25), _i32(100, 50)

    def run(x=buf, ldx=100, n=n, n_dev=buf, B=2, iu=2, ou=1, first=first, taps=taps, first_dev=buf, taps_dev=buf, w_dev=buf, ldw=25, out=buf,
            ldo=50, T_out=50):
        return lib.ktf_rs_resample(x, 0, ldx, n, n_dev, B, iu, ou, first, taps, first_dev, taps_dev, w_dev, ldw, out, 0, ldo, T_out, None)

    _refused(run(x=None), "null")
    _refused(run(n=None), "null")
    _refused(run(n_dev=None), "null")
    _refused(run(first=None), "null")
    _refused(run(w_dev=None), "null")
    _refused(run(out=None), "null")
    _refused(run(B=-1), "negative size")
    _refused(run(ldx=-1), "negative size")
    _refused(run(T_out=-1), "negative size")
    _refused(run(n=_i32(100, -5)), "negative size")
    _refused(run(iu=1, ou=1), "units")
    _refused(run(iu=0), "units")
    _refused(run(taps=_i32(0)), "taps")
    _refused(run(taps=_i32(257), ldw=257), "taps")
    _refused(run(ldw=24), "ldw")
    _refused(run(iu=16, ou=1), "spans")
    _refused(run(ldx=99), "row stride")
    _refused(run(T_out=49), "longest output row")
    _refused(run(ldo=49), "longest output row")
    _refused(run(n=_i32((1 << 30) + 1, 50), ldx=1 << 31, T_out=1 << 30, ldo=1 << 30), "2^30")
    _refused(run(iu=1, ou=2, n=_i32(1 << 30, 50), ldx=1 << 30, T_out=1 << 31, ldo=1 << 31, first=_i32(-6, -6), taps=_i32(13, 13)), "2^30")
    _refused(run(B=65536, n=_i32(*([1] * 65536))), "65535")


def test_python_refusals_without_gpu(monkeypatch):
    aug = ktf.augment
    monkeypatch.setattr(L, "require_gpu", lambda: None)
    for bad in (0, -8000, 8000.0, "8000", None, True):
        with pytest.raises(ValueError, match="positive int"):
            aug.Resampler(16000, bad)
        with pytest.raises(ValueError, match="positive int"):
            aug.resample(np.zeros((2, 100), np.float32), bad, 16000)
    with pytest.raises(ValueError, match="equal rates"):
        aug.Resampler(8000, 8000)
    for cutoff in (0, -1.0, 4000.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="lowpass_cutoff"):
            aug.Resampler(16000, 8000, lowpass_cutoff=cutoff)
    for zeros in (0, -3, 2.5):
        with pytest.raises(ValueError, match="num_zeros"):
            aug.Resampler(16000, 8000, num_zeros=zeros)
    with pytest.raises(ValueError, match="taps"):
        aug.Resampler(16000, 8000, num_zeros=200)
    with pytest.raises(ValueError, match="table"):
        aug.Resampler(16000, 15999)
    rs = aug.Resampler(16000, 8000)
    assert (rs.iu, rs.ou, rs.taps.tolist(), rs.first.tolist()) == (2, 1, [25], [-12]) and rs.cutoff == 0.99 * 0.5 * 8000
    with pytest.raises(ValueError, match="multi-channel"):
        rs(np.zeros((2, 3, 100), np.float32))
    with pytest.raises(ValueError, match="multi-channel"):
        rs([np.zeros((2, 100), np.float32)])
    with pytest.raises(ValueError, match="out_dtype"):
        rs(np.zeros((2, 100), np.float32), out_dtype=torch.float64)
    with pytest.raises(ValueError, match="samples"):
        rs.num_out((1 << 30) + 1)
    # speed perturbation plans p -> q for factor = p / q
    assert aug.speed_rates(1.1) == (11, 10) and aug.speed_rates(0.9) == (9, 10) and aug.speed_rates("1.05") == (21, 20)
    for bad in (0, -1.1, "fast", float("nan")):
        with pytest.raises(ValueError, match="factor"):
            aug.speed_rates(bad)
    planned = []

    class Spy(aug.Resampler):
        def __call__(self, wavs, lengths=None, out_dtype=None):
            planned.append((self.orig_rate, self.new_rate, self.iu, self.ou))
            return wavs, lengths

    monkeypatch.setattr(aug, "Resampler", Spy)
    x = torch.zeros((2, 100))
    aug.speed_perturb(x, 1.1)
    aug.speed_perturb(x, 0.9)
    aug.resample(x, 44100, 16000)
    assert planned == [(11, 10, 11, 10), (9, 10, 9, 10), (44100, 16000, 441, 160)]
    # equal rates: the input, unfiltered
    out, lens = aug.resample(x, 16000, 16000, lengths=[100, 40])
    assert out is x and lens == [100, 40]
    out, lens = aug.speed_perturb(x, 1.0)
    assert out is x and lens == [100, 100] and len(planned) == 3
    with pytest.raises(ValueError, match="lengths"):
        aug.resample(x, 16000, 16000, lengths=[100, 101])
    with pytest.raises(ValueError, match="out_dtype"):
        aug.resample(x, 16000, 16000, out_dtype=torch.int16)


# ----------------------------------------------------------------------------- the ops wrappers' library calls
def t(*shape, dt=F32):
    return torch.zeros(shape, dtype=dt)


def cases():
    out = []
    add = lambda label, fn, **kw: out.append((label, fn, kw))  # noqa: E731
    add("rs_tile", "rs_tile")
    add("rs_plan", "rs_plan", fi=16000, fo=8000, cutoff=3960.0, zeros=6)
    add("rs_plan_441_160", "rs_plan", fi=44100, fo=16000, cutoff=7920.0, zeros=6)
    add("rs_num_out", "rs_num_out", n=1000, fi=44100, fo=16000)
    n = np.array([100, 0, 7], np.int32)
    plan = dict(iu=2, ou=1, first=np.array([-12], np.int32), taps=np.array([25], np.int32), first_dev=t(1, dt=I32), taps_dev=t(1, dt=I32),
                w_dev=t(1, 25))
    for tag, x, o in (("f32", t(3, 100), t(3, 50)), ("i16", t(3, 100, dt=I16), t(3, 50, dt=I16)), ("i16_to_f32", t(3, 100, dt=I16), t(3, 50)),
                      ("strided", torch.zeros((3, 109))[:, 2:102], torch.zeros((3, 64))[:, 1:51])):
        add(f"rs_resample_{tag}", "rs_resample", x=x, n=n, n_dev=t(3, dt=I32), **plan, out=o)
    add("rs_resample_no_rows", "rs_resample", x=t(0, 100), n=n[:0], n_dev=t(0, dt=I32), **plan, out=t(0, 0))
    return out


def run_case(monkeypatch, case):
    label, fn, kw = case
    rec = _AugRecorder(L.load())
    rec.host_helpers = HOST_HELPERS
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
            shown.append(_shown(o) if isinstance(o, np.ndarray) else repr(o))
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
    assert called == set(L.RESAMPLE_PROTOTYPES), called ^ set(L.RESAMPLE_PROTOTYPES)
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    if lines != want:
        diff = list(difflib.unified_diff(want, lines, "golden", "ops", lineterm="", n=2))
        raise AssertionError("the resampling wrappers' library calls changed:\n" + "\n".join(diff[:80]))


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit(__doc__)
    mp = pytest.MonkeyPatch()
    try:
        lines, called = record(mp)
    finally:
        mp.undo()
    if called != set(L.RESAMPLE_PROTOTYPES):
        sys.exit(f"the cases do not reach {sorted(set(L.RESAMPLE_PROTOTYPES) - called)}")
    with open(GOLDEN, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{GOLDEN}: {len(lines)} lines, {len(cases())} cases")
