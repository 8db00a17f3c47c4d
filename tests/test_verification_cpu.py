"""CPU half of speaker verification (ktf.verification, the count-aware PLDA entry points): the NumPy restatement against an
independent Gaussian derivation and against the oracle at n = 1, EER and minDCF on hand-worked lists, the Kaldi text parsers,
and the argument checks every new C entry point makes before it launches anything."""

import ctypes as C

import numpy as np
import pytest
from scipy.stats import norm

import _golden as G
import _verif_ref as V
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L
from oracle import ktf_oracle as O

ver = ktf.verification


def _model(D, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(D) * 0.1, rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D), rng.uniform(0.05, 20.0, D)


def test_llr_matches_explicit_gaussian_log_densities():
    rng = np.random.default_rng(1)
    D, N, M = 12, 5, 7
    psi = rng.uniform(0.1, 10.0, D)
    y, e = rng.standard_normal((N, D)), rng.standard_normal((M, D))
    n = np.array([1, 2, 3, 5, 10, 50, 1.5])
    got = V.llr(y, e, psi, n)
    for i in range(N):
        for j in range(M):
            # class mean posterior after n examples with mean e: N(n psi e / (n psi + 1), psi / (n psi + 1)); a new example adds the
            # unit within-class variance. Without the class: N(0, psi + 1).
            m, v = n[j] * psi * e[j] / (n[j] * psi + 1), psi / (n[j] * psi + 1) + 1.0
            want = norm.logpdf(y[i], m, np.sqrt(v)).sum() - norm.logpdf(y[i], 0.0, np.sqrt(psi + 1.0)).sum()
            assert abs(got[i, j] - want) < 1e-10 * max(1.0, abs(want))


def test_restatement_at_one_example_is_the_oracle():
    z = G.load("plda.npz")
    p = ktf.io.KaldiPldaReader(G.GOLDEN + "/plda.bin", True)
    x = z["plda_input"][:, 0, :]
    s, y = O.plda(x, p.mean, p.transformMat, p.psi)
    tr = V.transform(x, p.mean, p.transformMat, p.psi, 1.0)
    assert np.abs(tr - y[:, :, 0]).max() < 1e-9
    assert np.abs(V.llr(tr, tr, p.psi, 1.0) - s).max() < 1e-7 * np.abs(s).max()


def test_restatement_counts_change_transform_and_scores():
    mean, T, psi = _model(16, 3)
    x = np.random.default_rng(4).standard_normal((4, 16))
    assert not np.allclose(V.transform(x, mean, T, psi, 3.0), V.transform(x, mean, T, psi, 1.0))
    assert np.allclose(V.transform(x, mean, T, psi, 3.0, simple_length_norm=True), V.transform(x, mean, T, psi, 1.0, simple_length_norm=True))
    tr = V.transform(x, mean, T, psi)
    assert not np.allclose(V.llr(tr, tr, psi, 4.0), V.llr(tr, tr, psi, 1.0))


def test_ivector_mean_restatement():
    raw = np.random.default_rng(2).standard_normal((6, 5)).astype(np.float32)
    m, n = V.ivector_mean(raw, [[0, 2], [5], [1, 1, 3]])
    assert n.tolist() == [2, 1, 3]
    assert np.array_equal(m[1], raw[5])
    assert np.array_equal(m[0], ((raw[0].astype(np.float64) + raw[2]) / 2).astype(np.float32))


# ----------------------------------------------------------------------------- EER and minDCF
def test_eer_hand_worked():
    assert ver.eer([3, 4, 1, 2], [1, 1, 0, 0]) == 0.0              # separated
    assert ver.eer([1, 2, 3, 4], [1, 1, 0, 0]) == 1.0              # reversed: every target below every non-target
    assert ver.eer([1, 3, 2, 4], [1, 1, 0, 0]) == 0.5              # crossing at one miss and one false alarm
    assert ver.eer([2, 2], [1, 0]) == 1.0                          # a tie is an error (the test is strict)
    assert ver.eer([1, 2, 3, 4, 0.5], [1, 1, 1, 1, 0]) == 0.0       # one non-target below all four targets
    assert ver.eer([5, 1, 2, 3, 4], [1, 0, 0, 0, 0]) == 0.0
    assert ver.eer([0, 1, 2, 3, 4], [1, 0, 0, 0, 0]) == 1.0
    for s, l in [([1, 2], [1, 1]), ([1, 2], [0, 0]), ([], [])]:
        with pytest.raises(ValueError):
            ver.eer(s, l)


def test_min_dcf_hand_worked():
    # separated: a threshold with neither misses nor false alarms exists
    assert ver.min_dcf([1, 2, 3, 4], [0, 0, 1, 1], 0.01) == 0.0
    # targets 1, 3; non-targets 2, 4 (p = 0.5): at position 0 P_miss 1/2, P_fa 1 -> 0.75; at 1: 1/2, 1/2 -> 0.5; at 2: 1, 1/2 -> 0.75;
    # at 3: 1, 0 -> 0.5. min 0.5 / min(0.5, 0.5) = 1.0
    assert ver.min_dcf([1, 3, 2, 4], [1, 1, 0, 0], 0.5) == pytest.approx(1.0)
    # ties keep the list order (stable sort): the same scores, the labels of the tied pair swapped, give another value
    a = ver.min_dcf([1, 2, 2, 3], [0, 1, 0, 1], 0.5)
    b = ver.min_dcf([1, 2, 2, 3], [0, 0, 1, 1], 0.5)
    assert a == pytest.approx(V.min_dcf([1, 2, 2, 3], [0, 1, 0, 1], 0.5)) and b == 0.0 and a > 0
    assert ver.min_dcf([1, 3, 2, 4], [1, 1, 0, 0], 0.05, c_miss=10, c_fa=1) == pytest.approx(
        V.min_dcf([1, 3, 2, 4], [1, 1, 0, 0], 0.05, c_miss=10, c_fa=1))
    for s, l in [([1, 2], [1, 1]), ([1, 2], [0, 0])]:
        with pytest.raises(ValueError):
            ver.min_dcf(s, l, 0.01)
    with pytest.raises(ValueError):
        ver.min_dcf([1, 2], [0, 1], 1.0)


@pytest.mark.parametrize("seed", range(6))
def test_eer_and_min_dcf_match_restatement_on_random_lists(seed):
    rng = np.random.default_rng(seed)
    nt, nn = int(rng.integers(1, 50)), int(rng.integers(1, 300))
    s = np.concatenate([rng.normal(2, 1, nt), rng.normal(0, 1, nn)]).round(1)        # rounded: ties
    lab = np.concatenate([np.ones(nt, bool), np.zeros(nn, bool)])
    perm = rng.permutation(nt + nn)
    s, lab = s[perm], lab[perm]
    assert ver.eer(s, lab) == V.eer(s, lab)
    for p in (0.01, 0.001, 0.5):
        assert ver.min_dcf(s, lab, p) == pytest.approx(V.min_dcf(s, lab, p), rel=1e-12, abs=1e-12)


# ----------------------------------------------------------------------------- parsers
def test_parsers(tmp_path):
    p = tmp_path / "spk2utt"
    p.write_text("spkA a1 a2 a3\n\nspkB b1\n")
    assert ver.read_spk2utt(str(p)) == [("spkA", ["a1", "a2", "a3"]), ("spkB", ["b1"])]
    p.write_text("spkA a1\nspkB\n")
    with pytest.raises(ValueError, match="without utterances"):
        ver.read_spk2utt(str(p))
    t = tmp_path / "trials"
    t.write_text("spkA u1 target\nspkB u1 nontarget\n  \nspkA u2 nontarget\n")
    m, te, lab = ver.read_trials(str(t))
    assert m == ["spkA", "spkB", "spkA"] and te == ["u1", "u1", "u2"] and lab.tolist() == [True, False, False]
    t.write_text("spkA u1\nspkB u2\n")
    assert ver.read_trials(str(t))[2] is None
    for bad in ("spkA u1 maybe\n", "spkA\n", "spkA u1 target\nspkB u2\n"):
        t.write_text(bad)
        with pytest.raises(ValueError):
            ver.read_trials(str(t))


# ----------------------------------------------------------------------------- C-ABI argument checks (before any launch)
def test_spk_mean_abi_argument_validation_without_gpu():
    lib = L.load()
    f = (C.c_float * 64)()
    i = (C.c_int32 * 8)()

    def call(raw=f, U=4, D=8, off=i, S=2, utts=i, n=3, means=f, nu=i):
        return lib.ktf_spk_mean_f32(raw, U, D, off, S, utts, n, means, nu, None)

    for kw, msg in [({"raw": None}, "null"), ({"off": None}, "null"), ({"utts": None}, "null"), ({"means": None}, "null"),
                    ({"nu": None}, "null"), ({"U": 0}, "bad sizes"), ({"D": 0}, "bad sizes"), ({"S": -1}, "bad sizes"),
                    ({"n": -1}, "bad sizes"), ({"S": 1 << 31}, "too many speakers")]:
        assert call(**kw) == -1, kw
        assert msg in L.last_error(), (kw, L.last_error())
    assert call(S=0) == 0                                    # nothing to do: no launch


@pytest.mark.parametrize("bits", [64, 32])
def test_plda_n_abi_argument_validation_without_gpu(bits):
    lib = L.load()
    sfx = "f64" if bits == 64 else "f32"
    b = ((C.c_double if bits == 64 else C.c_float) * 64)()
    tr = getattr(lib, "ktf_plda_transform_n_" + sfx)
    for kw, msg in [({"x": None}, "null"), ({"cnt": None}, "null"), ({"out": None}, "null"), ({"B": -1}, "bad sizes"),
                    ({"dim": 0}, "bad sizes"), ({"dim": 8192}, "too large")]:
        a = {"x": b, "B": 2, "dim": 4, "cnt": b, "out": b}
        a.update(kw)
        assert tr(a["x"], a["B"], a["dim"], b, b, b, a["cnt"], 1, 0, a["out"], None) == -1, kw
        assert msg in L.last_error(), (kw, L.last_error())
    assert tr(b, 0, 4, b, b, b, b, 1, 0, b, None) == 0
    sc = getattr(lib, "ktf_plda_score_n_" + sfx)
    for kw, msg in [({"t": None}, "null"), ({"cnt": None}, "null"), ({"s": None}, "null"), ({"N": -1}, "bad sizes"),
                    ({"M": -1}, "bad sizes"), ({"dim": 0}, "bad sizes"), ({"N": 64 * 65536}, "too many rows")]:
        a = {"t": b, "N": 2, "M": 3, "dim": 4, "cnt": b, "s": b}
        a.update(kw)
        assert sc(a["t"], a["N"], b, a["M"], a["dim"], b, a["cnt"], a["s"], None) == -1, kw
        assert msg in L.last_error(), (kw, L.last_error())
    assert sc(b, 0, b, 3, 4, b, b, b, None) == 0
    trials = getattr(lib, "ktf_plda_trials_" + sfx)
    pairs = (C.c_int32 * 8)()
    need = lib.ktf_plda_trials_workspace_bytes(2, 3, 4, bits // 8)
    assert need == bits // 8 * (2 * 3 * 4 + 3 + 2)
    assert lib.ktf_plda_trials_workspace_bytes(2, 3, 4, 2) == -1 and lib.ktf_plda_trials_workspace_bytes(-1, 3, 4, 8) == -1
    for kw, msg in [({"psi": None}, "null"), ({"pairs": None}, "null"), ({"s": None}, "null"), ({"t": None}, "null"),
                    ({"cnt": None}, "null"), ({"ws": None}, "null"), ({"T": -1}, "bad sizes"), ({"dim": 0}, "bad sizes"),
                    ({"N": 0}, "trials against"), ({"M": 0}, "trials against"), ({"M": 1 << 31}, "below 2^31"),
                    ({"wsb": need - 1}, "workspace of")]:
        a = {"t": b, "N": 2, "M": 3, "dim": 4, "psi": b, "cnt": b, "pairs": pairs, "T": 4, "s": b, "ws": b, "wsb": need}
        a.update(kw)
        assert trials(a["t"], a["N"], b, a["M"], a["dim"], a["psi"], a["cnt"], a["pairs"], a["T"], a["s"], a["ws"], a["wsb"], None) == -1, kw
        assert msg in L.last_error(), (kw, L.last_error())
    assert trials(None, 0, None, 0, 4, None, None, None, 0, None, None, 0, None) == 0       # T = 0: nothing to score
