"""Score normalisation without a GPU: the NumPy restatement against a hand-worked row, verification.as_norm on host tensors against
the per-trial loop, argument checks, and the new entry points' prototypes and host-side validation."""

import ctypes as C

import numpy as np
import pytest
import torch

import _snorm_ref as S
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L

ver = ktf.verification
NEW = ["ktf_topn_stats_f64", "ktf_topn_stats_f32", "ktf_plda_cohort_workspace_bytes", "ktf_plda_cohort_stats_f64",
       "ktf_plda_cohort_stats_f32"]


def test_restatement_hand_worked_row():
    row = np.array([[3.0, 5.0, 1.0, 3.0, 3.0]])
    m, s = S.topn_stats(row, 3)                                    # 5, 3, 3
    assert m[0] == pytest.approx(11.0 / 3.0, abs=1e-15) and s[0] == pytest.approx(np.sqrt(8.0 / 9.0), abs=1e-15)
    m, s = S.topn_stats(row, 2)                                    # 5, 3
    assert m[0] == 4.0 and s[0] == 1.0
    m, s = S.topn_stats(row, None)
    assert m[0] == 3.0 and s[0] == pytest.approx(np.sqrt(1.6), abs=1e-15)
    m2, s2 = S.topn_stats(row, 9)
    assert m2[0] == m[0] and s2[0] == s[0]
    m, s = S.topn_stats(row[:, [0, 3, 4]], 2)                      # all tied
    assert m[0] == 3.0 and s[0] == 0.0


def _case(seed=0, T=200, M=17, N=23):
    rng = np.random.default_rng(seed)
    scores = rng.standard_normal(T) * 20.0
    je, it = rng.integers(0, M, T), rng.integers(0, N, T)
    es = (rng.standard_normal(M) * 5.0, rng.uniform(0.5, 3.0, M))
    ts = (rng.standard_normal(N) * 5.0, rng.uniform(0.5, 3.0, N))
    return scores, je, it, es, ts


@pytest.mark.parametrize("sides", ["both", "enroll", "test"])
def test_as_norm_on_host_tensors_matches_loop(sides):
    scores, je, it, es, ts = _case()
    e = es if sides != "test" else None
    t = ts if sides != "enroll" else None
    want = S.as_norm(scores, je, it, e, t)
    tt = lambda p: None if p is None else tuple(torch.as_tensor(a) for a in p)  # noqa: E731
    for sc in (torch.as_tensor(scores), torch.as_tensor(scores.astype(np.float32))):
        for idx in ((je, it), (torch.as_tensor(je), torch.as_tensor(it)), (je.tolist(), it.astype(np.int32))):
            got = ver.as_norm(sc, idx[0], idx[1], enroll_stats=tt(e), test_stats=tt(t))
            assert got.dtype == torch.float64 and got.shape == (200,) and not got.is_cuda
            ref = want if sc.dtype == torch.float64 else S.as_norm(scores.astype(np.float32), je, it, e, t)
            # the same five IEEE operations per trial in both; a few ulps of the largest term allow for their order
            assert np.abs(got.numpy() - ref).max() <= 8 * np.finfo(np.float64).eps * np.abs(ref).max()


def test_as_norm_zero_sigma_is_ieee():
    got = ver.as_norm(torch.tensor([1.0, 2.0]), [0, 0], [0, 0], enroll_stats=(torch.tensor([1.0]), torch.tensor([0.0])))
    assert torch.isnan(got[0]) and torch.isinf(got[1])


def test_as_norm_argument_checks():
    scores, je, it, es, ts = _case()
    sc = torch.as_tensor(scores)
    tt = lambda p: tuple(torch.as_tensor(a) for a in p)  # noqa: E731
    with pytest.raises(ValueError):
        ver.as_norm(sc, je, it)                                    # neither side
    bad_e = je.copy()
    bad_e[5] = 17
    bad_t = it.copy()
    bad_t[0] = -1
    for a, b in ((bad_e, it), (je, bad_t), (je[:-1], it), (je.astype(np.float64), it), (je.reshape(2, -1), it),
                 (torch.as_tensor(bad_e), torch.as_tensor(it)), (torch.as_tensor(je) > 0, torch.as_tensor(it))):
        with pytest.raises(ValueError):
            ver.as_norm(sc, a, b, enroll_stats=tt(es), test_stats=tt(ts))
    with pytest.raises(ValueError):
        ver.as_norm(sc, je, it, enroll_stats=(torch.as_tensor(es[0]),))
    with pytest.raises(ValueError):
        ver.as_norm(sc, je, it, enroll_stats=(torch.as_tensor(es[0]), torch.as_tensor(es[1][:-1])))
    with pytest.raises(ValueError):
        ver.as_norm(sc.reshape(2, -1), je, it, enroll_stats=tt(es))
    with pytest.raises(ValueError):
        ver.score_normalized(None, None, None, (je, it), None, sides="left")


def test_new_prototypes_and_host_validation():
    for name in NEW:
        assert name in L.PROTOTYPES, name
    lib = L.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.ktf_plda_cohort_workspace_bytes(70, 90, 128, 8) == 70 * 90 * 8
    assert lib.ktf_plda_cohort_workspace_bytes(0, 90, 128, 4) == 0
    for bad in ((70, 0, 128, 8), (-1, 90, 128, 8), (70, 90, 0, 8), (70, 90, 128, 2)):
        assert lib.ktf_plda_cohort_workspace_bytes(*bad) < 0
    p = C.c_void_p(256)                                            # never dereferenced: every call below is refused or launches nothing
    for fn in (lib.ktf_topn_stats_f64, lib.ktf_topn_stats_f32):
        assert fn(None, 0, 5, 5, 2, None, None, None) == 0         # R == 0: success, nothing launched
        assert fn(p, 3, 0, 5, 2, p, p, None) == -1 and "C = 0" in L.last_error()
        assert fn(p, 3, 5, 5, 0, p, p, None) == -1 and "top_n" in L.last_error()
        assert fn(p, 3, 5, 4, 2, p, p, None) == -1 and "stride" in L.last_error()
        assert fn(None, 3, 5, 5, 2, p, p, None) == -1 and "null" in L.last_error()
        assert fn(p, 3, 5, 5, 2, None, p, None) == -1 and "null" in L.last_error()
    for fn in (lib.ktf_plda_cohort_stats_f64, lib.ktf_plda_cohort_stats_f32):
        assert fn(None, 0, None, 5, 8, None, None, 0, 2, None, None, None, 0, None) == 0
        assert fn(p, 3, p, 5, 8, p, None, 2, 2, p, p, p, 1 << 20, None) == -1 and "role" in L.last_error()
        assert fn(p, 3, p, 0, 8, p, None, 0, 2, p, p, p, 1 << 20, None) == -1
        assert fn(p, 3, p, 5, 8, p, None, 0, 0, p, p, p, 1 << 20, None) == -1 and "top_n" in L.last_error()
        assert fn(p, 3, None, 5, 8, p, None, 1, 2, p, p, p, 1 << 20, None) == -1 and "null" in L.last_error()
        assert fn(p, 3, p, 5, 8, p, None, 1, 2, p, p, p, 8, None) == -1 and "workspace" in L.last_error()
