"""CPU half of UBM training: the fp64 oracle (_ubm_train_ref) against facts that do not come from it (EM
monotonicity, the recovery of a generating mixture, the floors and the removal on inputs built to trigger them, the invariants of a
split), the host-side model classes and the Kaldi-binary writers, byte for byte. No kernel is launched here."""

import struct

import numpy as np
import pytest

import _fgmm_ref as FR
import _ubm_train_ref as U
from kaldi_tflite_amd import training
from kaldi_tflite_amd.io import (DiagGmmModel, FullGmmModel, KaldiDiagGmmReader, KaldiFullGmmReader, WriteKaldiDiagGmm,
                                 WriteKaldiFullGmm)


def _start_model(rng, x, I):
    x64 = x.astype(np.float64)
    var = np.tile(x64.var(0), (I, 1))
    return DiagGmmModel(np.full(I, 1.0 / I), x64[rng.choice(len(x), I, replace=False)] / var, 1.0 / var)


@pytest.mark.parametrize("full", [False, True], ids=["diag", "full"])
def test_em_does_not_decrease_the_frame_loglikelihood(full):
    """Six iterations over all Gaussians (every frame lists every Gaussian: exact EM); no floor and no removal engages."""
    rng = np.random.default_rng(5)
    I, D, F = 4, 3, 1200
    x = U.mixture(rng, I, D, F, spread=2.0)
    d = _start_model(rng, x, I)
    sel = np.tile(np.arange(I, dtype=np.int32), (F, 1))
    if full:
        _, objf, infos = U.train_full_ubm(U.diag_to_full(d), x, sel, 6, min_gaussian_occupancy=10.0)
    else:
        _, objf, infos = U.train_diag_ubm(d, x, sel, 6)
    assert all(not i["removed"] and i["floored"] == 0 for i in infos), infos
    assert all(b >= a - 1e-12 for a, b in zip(objf, objf[1:])), objf
    assert objf[-1] > objf[0] + 1e-3


def test_a_separated_mixture_is_recovered():
    """3 components, D = 2, means 12 apart, 3000 frames: after EM from frames of the three clusters the parameters are those of
    the generator within 3 standard errors of a component's sample mean, 3 / sqrt(frames per component) (unit variances);
    variances within 3 sqrt(2 / n), weights within 3 sqrt(w (1 - w) / F)."""
    rng = np.random.default_rng(11)
    means = np.array([[0.0, 0.0], [12.0, 0.0], [0.0, 12.0]])
    w_true = np.array([0.5, 0.3, 0.2])
    F = 3000
    c = rng.choice(3, F, p=w_true)
    x = (means[c] + rng.standard_normal((F, 2))).astype(np.float32)
    first = [int(np.nonzero(c == k)[0][0]) for k in range(3)]
    model, _, _ = U.init_diag_ubm(x, 3, 3, 8, first, iter(()))
    w, m, v = U.diag_params(model)
    n = np.bincount(c, minlength=3)
    for k in range(3):
        assert np.abs(m[k] - means[k]).max() < 3.0 / np.sqrt(n[k]), (k, m[k])
        assert np.abs(v[k] - 1.0).max() < 3.0 * np.sqrt(2.0 / n[k]), (k, v[k])
        assert abs(w[k] - w_true[k]) < 3.0 * np.sqrt(w_true[k] * (1 - w_true[k]) / F), (k, w[k])


def _stats_for(x, resp, full):
    I = resp.shape[1]
    sel = np.tile(np.arange(I, dtype=np.int32), (len(x), 1))
    return U.stats_on_pairs(x, sel, resp, I, full)


def test_floors_and_removal_engage_on_inputs_built_for_them():
    rng = np.random.default_rng(3)
    F, D = 600, 3
    x = rng.standard_normal((F, D))
    x[:, 2] *= 1e-3                                          # variance 1e-6 < min_variance / variance_floor
    x = x.astype(np.float32)
    resp = np.zeros((F, 3))
    resp[:400, 0] = 1.0
    resp[400:595, 1] = 1.0
    resp[595:, 2] = 1.0                                      # 5 frames < min_gaussian_occupancy
    d0 = DiagGmmModel(np.full(3, 1 / 3), np.zeros((3, D)), np.ones((3, D)))
    # diagonal: variance floor + removal
    d, info = U.diag_est(d0, *_stats_for(x, resp, False))
    assert info["removed"] == [2] and info["floored"] == 2 and d.numGauss == 2
    assert abs(float(d.weights.astype(np.float64).sum()) - 1.0) < 1e-6
    assert np.allclose(1.0 / d.inv_vars[:, 2], 0.001, rtol=1e-6)
    # kept instead of removed: the old parameters, weight prob_i
    d, info = U.diag_est(d0, *_stats_for(x, resp, False), remove=False)
    assert d.numGauss == 3 and not info["removed"] and np.array_equal(d.inv_vars[2], d0.inv_vars[2])
    assert abs(float(d.weights[2]) - 5 / F) < 1e-7
    # full: the condition-number floor (lam_max ~ 1, lam_min ~ 1e-6, max_condition 1e3 -> floor ~ 1e-3 > variance_floor 1e-4)
    g, info = U.full_est(U.diag_to_full(d0), *_stats_for(x, resp, True), variance_floor=1e-4, max_condition=1e3)
    assert info["removed"] == [2] and info["floored"] == 2
    assert abs(float(g.weights.astype(np.float64).sum()) - 1.0) < 1e-6
    lam = np.linalg.eigvalsh(g.inv_covars.astype(np.float64))
    assert (lam > 0).all() and (lam.max(1) / lam.min(1) <= 1e3 * (1 + 1e-5)).all(), lam
    # full: the variance floor alone
    g, info = U.full_est(U.diag_to_full(d0), *_stats_for(x, resp, True), variance_floor=0.01, max_condition=1e9)
    lam = np.linalg.eigvalsh(np.linalg.inv(g.inv_covars.astype(np.float64)))
    assert info["floored"] == 2 and np.allclose(lam.min(1), 0.01, rtol=1e-5)
    with pytest.raises(ValueError):
        U.diag_est(d0, *_stats_for(x[:9], resp[:9], False))  # 9 frames: nobody passes the occupancy gate


def test_split_keeps_total_weight_and_weighted_mean():
    rng = np.random.default_rng(8)
    w = np.array([0.2, 0.5, 0.3])
    mean, var = rng.standard_normal((3, 4)), rng.uniform(0.5, 2.0, (3, 4))
    normals = rng.standard_normal((3, 4))
    for fn in (U.split, training.split_largest):
        w2, m2, v2 = fn(w, mean, var, 6, iter(normals))
        assert len(w2) == 6 and abs(w2.sum() - 1.0) < 1e-15
        assert np.allclose(w2 @ m2, w @ mean, atol=1e-14)
        assert np.array_equal(v2[3], var[1]) and w2[3] == 0.25              # the largest (0.5) went first ...
        assert w2[2] == 0.15 and w2[1] == 0.125 and w2[5] == 0.125          # ... then 0.3, then the lower index of the 0.25 pair
    a, b = U.split(w, mean, var, 6, iter(normals)), training.split_largest(w, mean, var, 6, iter(normals))
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


def test_diag_to_full_and_back():
    rng = np.random.default_rng(2)
    I, D = 5, 4
    iv = rng.uniform(0.5, 2.0, (I, D))
    w = rng.uniform(0.5, 1.5, I)
    d = DiagGmmModel(w / w.sum(), rng.standard_normal((I, D)) * iv, iv)
    f = training.diag_to_full(d)
    assert isinstance(f, FullGmmModel) and np.array_equal(f.inv_covars, U.diag_to_full(d).inv_covars)
    back = f.toDiag()
    assert np.array_equal(back.weights, d.weights)
    assert np.allclose(back.inv_vars, d.inv_vars, rtol=2e-7, atol=0) and np.allclose(back.means_invvars, d.means_invvars, rtol=1e-6, atol=1e-7)
    assert np.allclose(f.gconsts, d.gconsts, atol=1e-5)


def _tok(t):
    return t.encode() + b" "


def _i32(v):
    return b"\x04" + struct.pack("<i", v)


@pytest.mark.parametrize("I,D", [(1, 1), (3, 4), (1, 5), (4, 1)])
def test_writers_round_trip_and_byte_layout(tmp_path, I, D):
    rng = np.random.default_rng(100 + 10 * I + D)
    w = rng.uniform(0.5, 1.5, I)
    iv = rng.uniform(0.5, 2.0, (I, D))
    d = DiagGmmModel(w / w.sum(), rng.standard_normal((I, D)), iv)
    p = str(tmp_path / "final.dubm")
    WriteKaldiDiagGmm(p, d)
    f4 = lambda a: np.ascontiguousarray(a, "<f4").tobytes()  # noqa: E731
    want = (b"\0B" + _tok("<DiagGMM>") + _tok("<GCONSTS>") + b"FV " + _i32(I) + f4(d.gconsts) + _tok("<WEIGHTS>") + b"FV " + _i32(I)
            + f4(d.weights) + _tok("<MEANS_INVVARS>") + b"FM " + _i32(I) + _i32(D) + f4(d.means_invvars) + _tok("<INV_VARS>") + b"FM "
            + _i32(I) + _i32(D) + f4(d.inv_vars) + _tok("</DiagGMM>"))
    assert open(p, "rb").read() == want
    r = KaldiDiagGmmReader(p)
    for k in ("weights", "means_invvars", "inv_vars", "gconsts"):
        assert np.array_equal(getattr(r, k), getattr(d, k)) and getattr(r, k).dtype == np.float32, k
    assert np.array_equal(r.storedGconsts, d.gconsts)

    stored, _ = FR.random_full_ubm(rng, I, D)
    g = FullGmmModel(*stored)
    p = str(tmp_path / "final.ubm")
    WriteKaldiFullGmm(p, g)
    tri = np.tril_indices(D)
    want = (b"\0B" + _tok("<FullGMM>") + _tok("<GCONSTS>") + b"FV " + _i32(I) + f4(g.gconsts) + _tok("<WEIGHTS>") + b"FV " + _i32(I)
            + f4(g.weights) + _tok("<MEANS_INVCOVARS>") + b"FM " + _i32(I) + _i32(D) + f4(g.means_invcovars) + _tok("<INV_COVARS>")
            + b"".join(b"FP " + _i32(D) + f4(g.inv_covars[i][tri]) for i in range(I)) + _tok("</FullGMM>"))
    assert open(p, "rb").read() == want
    r = KaldiFullGmmReader(p)
    for k in ("weights", "means_invcovars", "inv_covars", "gconsts"):
        assert np.array_equal(getattr(r, k), getattr(g, k)) and getattr(r, k).dtype == np.float32, k
    # the file of the test-suite's own writer, byte for byte
    q = str(tmp_path / "ref.ubm")
    FR.write_full_gmm(q, *stored, gconsts=g.gconsts)
    assert open(q, "rb").read() == open(p, "rb").read()
    with pytest.raises(NotImplementedError):
        WriteKaldiFullGmm(p, g, binary=False)
    with pytest.raises(NotImplementedError):
        WriteKaldiDiagGmm(p, d, binary=False)


def test_models_reject_bad_fields():
    with pytest.raises(ValueError):
        DiagGmmModel(np.ones(2) / 2, np.zeros((3, 2)), np.ones((3, 2)))
    with pytest.raises(ValueError):
        FullGmmModel(np.ones(1), np.zeros((1, 2)), np.array([[[1.0, 2.0], [2.0, 1.0]]]))     # not positive definite
    with pytest.raises(ValueError):
        training.DiagGmmStats(DiagGmmModel(np.ones(1), np.zeros((1, 200)), np.ones((1, 200))))   # D beyond the limit


def test_estimators_match_the_oracle_on_host_statistics():
    """diag_gmm_est / full_gmm_est (vectorised) against the oracle's per-Gaussian loops on the same statistics, removal included."""
    rng = np.random.default_rng(21)
    I, D, F = 5, 3, 900
    x = U.mixture(rng, I, D, F, spread=2.0)
    d0 = _start_model(rng, x, I)
    post, _, _ = U.softmax_rows(U.diag_loglikes(x, d0))
    post[:, 4] *= 1e-3                                       # Gaussian 4 falls under the occupancy gate
    for full in (False, True):
        occ, macc, sec = _stats_for(x, post, full)
        st = (training.FullGmmStats if full else training.DiagGmmStats)(U.diag_to_full(d0) if full else d0)
        st.host = lambda o=occ, m=macc, s=sec: (o, m, s)
        for remove in (True, False):
            if full:
                got = training.full_gmm_est(U.diag_to_full(d0), st, remove_low_count_gaussians=remove)
                want, info = U.full_est(U.diag_to_full(d0), occ, macc, sec, remove=remove)
                names = ("weights", "means_invcovars", "inv_covars")
            else:
                got = training.diag_gmm_est(d0, st, remove_low_count_gaussians=remove)
                want, info = U.diag_est(d0, occ, macc, sec, remove=remove)
                names = ("weights", "means_invvars", "inv_vars")
            assert got.estInfo["removed"] == len(info["removed"]) == (1 if remove else 0)
            assert got.estInfo["floored"] == info["floored"]
            for k in names:
                assert np.allclose(getattr(got, k), getattr(want, k), rtol=1e-5, atol=1e-6), k
