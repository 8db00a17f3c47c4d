"""CPU half of dense PLDA scoring (Kaldi ivector-plda-scoring-dense): the NumPy restatement is pinned to Kaldi's with-PCA golden,
and the C-ABI and PLDA.score_dense reject bad arguments before anything reaches a GPU."""

import ctypes as C

import numpy as np
import pytest

import _golden as G
import _plda_dense_ref as P
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L


def _golden_case():
    z, g = G.load("plda.npz"), G.load("plda_dense.npz")
    p = ktf.io.KaldiPldaReader(G.GOLDEN + "/plda.bin", True)
    return z["plda_input"][:, 0, :], p, g


def test_restatement_reproduces_kaldi_with_pca_golden():
    x, p, g = _golden_case()
    assert g["plda_dense_scores"].shape == (29, 29) and float(g["target_energy"]) == 0.1
    s, d = P.score_dense(x, p.mean, p.transformMat, p.psi, float(g["target_energy"]))
    assert d == 2
    assert G.rmse(g["plda_dense_scores"], s) <= 1e-6


def test_restatement_without_kaldis_off_by_one_does_not():
    x, p, g = _golden_case()
    s, d = P.score_dense(x, p.mean, p.transformMat, p.psi, 0.1, off_by_one=False)
    assert d == 1
    assert G.rmse(g["plda_dense_scores"], s) > 0.1
    # ... nor does scoring without PCA (the table the reference does test)
    s0, d0 = P.score_dense(x, p.mean, p.transformMat, p.psi, None)
    assert d0 == 0 and G.rmse(g["plda_dense_scores"], s0) > 0.1 and G.rmse(G.load("plda.npz")["plda_scores"], s0) < 1e-5


def test_restatement_edge_rules():
    rng = np.random.default_rng(5)
    D = 16
    T = rng.standard_normal((D, D)) / 4 + np.eye(D)
    mean, psi = rng.standard_normal(D) * 0.1, np.sort(rng.uniform(0.1, 10, D))[::-1]
    assert P.score_dense(rng.standard_normal((1, D)), mean, T, psi, 0.5)[1] == 0            # n = 1: rank 0
    assert P.score_dense(np.tile(rng.standard_normal(D), (6, 1)), mean, T, psi, 0.5)[1] == 0  # all rows equal
    x2 = rng.standard_normal((2, D))
    lam = np.linalg.eigvalsh(np.cov(x2.T, bias=True))[::-1]
    assert P.kaldi_pca_dim(lam, 0.5) == 2                                                     # Kaldi's d ...
    assert P.score_dense(x2, mean, T, psi, 0.5)[1] == 1                                       # ... clamped to the rank


def test_dense_abi_argument_validation_without_gpu():
    lib = L.load()
    buf = (C.c_double * 64)()
    fbuf = (C.c_float * 64)()
    ibuf = (C.c_int32 * 8)()
    lens = (C.c_int32 * 3)(2, 3, 4)

    def call(fn=lib.ktf_plda_dense_f64, b=buf, x=True, S=9, dim=8, lengths=lens, R=3, t=0.1, ws_bytes=1 << 30, consts=True,
             dims=True, status=True):
        return fn(b if x else None, S, dim, lengths, ibuf, R, t, b, b, b, buf if consts else None, buf, buf, 1, 0, b,
                  ibuf if dims else None, buf, ws_bytes, ibuf if status else None, None)

    for kw, msg in [({"x": False}, "null"), ({"dims": False}, "null"), ({"status": False}, "null"),
                    ({"consts": False}, "fp64 model constant"), ({"lengths": None}, "null lengths"),
                    ({"dim": 513}, "outside 1..512"), ({"dim": 0}, "outside 1..512"), ({"R": 0}, "at least one"),
                    ({"lengths": (C.c_int32 * 3)(2, 0, 7)}, "lengths[1] = 0"), ({"S": 10}, "add up to 9 rows"),
                    ({"t": 1.0}, "outside [0, 1)"), ({"t": -0.5}, "outside [0, 1)"), ({"t": float("nan")}, "outside [0, 1)"),
                    ({"ws_bytes": 64}, "workspace of 64 bytes"),
                    ({"fn": lib.ktf_plda_dense_f32, "b": fbuf, "dim": 600}, "outside 1..512")]:
        assert call(**kw) == -1, kw
        assert msg in L.last_error(), (kw, L.last_error())
    with pytest.raises(ValueError):
        L.check(-1, "x")
    # without PCA the fp64 constants are not needed, the other checks stand
    assert call(consts=False, t=L.PLDA_DENSE_NO_PCA, ws_bytes=8) == -1 and "workspace" in L.last_error()
    # the size query checks the same lengths; the no-PCA workspace is smaller
    with_pca = lib.ktf_plda_dense_workspace_bytes(lens, 3, 8, 0.1)
    without = lib.ktf_plda_dense_workspace_bytes(lens, 3, 8, L.PLDA_DENSE_NO_PCA)
    assert with_pca > without > 0
    assert lib.ktf_plda_dense_workspace_bytes((C.c_int32 * 2)(4, -1), 2, 8, 0.1) == -1 and "lengths[1]" in L.last_error()


def _layer(dim=8, dtype="float64"):
    rng = np.random.default_rng(3)
    return ktf.layers.PLDA(dim, rng.standard_normal(dim) * 0.1, rng.standard_normal((dim, dim)) / 4 + np.eye(dim),
                           np.sort(rng.uniform(0.1, 10, dim))[::-1].copy(), dtype=dtype)


@pytest.mark.parametrize("kwargs,inputs_shape", [
    ({"target_energy": 1.0}, (9, 8)),
    ({"target_energy": -0.1}, (9, 8)),
    ({"target_energy": float("nan")}, (9, 8)),
    ({"target_energy": "0.1"}, (9, 8)),
    ({"target_energy": True}, (9, 8)),
    ({"lengths": [4, 4]}, (9, 8)),
    ({"lengths": [9, 0]}, (9, 8)),
    ({"lengths": [4.5, 4.5]}, (9, 8)),
    ({"lengths": [[4, 5]]}, (9, 8)),
    ({"lengths": []}, (9, 8)),
    ({}, (9, 7)),
    ({}, (9, 2, 8)),
    ({}, (9, 8, 1)),
    ({}, (9,)),
])
def test_score_dense_rejects_bad_arguments(kwargs, inputs_shape):
    with pytest.raises(ValueError):
        _layer().score_dense(np.zeros(inputs_shape), **kwargs)


def test_score_dense_rejects_dims_above_512():
    with pytest.raises(ValueError, match="dim <= 512"):
        _layer(dim=520, dtype="float32").score_dense(np.zeros((4, 1, 520)), lengths=[1, 3])
