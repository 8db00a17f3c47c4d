"""CPU half of i-vector extraction: the extractor reader against the 15 Kaldi dummy extractors, the DiagGMM reader, the two NumPy
forms of the extraction against each other, the count scale, and the C-ABI / layer argument checks that run before any launch."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import _ivector_ref as R
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L
from kaldi_tflite_amd.io import KaldiDiagGmmReader, KaldiIvecExtractorReader, ReadKaldiArray

DUMMIES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ivector_extractor")


def dummy_params(name):
    """The reference's fixture parameters (testdata/ivector_extractor/ivector_extractor.py getParams): M from M.mat.txt, the full
    SigmaInv from the lower triangle in sigma_inv.mat.txt, the sizes and offset from test_params.txt."""
    d = os.path.join(DUMMIES, name)
    p = {"M": ReadKaldiArray(os.path.join(d, "M.mat.txt"), binary=False, dtype=np.float64)}
    with open(os.path.join(d, "sigma_inv.mat.txt")) as f:
        lines = [ln.strip() for ln in f.readlines()][1:]
    sig = np.zeros((len(lines), len(lines)))
    for i, ln in enumerate(lines):
        vals = ln.split()
        if vals[-1] == "]":
            vals = vals[:-1]
        for j, v in enumerate(vals):
            sig[i][j] = float(v)
    p["sigmaInv"] = sig
    with open(os.path.join(d, "test_params.txt")) as f:
        for ln in f:
            if ln.strip():
                k, v = ln.strip().split("=")
                p[k] = int(v) if k in ("numGauss", "featDim", "ivecDim") else float(v)
    return p


@pytest.mark.parametrize("name", [f"dummy_{i:03d}" for i in range(1, 16)])
def test_reader_matches_kaldi_dummies(name):
    want = dummy_params(name)
    got = KaldiIvecExtractorReader(os.path.join(DUMMIES, name, "final.ie"), binary=True)
    assert (got.numGauss, got.featDim, got.ivecDim) == (want["numGauss"], want["featDim"], want["ivecDim"])
    assert got.priorOffset == want["priorOffset"]
    n = want["numGauss"]
    assert len(got.M) == n and len(got.sigmaInv) == n
    assert np.array_equal(want["M"], got.M[0])
    assert np.array_equal(want["sigmaInv"], got.sigmaInv[0])
    wantSigmaInvM = np.matmul(want["sigmaInv"], want["M"])
    assert np.array_equal(wantSigmaInvM, got.sigmaInvM[0])
    wantU = np.matmul(want["M"].T, wantSigmaInvM)
    assert np.array_equal(wantU[np.tril_indices(wantU.shape[0])], got.U[0])
    assert got.U.shape == (n, want["ivecDim"] * (want["ivecDim"] + 1) // 2)
    assert got.w.size == 0 and got.wVec.shape == (n,)


def test_extractor_write_read_round_trip_full_sigma(tmp_path):
    rng = np.random.default_rng(5)
    _, (M, sig) = R.random_models(rng, 5, 3, 7)
    path = str(tmp_path / "final.ie")
    R.write_ivector_extractor(path, M, sig, 42.0)
    r = KaldiIvecExtractorReader(path)
    assert r.priorOffset == 42.0 and (r.numGauss, r.featDim, r.ivecDim) == (5, 3, 7)
    assert np.array_equal(np.asarray(r.M), M)
    assert np.array_equal(np.asarray(r.sigmaInv), sig)          # full symmetric, off-diagonals included
    sim, U = R.derived(M, sig)
    np.testing.assert_allclose(r.sigmaInvM, sim, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(r.U, U, rtol=1e-12, atol=1e-12)


def test_diag_gmm_round_trip_recomputes_gconsts(tmp_path):
    rng = np.random.default_rng(6)
    (w, mi, iv), _ = R.random_models(rng, 9, 4, 3)
    path = str(tmp_path / "final.dubm")
    R.write_diag_gmm(path, w, mi, iv, gconsts=np.full(9, 123.0, np.float32))     # stored values are not trusted
    g = KaldiDiagGmmReader(path)
    assert (g.numGauss, g.featDim) == (9, 4)
    assert np.array_equal(g.weights, w) and np.array_equal(g.means_invvars, mi) and np.array_equal(g.inv_vars, iv)
    assert np.array_equal(g.storedGconsts, np.full(9, 123.0, np.float32))
    assert g.gconsts.dtype == np.float32
    mean = mi.astype(np.float64) / iv
    want = np.log(w.astype(np.float64)) - 0.5 * 4 * np.log(2 * np.pi) + np.sum(0.5 * np.log(iv) - 0.5 * mean * mean * iv, axis=1)
    np.testing.assert_allclose(g.gconsts, want, rtol=1e-5, atol=1e-5)
    # the log-likelihood these give is the Gaussian's log density
    x = rng.standard_normal((3, 4))
    ll = R.loglikes(x, (g.gconsts, mi, iv))
    dens = np.log(w)[None] + np.sum(-0.5 * np.log(2 * np.pi) + 0.5 * np.log(iv)[None] - 0.5 * (x[:, None] - mean[None]) ** 2 * iv[None], axis=2)
    np.testing.assert_allclose(ll, dens, rtol=1e-5, atol=1e-4)


def test_oracle_forms_agree():
    rng = np.random.default_rng(7)
    for I, D, S in ((2, 2, 4), (6, 5, 9), (17, 7, 30)):
        (w, mi, iv), (M, sig) = R.random_models(rng, I, D, S)
        gm = KaldiDiagGmmReader.__new__(KaldiDiagGmmReader)
        gm.weights, gm.means_invvars, gm.inv_vars, gm.numGauss, gm.featDim = w, mi, iv, I, D
        x = (rng.standard_normal((40, D)) * 1.2).astype(np.float32)
        g, p = R.posteriors(x, (gm.computeGconsts(), mi, iv), 4, 0.025)
        gamma, F = R.stats(x, g, p, I)
        sim, U = R.derived(M, sig)
        a = R.extract_packed(gamma, F, sim, U, 100.0)
        b = R.extract_dense(gamma, F, M, sig, 100.0)
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9 * np.abs(b).max())
        assert np.abs(a).max() > 1e-3


def test_empty_utterance_is_zero():
    rng = np.random.default_rng(8)
    _, (M, sig) = R.random_models(rng, 3, 2, 5)
    sim, U = R.derived(M, sig)
    gamma, F = R.stats(np.zeros((0, 2), np.float32), np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32), 3)
    assert np.array_equal(R.extract_packed(gamma, F, sim, U, 50.0), np.zeros(5))
    assert np.array_equal(R.extract_dense(gamma, F, M, sig, 50.0), np.zeros(5))


def test_selection_contract_by_hand():
    ll = np.array([0.0, 2.0, 2.0, -1.0, -9.0])
    idx, p = R.select(ll, 3, 0.0)
    assert idx.tolist() == [1, 2, 0]                   # ties: the lower index first
    e = np.exp([0.0, 0.0, -2.0])
    np.testing.assert_allclose(p, e / e.sum())
    idx, p = R.select(ll, 5, 0.05)                     # -1 and -9 fall below 0.05 of the running sum, 0 does not
    assert idx.tolist() == [1, 2, 0]
    idx, p = R.select(np.array([0.0, -50.0]), 2, 0.5)  # at least one kept
    assert idx.tolist() == [0] and p.tolist() == [1.0]


def test_max_count_arithmetic():
    post = np.full((100, 2), 0.5, np.float32)          # 100 frames' worth of posterior
    np.testing.assert_array_equal(R.count_scale(post), post)
    np.testing.assert_array_equal(R.count_scale(post, max_count=200.0), post)     # under the cap: untouched
    w = R.count_scale(post, max_count=40.0)
    assert w.dtype == np.float32 and abs(float(w.sum(dtype=np.float64)) - 40.0) < 1e-4
    assert np.all(w == np.float32(0.5) * np.float32(0.4))
    w = R.count_scale(post, posterior_scale=0.5, acoustic_weight=2.0, max_count=80.0)   # 2 * 50 = 100 > 80
    assert np.all(w == np.float32(0.25) * np.float32(2.0 * 0.8))
    w = R.count_scale(post, posterior_scale=0.1, acoustic_weight=0.5)
    assert np.all(w == (np.float32(0.5) * np.float32(0.1)) * np.float32(0.5))


def _p(n=0):
    return C.c_void_p(0x1000 + 256 * n) if n >= 0 else None


def test_cabi_rejects_bad_arguments_without_gpu():
    lib = L.load()
    wsb = lib.ktf_ivector_workspace_bytes
    assert wsb(4, 8, 3, 5) > 0
    for args in ((0, 8, 3, 5), (4, 0, 3, 5), (4, 8, 0, 5), (4, 8, 129, 5), (4, 8, 3, 0), (4, 8, 3, 1025), (4, 8193, 3, 5)):
        assert wsb(*args) == -1, args
    post = lib.ktf_ivector_post_f32
    ok = dict(x=_p(), F=10, D=3, ldx=3, W=_p(1), g=_p(2), I=8, n=4, mp=0.025, ga=_p(3), po=_p(4))

    def call_post(**kw):
        a = dict(ok, **kw)
        return post(a["x"], a["F"], a["D"], a["ldx"], a["W"], a["g"], a["I"], a["n"], a["mp"], a["ga"], a["po"], None)
    for bad in (dict(D=0), dict(D=129), dict(ldx=2), dict(I=0), dict(n=0), dict(n=65), dict(mp=1.0), dict(mp=-0.1), dict(F=-1),
                dict(x=None), dict(W=None), dict(ga=None)):
        assert call_post(**bad) == -1, bad
        assert L.last_error().startswith("ktf_ivector_post_f32")
    assert call_post(F=0, x=None) == 0                  # nothing to do, nothing launched
    ext = lib.ktf_ivector_extract
    need = wsb(2, 8, 3, 5)
    base = dict(x=_p(), F=10, D=3, ldx=3, off=_p(1), B=2, ga=_p(2), po=_p(3), n=4, ps=1.0, aw=1.0, mc=0.0, sim=_p(4), U=_p(5), I=8, S=5,
                po0=10.0, out=_p(6), ob=4, ws=_p(7), wsn=need)

    def call_ext(**kw):
        a = dict(base, **kw)
        return ext(a["x"], a["F"], a["D"], a["ldx"], a["off"], a["B"], a["ga"], a["po"], a["n"], a["ps"], a["aw"], a["mc"], a["sim"],
                   a["U"], a["I"], a["S"], a["po0"], a["out"], a["ob"], a["ws"], a["wsn"], None)
    for bad in (dict(B=0), dict(I=0), dict(S=1025), dict(D=0), dict(ldx=2), dict(n=0), dict(n=65), dict(ps=-1.0), dict(aw=-1.0),
                dict(mc=-1.0), dict(ob=2), dict(wsn=need - 1), dict(ws=C.c_void_p(0x1008)), dict(off=None), dict(U=None), dict(sim=None),
                dict(out=None), dict(x=None), dict(ga=None), dict(F=-1)):
        assert call_ext(**bad) == -1, bad
        assert L.last_error().startswith("ktf_ivector")


def _model_files(tmp_path, rng, I=4, D=3, S=5, w=None):
    (wt, mi, iv), (M, sig) = R.random_models(rng, I, D, S)
    ie, ubm = str(tmp_path / "final.ie"), str(tmp_path / "final.dubm")
    R.write_ivector_extractor(ie, M, sig, 100.0, w=w)
    R.write_diag_gmm(ubm, wt, mi, iv)
    return ie, ubm


def test_weight_projection_extractor_raises(tmp_path):
    rng = np.random.default_rng(9)
    ie, ubm = _model_files(tmp_path, rng, w=rng.standard_normal((4, 5)))
    r = KaldiIvecExtractorReader(ie)                    # the reader still parses it
    assert r.w.shape == (4, 5)
    with pytest.raises(NotImplementedError):
        ktf.layers.IvectorExtractor(ie, ubm)


def test_layer_rejects_bad_configuration(tmp_path):
    rng = np.random.default_rng(10)
    ie, ubm = _model_files(tmp_path, rng)
    for kw in (dict(num_gselect=0), dict(num_gselect=65), dict(min_post=1.0), dict(min_post=-0.5), dict(max_count=-1.0)):
        with pytest.raises(ValueError):
            ktf.layers.IvectorExtractor(ie, ubm, **kw)
    ubm2 = str(tmp_path / "other.dubm")
    (wt, mi, iv), _ = R.random_models(rng, 6, 3, 5)
    R.write_diag_gmm(ubm2, wt, mi, iv)
    with pytest.raises(ValueError):
        ktf.layers.IvectorExtractor(ie, ubm2)
    layer = ktf.layers.IvectorExtractor(KaldiIvecExtractorReader(ie), KaldiDiagGmmReader(ubm))
    assert (layer.numGselect, layer.minPost, layer.ivecDim) == (20, 0.025, 5)
    with pytest.raises(ValueError):
        layer(torch.zeros((1, 4, 3)))                   # not on a GPU
