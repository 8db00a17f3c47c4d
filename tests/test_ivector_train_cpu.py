"""CPU half of i-vector extractor training: the writer against the 15 Kaldi dummy extractors (all 15 are Kaldi-binary files), the
update rules of the oracle (_ivector_train_ref) and of training.ivector_extractor_est on the oracle's statistics, EM monotonicity and
recovery of a known model, and the C-ABI argument checks that run before any launch."""

import ctypes as C
import os

import numpy as np
import pytest
import torch

import _ivector_ref as R
import _ivector_train_ref as T
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L
from kaldi_tflite_amd.io import IvecExtractorModel, KaldiIvecExtractorReader, WriteKaldiIvecExtractor

DUMMIES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ivector_extractor")


@pytest.mark.parametrize("name", [f"dummy_{i:03d}" for i in range(1, 16)])
def test_writer_reproduces_kaldi_dummies(name, tmp_path):
    src = os.path.join(DUMMIES, name, "final.ie")
    raw = open(src, "rb").read()
    assert raw[:2] == b"\0B"                            # a Kaldi-binary fixture
    out = str(tmp_path / "final.ie")
    WriteKaldiIvecExtractor(out, KaldiIvecExtractorReader(src, binary=True))
    assert open(out, "rb").read() == raw


def test_writer_refuses_text_mode(tmp_path):
    _, (M, sig) = R.random_models(np.random.default_rng(1), 3, 2, 4)
    with pytest.raises(NotImplementedError):
        WriteKaldiIvecExtractor(str(tmp_path / "x.ie"), IvecExtractorModel(M, sig, 10.0), binary=False)


def _synthetic(rng, I, D, S, n_utts, frames, n=3, prior_offset=20.0):
    (w, mi, iv), (M, sig) = R.random_models(rng, I, D, S, prior_offset=prior_offset)
    gc = np.log(w) - 0.5 * D * np.log(2 * np.pi) + np.sum(0.5 * np.log(iv) - 0.5 * mi * mi / iv, axis=1)
    utts = []
    for _ in range(n_utts):
        x = (rng.standard_normal((frames, D)) * 1.3 + rng.standard_normal(D) * 0.5).astype(np.float32)
        g, p = R.posteriors(x, (gc, mi, iv), n, 0.025)
        utts.append((x, g, p))
    return M, sig, prior_offset, utts


def test_update_invariants():
    rng = np.random.default_rng(21)
    M, sig, po, utts = _synthetic(rng, 5, 4, 3, 40, 30)
    a = T.accumulate(utts, M, sig, po)
    det = {}
    M2, sig2, po2 = T.update(M, sig, a, gaussian_min_count=0.0, details=det)
    assert po2 > 0
    V = det["V"]
    # the transformed first and second moments of the training i-vectors: mean offset e0, identity covariance
    np.testing.assert_allclose(V @ det["m"], po2 * np.eye(3)[0], atol=1e-9 * po2)
    np.testing.assert_allclose(V @ det["cov"] @ V.T, np.eye(3), atol=1e-9)
    G = sum(a["gamma"][i] * (M2[i].T @ sig2[i] @ M2[i]) for i in range(5)) / a["gamma"].sum()
    off = G[1:, 1:] - np.diag(np.diag(G[1:, 1:]))
    assert np.abs(off).max() <= 1e-9 * np.abs(G).max()
    assert np.all(np.diff(np.diag(G[1:, 1:])) <= 1e-12 * np.abs(G).max())          # eigh_desc: descending
    # the model means are those of the untransformed model at the mean i-vector
    for i in range(5):
        np.testing.assert_allclose(M2[i][:, 0] * po2, det["M_before_prior"][i] @ det["m"], rtol=1e-9, atol=1e-9)
    # without diagonalize the whitening and the offset still hold
    M3, _, po3 = T.update(M, sig, a, gaussian_min_count=0.0, diagonalize=False)
    assert po3 > 0 and abs(po3 - po2) <= 1e-9 * po2


def test_projection_rule():
    rng = np.random.default_rng(22)
    M, sig, po, utts = _synthetic(rng, 4, 3, 3, 30, 25)
    a = T.accumulate(utts, M, sig, po)
    thr = float(np.sort(a["gamma"])[1]) + 1e-9            # the two smallest counts stay below it
    det = {}
    T.update(M, sig, a, gaussian_min_count=thr, details=det)
    assert len(det["updated"]) == 2
    for i in range(4):
        got = det["M_before_prior"][i]
        if i in det["updated"]:
            assert det["floored"][i] == 0
            want = a["Y"][i] @ np.linalg.inv(a["R"][i])
            assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
        else:
            assert np.array_equal(got, M[i])
    # rank-deficient R: one utterance's worth of scatter without its covariance
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    v = rng.standard_normal(3)
    b["R"][0] = 7.0 * np.outer(v, v)
    det = {}
    T.update(M, sig, b, gaussian_min_count=0.0, details=det, update_variances=False)   # (these statistics have no consistent Ssec)
    assert det["floored"][0] == 2 and np.isfinite(det["M_before_prior"][0]).all()


def _cpu_stats(model, a):
    st = ktf.training.IvectorStats(model)
    st._alloc("cpu")
    I, D, S = st.shape
    st.gamma.copy_(torch.as_tensor(a["gamma"]))
    st.Y.copy_(torch.as_tensor(a["Y"].reshape(I * D, S)))
    st.R.copy_(torch.as_tensor(T.pack(a["R"])))
    st.Ssec.copy_(torch.as_tensor(a["Ssec"]))
    st.ivector_sum.copy_(torch.as_tensor(a["ivector_sum"]))
    st.ivector_scatter.copy_(torch.as_tensor(T.pack(a["ivector_scatter"])))
    st.totals[0] = a["num_ivectors"]
    return st


@pytest.mark.parametrize("kw", [dict(), dict(gaussian_min_count=0.0, variance_floor_factor=1e-6), dict(diagonalize=False),
                                dict(gaussian_min_count=0.0, variance_floor_factor=5.0)])
def test_library_update_matches_oracle(kw):
    rng = np.random.default_rng(23)
    M, sig, po, utts = _synthetic(rng, 6, 4, 5, 60, 40)
    a = T.accumulate(utts, M, sig, po)
    if not kw:
        kw = dict(gaussian_min_count=float(np.median(a["gamma"])))
    model = IvecExtractorModel(M, sig, po)
    got = ktf.training.ivector_extractor_est(model, _cpu_stats(model, a), **kw)
    M2, sig2, po2 = T.update(M, sig, a, **kw)
    assert got.estInfo["backend"] == "numpy-host" and got.estInfo["seconds"] >= 0
    assert abs(got.priorOffset - po2) <= 1e-8 * po2
    assert np.abs(np.asarray(got.M) - M2).max() <= 1e-8 * np.abs(M2).max()
    assert np.abs(np.asarray(got.sigmaInv) - sig2).max() <= 1e-8 * np.abs(sig2).max()
    sim, U = R.derived(np.asarray(got.M), np.asarray(got.sigmaInv))
    np.testing.assert_allclose(got.sigmaInvM, sim, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got.U, U, rtol=1e-12, atol=1e-12)


def test_objf_forms_agree():
    rng = np.random.default_rng(24)
    M, sig, po, utts = _synthetic(rng, 5, 4, 6, 12, 20)
    a = T.accumulate(utts, M, sig, po, posterior_scale=0.5)
    model = IvecExtractorModel(M, sig, po)
    st = _cpu_stats(model, a)
    s = 0.0
    for x, g, p in utts:
        _, _, lin, Q, _, w, _ = T.utt_terms(x, g, p, M, sig, po, 0.5)
        s += 0.5 * lin @ w - np.log(np.diag(np.linalg.cholesky(Q))).sum() - 0.5 * po * po
    st.totals[1] = s
    want = T.marginal_objf(utts, M, sig, po, posterior_scale=0.5)
    assert abs(st.objf() - want) <= 1e-10 * abs(want)
    with pytest.raises(ValueError):
        ktf.training.IvectorStats(model, update_variances=False).objf()


MARGIN = 0.02       # nats per frame, see test_em_is_monotone_and_recovers_the_model


def test_em_is_monotone_and_recovers_the_model():
    """400 utterances of 20 frames from a known model (I = 4, D = 3, S = 2), floors inactive. EM must not decrease the marginal
    likelihood. The final model is compared with the generating one on the training data: the maximum-likelihood fit lies ABOVE the
    generating model by about (free parameters) / (2 frames) = 48 / 16000 = 0.003 nats per frame (I (D S + D (D + 1) / 2) = 48), and
    five iterations from a random start may still be short of the maximum; MARGIN = 0.02 nats per frame allows six times that gap in
    either direction, while the initial model is several nats per frame away."""
    rng = np.random.default_rng(25)
    I, D, S, po = 4, 3, 2, 10.0
    (_, _, _), (Mt, sig_t) = R.random_models(rng, I, D, S, prior_offset=po)
    Mt[:, :, 1:] *= 3.0
    sigma_t = np.linalg.inv(sig_t)
    utts = T.sample(rng, Mt, sigma_t, po, 400, 20)
    means = np.stack([np.mean(np.concatenate([x[g[:, 0] == i] for x, g, _ in utts]), axis=0) for i in range(I)])
    covs = np.stack([np.cov(np.concatenate([x[g[:, 0] == i] for x, g, _ in utts]).T.astype(np.float64)) for i in range(I)])
    M, sig, off = T.init(means, np.linalg.inv(covs), S, seed=3)
    objf = []
    for _ in range(5):
        objf.append(T.marginal_objf(utts, M, sig, off))
        a = T.accumulate(utts, M, sig, off)
        M, sig, off = T.update(M, sig, a, variance_floor_factor=1e-8, gaussian_min_count=0.0)
    objf.append(T.marginal_objf(utts, M, sig, off))
    truth = T.marginal_objf(utts, Mt, sig_t, po)
    print("objf per iteration", objf, "generating model", truth)
    assert all(b >= a - 1e-10 * abs(a) for a, b in zip(objf, objf[1:])), objf
    assert abs(objf[-1] - truth) <= MARGIN, (objf, truth)
    assert objf[0] < truth - 10 * MARGIN


def test_init_from_full_ubm(tmp_path):
    import _fgmm_ref as FG
    rng = np.random.default_rng(26)
    if not hasattr(FG, "write_full_gmm"):
        pytest.fail("the full-GMM writer of _fgmm_ref is gone")
    I, D = 5, 3
    w = rng.uniform(0.5, 1.5, I)
    w = (w / w.sum()).astype(np.float32)
    A = rng.standard_normal((I, D, D)) * 0.3
    ic = (np.einsum("idk,iek->ide", A, A) + np.eye(D)[None]).astype(np.float32)
    ic = 0.5 * (ic + np.swapaxes(ic, 1, 2))
    mean = rng.standard_normal((I, D))
    mic = np.einsum("ide,ie->id", ic.astype(np.float64), mean).astype(np.float32)
    path = str(tmp_path / "final.ubm")
    FG.write_full_gmm(path, w, mic, ic)
    m = ktf.training.ivector_extractor_init(path, 4, seed=7)
    assert (m.numGauss, m.featDim, m.ivecDim, m.priorOffset) == (I, D, 4, 100.0) and m.w.size == 0
    np.testing.assert_array_equal(np.asarray(m.sigmaInv), ic.astype(np.float64))
    np.testing.assert_allclose(np.asarray(m.M)[:, :, 0] * 100.0, np.linalg.solve(ic.astype(np.float64), mic.astype(np.float64)[:, :, None])[:, :, 0],
                               rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(m.wVec, np.log(w.astype(np.float64)))
    np.testing.assert_array_equal(np.asarray(m.M)[:, :, 1:], np.random.default_rng(7).standard_normal((I, D, 4))[:, :, 1:])
    again = ktf.training.ivector_extractor_init(path, 4, seed=7)
    assert np.array_equal(np.asarray(again.M), np.asarray(m.M))
    with pytest.raises(ValueError):
        ktf.training.ivector_extractor_init(path, 0)


def _p(n=0):
    return C.c_void_p(0x1000 + 256 * n) if n >= 0 else None


def test_cabi_rejects_bad_arguments_without_gpu():
    lib = L.load()
    wsb = lib.ktf_ivector_train_workspace_bytes
    assert wsb(4, 8, 3, 5) >= lib.ktf_ivector_workspace_bytes(4, 8, 3, 5) + 4 * (15 + 5 + 2) * 8
    for args in ((0, 8, 3, 5), (4, 0, 3, 5), (4, 8, 0, 5), (4, 8, 129, 5), (4, 8, 3, 0), (4, 8, 3, 1025), (4, 8193, 3, 5), (65536, 8, 3, 5)):
        assert wsb(*args) == -1, args
    acc = lib.ktf_ivector_acc_stats
    need = wsb(2, 8, 3, 5)
    base = dict(x=_p(), F=10, D=3, ldx=3, off=_p(1), B=2, ga=_p(2), po=_p(3), n=4, ps=1.0, sim=_p(4), U=_p(5), I=8, S=5, po0=10.0,
                gm=_p(6), Y=_p(7), R=_p(8), isum=_p(9), isc=_p(10), tot=_p(11), ws=_p(12), wsn=need)

    def call_acc(**kw):
        a = dict(base, **kw)
        return acc(a["x"], a["F"], a["D"], a["ldx"], a["off"], a["B"], a["ga"], a["po"], a["n"], a["ps"], a["sim"], a["U"], a["I"], a["S"],
                   a["po0"], a["gm"], a["Y"], a["R"], a["isum"], a["isc"], a["tot"], a["ws"], a["wsn"], None)
    for bad in (dict(B=0), dict(I=0), dict(I=8193), dict(S=1025), dict(D=0), dict(D=129), dict(ldx=2), dict(n=0), dict(n=65), dict(ps=-1.0),
                dict(wsn=need - 1), dict(ws=C.c_void_p(0x1008)), dict(ws=None), dict(off=None), dict(U=None), dict(sim=None), dict(gm=None),
                dict(Y=None), dict(R=None), dict(isum=None), dict(isc=None), dict(tot=None), dict(x=None), dict(ga=None), dict(po=None),
                dict(F=-1), dict(F=1 << 31)):
        assert call_acc(**bad) == -1, bad
        assert L.last_error().startswith("ktf_ivector"), L.last_error()
    w2 = lib.ktf_ivector_acc2_workspace_bytes
    assert w2(100, 8, 4) > 0 and w2(0, 8, 4) > 0
    for args in ((-1, 8, 4), (100, 0, 4), (100, 8193, 4), (100, 8, 0), (100, 8, 65), ((1 << 31) // 4, 8, 4)):
        assert w2(*args) == -1, args
    sec = lib.ktf_ivector_acc_second_order
    need2 = w2(10, 8, 4)
    b2 = dict(x=_p(), F=10, D=3, ldx=3, ga=_p(1), po=_p(2), n=4, ps=1.0, I=8, S2=_p(3), ws=_p(4), wsn=need2)

    def call_sec(**kw):
        a = dict(b2, **kw)
        return sec(a["x"], a["F"], a["D"], a["ldx"], a["ga"], a["po"], a["n"], a["ps"], a["I"], a["S2"], a["ws"], a["wsn"], None)
    for bad in (dict(D=0), dict(D=129), dict(ldx=2), dict(n=0), dict(n=65), dict(I=0), dict(I=8193), dict(ps=-0.5), dict(S2=None),
                dict(ws=None), dict(ws=C.c_void_p(0x1010)), dict(wsn=need2 - 1), dict(x=None), dict(ga=None), dict(po=None), dict(F=-1)):
        assert call_sec(**bad) == -1, bad
        assert L.last_error().startswith("ktf_ivector_acc"), L.last_error()
    assert call_sec(F=0, x=None, ga=None, po=None) == 0           # nothing to do, nothing launched
    atb = lib.ktf_atb_f64
    ok = dict(A=_p(), lda=8, B=_p(1), ldb=5, C=_p(2), ldc=5, M=8, N=5, K=3)

    def call_atb(**kw):
        a = dict(ok, **kw)
        return atb(a["A"], a["lda"], a["B"], a["ldb"], a["C"], a["ldc"], a["M"], a["N"], a["K"], None)
    for bad in (dict(M=0), dict(N=0), dict(K=-1), dict(lda=7), dict(ldb=4), dict(ldc=4), dict(A=None), dict(B=None), dict(C=None),
                dict(M=(1 << 22) + 1, lda=1 << 23), dict(N=(1 << 21) + 1, ldb=1 << 22, ldc=1 << 22)):
        assert call_atb(**bad) == -1, bad
        assert L.last_error().startswith("ktf_atb_f64")
    assert call_atb(K=0, A=None, B=None) == 0


def test_layer_rejects_training_misuse_without_gpu(tmp_path):
    rng = np.random.default_rng(27)
    (wt, mi, iv), (M, sig) = R.random_models(rng, 4, 3, 5)
    ubm = str(tmp_path / "final.dubm")
    R.write_diag_gmm(ubm, wt, mi, iv)
    model = IvecExtractorModel(M, sig, 100.0)
    with pytest.raises(NotImplementedError):
        ktf.training.IvectorStats(IvecExtractorModel(M, sig, 100.0, w=rng.standard_normal((4, 5))))
    st = ktf.training.IvectorStats(model)
    other = ktf.training.IvectorStats(IvecExtractorModel(M[:, :, :4], sig, 100.0))
    with pytest.raises(ValueError):
        st.merge(other)
    layer = ktf.layers.IvectorExtractor(model, ubm)
    with pytest.raises(ValueError):
        layer.accumulate(st, torch.zeros((1, 4, 3)))    # not on a GPU
    h = st.host()
    assert h["num_ivectors"] == 0 and h["R"].shape == (4, 15) and h["ivector_scatter"].shape == (5, 5)
