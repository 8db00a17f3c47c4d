"""CPU half of the full-covariance posterior stage and add-deltas: the <FullGMM> reader against the writer, toDiag and the
gconsts against the oracle, checks of the oracle that do not come from the oracle, the delta coefficients, the C-ABI argument checks
that run before any launch, and the share of well-posed frames of every configuration the GPU test uses."""

import ctypes as C

import numpy as np
import pytest

import _fgmm_ref as G
import _ivector_ref as R
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L
from kaldi_tflite_amd.io import KaldiDiagGmmReader, KaldiFullGmmReader


def test_full_gmm_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    (w, mic, ic), _ = G.random_full_ubm(rng, 7, 5)
    for with_gconsts in (True, False):
        path = str(tmp_path / f"final_{int(with_gconsts)}.ubm")
        G.write_full_gmm(path, w, mic, ic, gconsts=np.full(7, 9.0, np.float32), with_gconsts=with_gconsts)
        r = KaldiFullGmmReader(path)
        assert (r.numGauss, r.featDim) == (7, 5)
        assert np.array_equal(r.weights, w) and np.array_equal(r.means_invcovars, mic)
        assert r.inv_covars.dtype == np.float32 and np.array_equal(r.inv_covars, ic)        # full symmetric
        if with_gconsts:
            assert np.array_equal(r.storedGconsts, np.full(7, 9.0, np.float32))              # kept, not trusted
        else:
            assert r.storedGconsts is None
        assert r.gconsts.dtype == np.float32
        assert np.array_equal(r.gconsts, G.gconsts(w, mic, ic).astype(np.float32))
    assert ktf.io.KaldiFullGmmReader is KaldiFullGmmReader


def test_full_gmm_value_errors(tmp_path):
    rng = np.random.default_rng(2)
    (w, mic, ic), _ = G.random_full_ubm(rng, 4, 3)
    bad = ic.copy()
    bad[2] = -bad[2]                                                                         # not positive definite
    p = str(tmp_path / "npd.ubm")
    G.write_full_gmm(p, w, mic, bad)
    with pytest.raises(ValueError):
        KaldiFullGmmReader(p)
    p = str(tmp_path / "weights.ubm")
    G.write_full_gmm(p, w[:3], mic, ic)                                                      # 3 weights, 4 Gaussians
    with pytest.raises(ValueError):
        KaldiFullGmmReader(p)
    p = str(tmp_path / "dim.ubm")
    G.write_full_gmm(p, w, mic, ic[:, :2, :2])                                               # 2 x 2 matrices, feature dim 3
    with pytest.raises(ValueError):
        KaldiFullGmmReader(p)
    p = str(tmp_path / "short.ubm")
    G.write_full_gmm(p, w[:3], mic[:3], ic[:3])
    with open(p, "rb") as f:
        data = f.read()
    (tmp_path / "four.ubm").write_bytes(data.replace(R._vec(w[:3], np.float32), R._vec(w, np.float32))
                                        .replace(R._mat(mic[:3], np.float32), R._mat(mic, np.float32)))   # 4 declared, 3 matrices
    with pytest.raises(ValueError):
        KaldiFullGmmReader(str(tmp_path / "four.ubm"))
    with pytest.raises(NotImplementedError):
        KaldiFullGmmReader(p, binary=False)


def test_to_diag_matches_oracle(tmp_path):
    rng = np.random.default_rng(3)
    (w, mic, ic), _ = G.random_full_ubm(rng, 11, 6)
    p = str(tmp_path / "final.ubm")
    G.write_full_gmm(p, w, mic, ic)
    d = KaldiFullGmmReader(p).toDiag()
    assert isinstance(d, KaldiDiagGmmReader) and (d.numGauss, d.featDim) == (11, 6)
    ww, mi, iv = G.to_diag(w, mic, ic)
    assert np.array_equal(d.weights, w)
    np.testing.assert_allclose(d.inv_vars, iv, rtol=2e-7, atol=0)                           # fp32 rounding of the fp64 values
    np.testing.assert_allclose(d.means_invvars, mi, rtol=2e-7, atol=1e-9)
    assert d.gconsts.dtype == np.float32 and np.array_equal(d.gconsts, d.computeGconsts())
    # a diagonal full UBM gives back its own diagonal
    dg = np.zeros((3, 4, 4), np.float32)
    ivs = rng.uniform(0.5, 2.0, (3, 4)).astype(np.float32)
    dg[:, np.arange(4), np.arange(4)] = ivs
    _, mi2, iv2 = G.to_diag(np.full(3, 1 / 3), np.ones((3, 4)), dg)
    np.testing.assert_allclose(iv2, ivs, rtol=1e-12)
    np.testing.assert_allclose(mi2, np.ones((3, 4)), rtol=1e-12)


def test_oracle_diagonal_covariances_give_the_diagonal_oracle():
    rng = np.random.default_rng(4)
    I, D = 9, 5
    (w, mi, iv), _ = R.random_models(rng, I, D, 2)
    ic = np.zeros((I, D, D))
    ic[:, np.arange(D), np.arange(D)] = iv
    gc = G.gconsts(w, mi, ic)
    x = rng.standard_normal((13, D))
    sel = np.tile(np.arange(I, dtype=np.int32), (13, 1))
    got = G.loglikes_on(x, (gc, mi, ic), sel)
    mean = mi.astype(np.float64) / iv
    dgc = np.log(w.astype(np.float64)) - 0.5 * D * np.log(2 * np.pi) + np.sum(0.5 * np.log(iv.astype(np.float64)) - 0.5 * mean * mean * iv, axis=1)
    np.testing.assert_allclose(got, R.loglikes(x, (dgc, mi, iv)), rtol=1e-12, atol=1e-12)


def test_oracle_is_bayes_rule_on_gaussian_densities():
    rng = np.random.default_rng(5)
    I, D = 6, 4
    (w, mic, ic), (mean, cov) = G.random_full_ubm(rng, I, D)
    # the model the fp32 fields define: Sigma = inv(inv_covars), mu = Sigma means_invcovars
    cov = np.linalg.inv(ic.astype(np.float64))
    mu = np.einsum("ide,ie->id", cov, mic.astype(np.float64))
    x = G.draw_frames(rng, mean, cov, 20).astype(np.float64)
    dens = np.zeros((20, I))
    for i in range(I):
        d = x - mu[i]
        dens[:, i] = w[i] * np.exp(-0.5 * np.einsum("fd,de,fe->f", d, np.linalg.inv(cov[i]), d)) / np.sqrt((2 * np.pi) ** D * np.linalg.det(cov[i]))
    want = dens / dens.sum(1, keepdims=True)
    sel = np.tile(np.arange(I, dtype=np.int32), (20, 1))
    g, p, _ = G.posteriors(x, (G.gconsts(w, mic, ic), mic, ic), sel, 0.0)
    for t in range(20):
        assert np.all(np.diff(p[t]) <= 0) and sorted(g[t].tolist()) == list(range(I))
        np.testing.assert_allclose(p[t][np.argsort(g[t])], want[t], rtol=1e-9, atol=1e-300)


def test_prune_rule_by_hand():
    idx = np.array([7, 3, 5, -1])
    ll = np.log(np.array([0.5, 0.3, 0.2, 1.0]))
    g, p, pre = G.prune(idx, ll, 0.0)
    assert g.tolist() == [7, 3, 5]
    np.testing.assert_allclose(p, [0.5, 0.3, 0.2], rtol=1e-15)
    g, p, pre = G.prune(idx, ll, 0.25)                                        # 0.2 dropped, the rest renormalised by 0.8
    assert g.tolist() == [7, 3]
    np.testing.assert_allclose(p, [0.625, 0.375], rtol=1e-15)
    np.testing.assert_allclose(pre, [0.5, 0.3, 0.2], rtol=1e-15)
    g, p, _ = G.prune(np.array([9, 4, 6, 8]), np.zeros(4), 0.3)               # all 0.25 < 0.3: the arg-max (lowest index) gets 1
    assert g.tolist() == [4] and p.tolist() == [1.0]
    g, p, _ = G.prune(np.array([2, 1]), np.array([0.0, -1e4]), 0.0)           # an exact zero is dropped, min_post or not
    assert g.tolist() == [2] and p.tolist() == [1.0]
    g, p, _ = G.prune(np.array([5, 2, 9]), np.array([1.0, 1.0, 0.0]), 0.0)    # ties: the lower index first
    assert g.tolist() == [2, 5, 9]
    g, p, _ = G.prune(np.array([-1, -1]), np.zeros(2), 0.025)                 # nothing listed
    assert len(g) == 0 and len(p) == 0


def test_delta_coefficients():
    f = np.float32
    s = G.delta_coeffs(1, 2)
    assert np.array_equal(s[1], np.array([-2, -1, 0, 1, 2], f) / f(10))
    s = G.delta_coeffs(2, 2)
    np.testing.assert_allclose(s[2], np.convolve(s[1].astype(np.float64), s[1].astype(np.float64)), rtol=1e-6, atol=1e-9)
    for order, window in ((0, 2), (1, 2), (2, 2), (2, 3), (3, 1)):
        got = ktf.layers.AddDeltas.coefficients(order, window)
        want = G.delta_coeffs(order, window)
        ow = order * window
        assert got.dtype == f and got.shape == (order + 1, 2 * ow + 1)
        for i in range(order + 1):
            assert np.array_equal(got[i, ow - i * window:ow + i * window + 1], want[i])
            assert not got[i, :ow - i * window].any() and not got[i, ow + i * window + 1:].any()
    # edge clamping: one frame -> every delta is s * x summed = 0 up to rounding; two frames by hand
    x = np.array([[[1.0], [3.0]]], f)
    out = G.add_deltas(x, None, 1, 2)
    c = s[1]
    assert out[0, 0, 0] == 1.0 and out[0, 1, 0] == 3.0
    np.testing.assert_allclose(out[0, 0, 1], (c[0] + c[1]) * 1 + (c[3] + c[4]) * 3, rtol=1e-6)       # taps -2, -1 clamp to frame 0
    np.testing.assert_allclose(out[0, 1, 1], (c[0] + c[1]) * 1 + (c[3] + c[4]) * 3, rtol=1e-6)       # taps +1, +2 clamp to frame 1
    assert abs(out[0, 0, 1] - 0.6) < 1e-6
    one = G.add_deltas(np.array([[[2.5]]], f), None, 2, 2)
    assert one[0, 0, 0] == 2.5 and abs(one[0, 0, 1]) < 1e-6 and abs(one[0, 0, 2]) < 1e-6
    assert not G.add_deltas(x, [1], 1, 2)[0, 1].any()                         # beyond the length: zeros


def test_add_deltas_layer_configuration():
    for kw in (dict(order=-1), dict(window=0), dict(order=11, window=3), dict(order=1.5)):
        with pytest.raises(ValueError):
            ktf.layers.AddDeltas(**kw)
    with pytest.raises(TypeError):
        ktf.layers.AddDeltas(windw=3)                                          # a misspelt argument is not swallowed
    layer = ktf.layers.AddDeltas(2, 3)
    cfg = layer.get_config()
    assert (cfg["order"], cfg["window"]) == (2, 3)
    again = ktf.layers.AddDeltas.from_config(cfg)
    assert (again.order, again.window) == (2, 3)
    assert ktf.layers.AddDeltas().get_config()["window"] == 2
    assert layer.compute_output_shape([4, 100, 20]) == [4, 100, 60]


def _p(n=0):
    return C.c_void_p(0x1000 + 256 * n) if n >= 0 else None


def test_cabi_rejects_bad_arguments_without_gpu():
    lib = L.load()
    wsb = lib.ktf_fgmm_workspace_bytes
    assert wsb(100, 8, 3, 5) > 0 and wsb(0, 8, 3, 5) > 0
    assert wsb(200, 8, 3, 5) >= wsb(100, 8, 3, 5)
    for args in ((-1, 8, 3, 5), (100, 0, 3, 5), (100, 8193, 3, 5), (100, 8, 0, 5), (100, 8, 129, 5), (100, 8, 3, 0), (100, 8, 3, 65),
                 ((1 << 31) // 5 + 1, 8, 3, 5)):
        assert wsb(*args) == -1, args
        assert L.last_error().startswith("ktf_fgmm_workspace_bytes")
    post = lib.ktf_fgmm_post_f32
    need = wsb(10, 8, 3, 4)
    ok = dict(x=_p(), F=10, D=3, ldx=3, sel=_p(1), n=4, mic=_p(2), ic=_p(3), gc=_p(4), I=8, mp=0.025, ga=_p(5), po=_p(6), ws=_p(7), wsn=need)

    def call(**kw):
        a = dict(ok, **kw)
        return post(a["x"], a["F"], a["D"], a["ldx"], a["sel"], a["n"], a["mic"], a["ic"], a["gc"], a["I"], a["mp"], a["ga"], a["po"],
                    a["ws"], a["wsn"], None)
    for bad in (dict(D=0), dict(D=129), dict(ldx=2), dict(I=0), dict(I=8193), dict(n=0), dict(n=65), dict(mp=1.0), dict(mp=-0.1),
                dict(F=-1), dict(x=None), dict(sel=None), dict(mic=None), dict(ic=None), dict(gc=None), dict(ga=None), dict(po=None),
                dict(ws=None), dict(wsn=need - 1), dict(ws=C.c_void_p(0x1008))):
        assert call(**bad) == -1, bad
        assert L.last_error().startswith("ktf_fgmm"), (bad, L.last_error())
    assert call(F=0, x=None, ws=None, wsn=0) == 0                              # nothing to do, nothing launched
    dl = lib.ktf_add_deltas_f32
    okd = dict(x=_p(), B=2, T=5, D=3, sb=15, st=3, n=_p(1), c=_p(2), order=2, window=2, out=_p(3))

    def calld(**kw):
        a = dict(okd, **kw)
        return dl(a["x"], a["B"], a["T"], a["D"], a["sb"], a["st"], a["n"], a["c"], a["order"], a["window"], a["out"], None)
    for bad in (dict(order=-1), dict(window=0), dict(order=11, window=3), dict(D=0), dict(B=-1), dict(T=-1), dict(st=2), dict(x=None),
                dict(c=None), dict(out=None)):
        assert calld(**bad) == -1, bad
        assert L.last_error().startswith("ktf_add_deltas_f32")
    assert calld(B=0, x=None) == 0 and calld(T=0, out=None) == 0


def _files(tmp_path, rng, I=4, D=3, S=5):
    (wt, mi, iv), (M, sig) = R.random_models(rng, I, D, S)
    (w, mic, ic), _ = G.random_full_ubm(rng, I, D)
    ie, dubm, ubm = str(tmp_path / "final.ie"), str(tmp_path / "final.dubm"), str(tmp_path / "final.ubm")
    R.write_ivector_extractor(ie, M, sig, 100.0)
    R.write_diag_gmm(dubm, wt, mi, iv)
    G.write_full_gmm(ubm, w, mic, ic)
    return ie, dubm, ubm


def test_layer_takes_a_full_ubm(tmp_path):
    rng = np.random.default_rng(6)
    ie, dubm, ubm = _files(tmp_path, rng)
    with pytest.raises(ValueError):
        ktf.layers.IvectorExtractor(ie)                                         # neither UBM
    a = ktf.layers.IvectorExtractor(ie, dubm, full_ubm=ubm)
    b = ktf.layers.IvectorExtractor(ie, full_ubm=KaldiFullGmmReader(ubm))
    c = ktf.layers.IvectorExtractor(ie, KaldiFullGmmReader(ubm).toDiag(), full_ubm=ubm)
    assert np.array_equal(b._W, c._W) and np.array_equal(b._gconst, c._gconst) and not np.array_equal(a._W, b._W)
    assert a._full[1].shape == (4, 3, 3) and a._full[1].dtype == np.float32
    assert ktf.layers.IvectorExtractor(ie, dubm)._full is None
    other = str(tmp_path / "other.ubm")
    (w, mic, ic), _ = G.random_full_ubm(rng, 6, 3)
    G.write_full_gmm(other, w, mic, ic)
    with pytest.raises(ValueError):
        ktf.layers.IvectorExtractor(ie, dubm, full_ubm=other)                   # 6 Gaussians against 4
    with pytest.raises(ValueError):
        ktf.layers.IvectorExtractor(ie, full_ubm=other)
    wsb = L.load().ktf_fgmm_workspace_bytes
    assert wsb(a._frame_step(), 4, 3, 20) <= 1 << 30 < wsb(a._frame_step() + 1, 4, 3, 20)
    huge = ktf.layers.IvectorExtractor(ie, dubm, full_ubm=ubm, workspace_limit=1 << 40)
    assert huge._frame_step() == ((1 << 31) - 1) // 20                          # the entry point's own limit: F * n < 2^31
    small = ktf.layers.IvectorExtractor(ie, dubm, full_ubm=ubm, workspace_limit=1 << 16)
    step = small._frame_step()
    assert 1 <= step < 1 << 16
    assert wsb(step, 4, 3, 20) <= 1 << 16 < wsb(step + 1, 4, 3, 20)


@pytest.mark.parametrize("k", range(len(G.CONFIGS)))
def test_well_posed_share(k):
    """At most 10 % of a configuration's frames may be left out of the GPU comparison, and at least 300 must remain."""
    *_, ok = G.config_case(k)
    left_out = 1.0 - ok.mean()
    print(f"config {G.CONFIGS[k]}: {100 * left_out:.1f} % of {G.FRAMES} frames left out")
    assert left_out <= 0.10, left_out
    assert ok.sum() >= 300


def test_well_posed_share_of_the_skewed_and_whole_call_cases():
    """The same cap for the two further configurations of the GPU tests."""
    *_, sel, ok = G.popular_case()
    counts = np.bincount(sel[sel >= 0], minlength=G.POPULAR[0])
    print(f"skewed case: {100 * (1 - ok.mean()):.1f} % left out, {counts[3]} pairs on Gaussian 3, {(counts == 0).sum()} empty Gaussians")
    assert 1.0 - ok.mean() <= 0.10 and ok.sum() >= 300
    assert counts[3] == G.POPULAR_FRAMES and (counts == 0).sum() >= 1
    *_, ok = G.whole_call_case()
    print(f"whole-call pool: {100 * (1 - ok.mean()):.1f} % left out")
    assert 1.0 - ok.mean() <= 0.10 and ok.sum() >= max(300, sum(G.WHOLE_LENS))
