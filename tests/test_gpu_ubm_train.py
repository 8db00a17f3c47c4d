"""GPU half of UBM training against the fp64 oracle (_ubm_train_ref): the EM statistics of ktf_gmm_acc_f64 on
supplied posteriors (so that no selection can flip), the three E-steps with their frame log-likelihoods, the three loops, the
writer round trip into IvectorExtractor and the rejected inputs.

Bounds: an fp64 accumulator is within 1e-8 of its array's largest magnitude of the oracle (the bound of test_gpu_ivector_train);
posteriors within 1e-5 absolute (the bound of test_gpu_fgmm); a frame log-likelihood, and every quantity of an EM loop, within 8 x
the gap between the oracle with fp64 and with float32 log-likelihoods, measured in the test (the factor covers another summation
order at the same error scale). The measured figures are printed (pytest -s) and recorded in INTEGRATION.md §2i."""

import functools

import numpy as np
import pytest
import torch

import _fgmm_ref as FR
import _ubm_train_ref as U
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L
from kaldi_tflite_amd import ops, training
from kaldi_tflite_amd.io import DiagGmmModel, FullGmmModel, KaldiFullGmmReader, WriteKaldiFullGmm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
R = L.GMM_ACC_ITEM_ROWS
# (D, I, n, F): ragged against the 16-wide tile and the 4-row K-step; the last sends most pairs to one Gaussian (>= 3 items)
SHAPES = [(5, 8, 3, 203), (15, 8, 3, 203), (16, 33, 4, 1001), (40, 6, 2, 3 * R + 7)]


def d(a):
    return torch.as_tensor(np.array(a), device=DEV)          # a copy: the cached cases are read-only


@functools.lru_cache(maxsize=None)
def stats_case(k):
    """Frames, slots and the oracle's statistics (both forms) of shape k: computed once, never modified."""
    D, I, n, F = SHAPES[k]
    rng = np.random.default_rng(700 + k)
    x = (rng.standard_normal((F, D)) * 1.3 + rng.standard_normal(D) * 0.5).astype(np.float32)
    gauss = rng.integers(0, I - 1, (F, n)).astype(np.int32)              # Gaussian I - 1: nobody selects it
    if k == 3:
        gauss[rng.random((F, n)) < 0.72] = 0
    post = rng.uniform(0.05, 1.0, (F, n)).astype(np.float32)
    gauss[rng.choice(F, 5, replace=False), rng.integers(0, n, 5)] = -1   # a few unused slots ...
    gauss[rng.choice(F, 2, replace=False), 0] = I + 3                    # ... and indices beyond I
    post[rng.choice(F, 6, replace=False), rng.integers(0, n, 6)] = 0.0   # a few zero weights
    if k == 3:
        assert (gauss == 0).sum() >= 2 * F * n / 3 and (gauss == 0).sum() > 2 * R
    for a in (x, gauss, post):
        a.setflags(write=False)
    return x, gauss, post, {full: U.stats_on_pairs(x, gauss, post, I, full) for full in (False, True)}


def run_acc(x, gauss, post, I, full, acc=None):
    D = x.shape[1]
    if acc is None:
        z = lambda *s: torch.zeros(s, dtype=torch.float64, device=DEV)  # noqa: E731
        acc = (z(I), z(I, D), z(I, D, D) if full else z(I, D))
    ops.gmm_acc(d(x), d(gauss), d(post), *acc)
    return acc


def worst(got, want):
    return max(float(np.abs(g.cpu().numpy() - w).max() / np.abs(w).max()) for g, w in zip(got, want))


@pytest.mark.parametrize("full", [False, True], ids=["diag", "full"])
@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_statistics_on_supplied_posteriors(k, full):
    x, gauss, post, want = stats_case(k)
    D, I, n, F = SHAPES[k]
    got = run_acc(x, gauss, post, I, full)
    err = worst(got, want[full])
    print(f"gmm_acc {'full' if full else 'diag'} (D, I, n, F) = {SHAPES[k]}: worst accumulator deviation {err:.3e} (bound 1e-8)")
    assert err <= 1e-8
    assert float(got[0][I - 1]) == 0.0 and not got[2][I - 1].any()
    if full:
        assert torch.equal(got[2], got[2].transpose(1, 2))
    again = run_acc(x, gauss, post, I, full)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    h = F // 2 + 1
    two = run_acc(x[:h], gauss[:h], post[:h], I, full)
    run_acc(x[h:], gauss[h:], post[h:], I, full, two)
    err2 = worst(two, want[full])
    print(f"  ... accumulated in two calls: {err2:.3e}")
    assert err2 <= 1e-8
    if full:
        assert torch.equal(two[2], two[2].transpose(1, 2))


# ------------------------------------------------------------------ posteriors
def random_diag(rng, I, D):
    w = rng.uniform(0.5, 1.5, I)
    iv = rng.uniform(0.5, 2.0, (I, D))
    return DiagGmmModel(w / w.sum(), rng.standard_normal((I, D)) * iv, iv)


def ll_bound(l64, l32):
    gap = float(np.abs(l64 - l32.astype(np.float64)).max())
    assert gap > 0
    return gap


def test_preselect_posteriors_and_loglike():
    rng = np.random.default_rng(41)
    I, D, n, F = 33, 16, 4, 301
    g = random_diag(rng, I, D)
    x = (rng.standard_normal((F, D)) * 1.2).astype(np.float32)
    sel = U.gselect(x, g, n)
    sel = sel[:, rng.permutation(n)].copy()                  # the list's own order, not sorted
    sel[7] = -1                                              # an empty list
    sel[9, 1], sel[11, 0] = -1, I                            # skipped entries
    p64, l64, valid = U.softmax_rows(U.on_list(U.diag_loglikes(x, g), sel))
    _, l32, _ = U.softmax_rows(U.on_list(U.diag_loglikes(x, g, np.float32), sel))
    _, gc, mi, iv = training._diag_consts(g, DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    post, ll = ops.gmm_post_preselect(d(x), d(sel), mi, iv, gc, cnt)
    post, ll = post.cpu().numpy(), ll.cpu().numpy()
    gap = ll_bound(l64, l32)
    err_p, err_l = float(np.abs(post - p64).max()), float(np.abs(ll - l64).max())
    print(f"preselect: posterior deviation {err_p:.3e} (bound 1e-5), loglike deviation {err_l:.3e} (fp32 oracle gap {gap:.3e}, bound 8 x)")
    assert err_p <= 1e-5 and np.abs(post[valid].sum(1) - 1.0).max() <= 1e-5
    assert err_l <= 8 * gap
    assert int(cnt.item()) == F - 1 and not post[7].any() and ll[7] == 0.0
    assert post[9, 1] == 0.0 and post[11, 0] == 0.0
    # a frame's bits depend on its own row and list alone
    post2, ll2 = ops.gmm_post_preselect(d(x[5:40]), d(sel[5:40]), mi, iv, gc)
    assert np.array_equal(post2.cpu().numpy(), post[5:40]) and np.array_equal(ll2.cpu().numpy(), ll[5:40])


@pytest.mark.parametrize("I,D,F", [(33, 16, 70), (300, 5, 45)], ids=["one-tile", "two-tiles"])
def test_dense_posteriors_and_loglike(I, D, F):
    rng = np.random.default_rng(43 + I)
    g = random_diag(rng, I, D)
    x = (rng.standard_normal((F, D)) * 1.2).astype(np.float32)
    p64, l64, _ = U.softmax_rows(U.diag_loglikes(x, g))
    _, l32, _ = U.softmax_rows(U.diag_loglikes(x, g, np.float32))
    W, gc, _, _ = training._diag_consts(g, DEV)
    P, Xaug, ll = ops.gmm_post_dense(d(x), W, gc)
    P, Xaug, ll = P.cpu().numpy(), Xaug.cpu().numpy(), ll.cpu().numpy()
    gap = ll_bound(l64, l32)
    err_p, err_l = float(np.abs(P - p64).max()), float(np.abs(ll - l64).max())
    print(f"dense I={I}: posterior deviation {err_p:.3e} (bound 1e-5), loglike deviation {err_l:.3e} (fp32 oracle gap {gap:.3e}, bound 8 x)")
    assert err_p <= 1e-5 and np.abs(P.sum(1) - 1.0).max() <= 1e-5
    assert err_l <= 8 * gap
    x64 = x.astype(np.float64)
    assert np.array_equal(Xaug, np.concatenate([np.ones((F, 1)), x64, x64 * x64], axis=1))
    # the log-likelihoods are those of ktf_ivector_post_f32: the best Gaussian and its posterior agree with it
    gs, ps = ops.ivector_post(d(x), W, gc, 1, 0.0)
    assert np.array_equal(gs.cpu().numpy()[:, 0], P.argmax(1))


@pytest.mark.parametrize("min_post", [0.0, 0.025])
def test_fgmm_post_ll_keeps_the_bits_and_adds_the_loglike(min_post):
    rng = np.random.default_rng(47)
    I, D, n, F = 12, 24, 5, 203
    stored, (mean, cov) = FR.random_full_ubm(rng, I, D)
    g = FullGmmModel(*stored)
    x = FR.draw_frames(rng, mean, cov, F)
    sel = U.gselect(x, g.toDiag(), n)
    sel[3] = -1
    sel[8, 2] = -1
    mic, ic, gc = training._full_consts(g, DEV)
    g0, p0 = ops.fgmm_post(d(x), d(sel), mic, ic, gc, min_post)
    g1, p1, ll = ops.fgmm_post_ll(d(x), d(sel), mic, ic, gc, min_post)
    g2, p2, none = ops.fgmm_post_ll(d(x), d(sel), mic, ic, gc, min_post, want_loglike=False)
    assert none is None
    assert torch.equal(g0, g1) and torch.equal(p0, p1) and torch.equal(g0, g2) and torch.equal(p0, p2)
    _, l64, _ = U.softmax_rows(U.full_loglikes_on(x, g, sel))
    _, l32, _ = U.softmax_rows(U.full_loglikes_on(x, g, sel, np.float32))
    gap = ll_bound(l64, l32)
    err = float(np.abs(ll.cpu().numpy() - l64).max())
    print(f"fgmm_post_ll min_post={min_post}: loglike deviation {err:.3e} (fp32 oracle gap {gap:.3e}, bound 8 x)")
    assert err <= 8 * gap and float(ll[3]) == 0.0


# ------------------------------------------------------------------ EM loops
SEED, NG, NGI, ITERS, GD, GF = 17, 8, 4, 6, 6, 1500
FULL_EST = dict(min_gaussian_occupancy=20.0)


@functools.lru_cache(maxsize=None)
def em_case():
    """The data, the draws init_diag_ubm makes from default_rng(SEED) and the oracle's three loops with fp64 and with float32
    log-likelihoods (computed once, never modified)."""
    x = U.mixture(np.random.default_rng(3), 5, GD, GF)
    out = {}
    for t in (np.float64, np.float32):
        rng = np.random.default_rng(SEED)                    # F <= num_frames: no subset draw
        first = rng.choice(GF, NGI, replace=False)
        normals = (rng.standard_normal(GD) for _ in iter(int, 1))   # one draw per split, in split order
        out[t] = dict(init=U.init_diag_ubm(x, NG, NGI, ITERS, first, normals, t))
    start = out[np.float64]["init"][0]
    sel = U.gselect(x, start, 3)
    for t in (np.float64, np.float32):
        out[t]["diag"] = U.train_diag_ubm(start, x, sel, 3, t)
        out[t]["full"] = U.train_full_ubm(U.diag_to_full(out[np.float64]["diag"][0]), x, sel, 3, t, **FULL_EST)
    for stage in ("init", "diag", "full"):                   # both oracles remove and floor the same Gaussians
        assert out[np.float64][stage][2] == out[np.float32][stage][2], stage
    return x, sel, out


def check_loop(stage, model, objf, out):
    m64, o64, _ = out[np.float64][stage]
    m32, o32, _ = out[np.float32][stage]
    assert model.numGauss == m64.numGauss
    gap = dict(U.model_gap(m32, m64), objf=float(np.abs(np.array(o32) - o64).max()))
    got = dict(U.model_gap(model, m64), objf=float(np.abs(np.array(objf) - o64).max()))
    for k in ("weights", "means", "covars", "objf"):
        print(f"{stage}: {k} deviation {got[k]:.3e} (fp32 oracle gap {gap[k]:.3e}, bound 8 x)")
    for k in got:
        assert got[k] <= 8 * gap[k], (stage, k, got[k], gap[k])
    noise = gap["objf"]                                      # the error scale of a float32 frame log-likelihood
    assert all(b >= a - noise for a, b in zip(objf, objf[1:])), objf


def test_init_diag_ubm_follows_the_oracle():
    x, _, out = em_case()
    model, objf = training.init_diag_ubm(d(x)[None], NG, NGI, num_iters=ITERS, seed=SEED)
    assert isinstance(model, DiagGmmModel) and len(objf) == ITERS
    check_loop("init", model, objf, out)


def test_train_diag_ubm_follows_the_oracle():
    x, sel, out = em_case()
    model, objf = training.train_diag_ubm(out[np.float64]["init"][0], [(d(x)[None],)], num_iters=3, gselect=[d(sel)])
    check_loop("diag", model, objf, out)


def test_train_full_ubm_follows_the_oracle():
    x, sel, out = em_case()
    start = training.diag_to_full(out[np.float64]["diag"][0])
    model, objf = training.train_full_ubm(start, [(d(x)[None],)], num_iters=3, gselect=[d(sel)], **FULL_EST)
    assert isinstance(model, FullGmmModel)
    check_loop("full", model, objf, out)


def test_select_gaussians_is_gmm_gselect():
    x, _, out = em_case()
    start = out[np.float64]["init"][0]
    ll = np.sort(U.diag_loglikes(x, start), axis=1)[:, ::-1]
    clear = (ll[:, :3] - ll[:, 1:4]).min(1) > 1e-3           # frames whose ranking a float32 error cannot change
    got = training.select_gaussians(start, d(x)[None], 3).cpu().numpy()
    assert clear.sum() > GF // 2 and np.array_equal(got[clear], U.gselect(x, start, 3)[clear])
    lens = [700]
    assert np.array_equal(training.select_gaussians(start, d(x)[None], 3, lengths=lens).cpu().numpy(), got[:700])


def test_end_to_end_into_the_ivector_extractor(tmp_path):
    x, _, out = em_case()
    feats = d(x[:1200].reshape(2, 600, GD))
    full0 = training.diag_to_full(out[np.float64]["diag"][0])
    model, objf = training.train_full_ubm(full0, [(feats,), (feats[:1], [300])], gselect_n=3, num_iters=2, **FULL_EST)
    assert len(objf) == 2 and objf[1] >= objf[0] - 1e-4
    path = str(tmp_path / "final.ubm")
    WriteKaldiFullGmm(path, model)
    back = KaldiFullGmmReader(path)
    for k in ("weights", "means_invcovars", "inv_covars", "gconsts"):
        assert np.array_equal(getattr(back, k), getattr(model, k)), k
    ie = training.ivector_extractor_init(model, 5, seed=1)
    a = ktf.layers.IvectorExtractor(ie, full_ubm=model, num_gselect=3)(feats)
    b = ktf.layers.IvectorExtractor(ie, full_ubm=path, num_gselect=3)(feats)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_merge_adds_statistics():
    x, sel, out = em_case()
    g = out[np.float64]["init"][0]
    whole, a, b = (training.DiagGmmStats(g) for _ in range(3))
    training.acc_diag_gmm(whole, g, d(x)[None], d(sel))
    training.acc_diag_gmm(a, g, d(x[:800])[None], d(sel[:800]))
    training.acc_diag_gmm(b, g, d(x[800:])[None], d(sel[800:]))
    a.merge(b)
    assert a.frames == whole.frames == GF and abs(a.objf() - whole.objf()) < 1e-9
    assert worst((a.occ, a.mean_acc, a.var_acc), [t.cpu().numpy() for t in (whole.occ, whole.mean_acc, whole.var_acc)]) <= 1e-12
    # chunks under a small workspace limit: the same statistics
    c = training.DiagGmmStats(g)
    assert training.acc_diag_gmm(c, g, d(x)[None], d(sel), workspace_limit=8000) > 1
    assert worst((c.occ, c.mean_acc, c.var_acc), [t.cpu().numpy() for t in (whole.occ, whole.mean_acc, whole.var_acc)]) <= 1e-12


# ------------------------------------------------------------------ rejected inputs
def test_rejected_inputs():
    with pytest.raises(ValueError):
        ops.gmm_acc_workspace_bytes(10, 8, L.IVECTOR_MAX_FEAT_DIM + 1, 3, 1)
    with pytest.raises(ValueError):
        ops.gmm_acc_workspace_bytes(10, L.IVECTOR_MAX_GAUSS + 1, 5, 3, 0)
    with pytest.raises(ValueError):
        ops.gmm_acc_workspace_bytes(10, 8, 5, L.IVECTOR_MAX_GSELECT + 1, 0)
    with pytest.raises(ValueError):
        ops.gmm_acc_workspace_bytes(2 ** 30, 8, 5, 2, 0)     # F * n = 2^31
    assert ops.gmm_acc_workspace_bytes(2 ** 30 - 1, 8, 5, 2, 0) > 0
    with pytest.raises(ValueError):
        ops.gmm_post_dense_workspace_bytes(10, L.IVECTOR_MAX_GAUSS + 1)
    lib = L.load()
    x = torch.zeros((4, 5), device=DEV)
    sel = torch.zeros((4, 2), dtype=torch.int32, device=DEV)
    p = torch.zeros((4, 2), device=DEV)
    assert lib.ktf_gmm_post_preselect_f32(L.ptr(x), 4, 5, 4, L.ptr(sel), 2, L.ptr(x), L.ptr(x), L.ptr(x), 3, L.ptr(p), L.ptr(p), None,
                                          None) == -1       # ldx < D
    assert L.last_error().startswith("ktf_gmm_post_preselect_f32")
    rng = np.random.default_rng(1)
    g, other = random_diag(rng, 4, 5), random_diag(rng, 3, 5)
    feats = torch.zeros((1, 6, 5), device=DEV)
    with pytest.raises(ValueError):
        training.acc_diag_gmm(training.DiagGmmStats(g), g, feats, gselect=torch.zeros((5, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        training.acc_diag_gmm(training.DiagGmmStats(g), g, feats, gselect=torch.zeros((6, 65), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        training.acc_diag_gmm(training.DiagGmmStats(other), g, feats)
    with pytest.raises(ValueError):
        training.acc_full_gmm(training.DiagGmmStats(g), training.diag_to_full(g), feats, torch.zeros((6, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        training.diag_gmm_est(g, training.DiagGmmStats(other))
    with pytest.raises(ValueError):
        training.full_gmm_est(training.diag_to_full(g), training.FullGmmStats(training.diag_to_full(other)))
    with pytest.raises(ValueError):
        FullGmmModel(np.ones(1), np.zeros((1, 2)), np.array([[[1.0, 2.0], [2.0, 1.0]]]))     # not positive definite
    with pytest.raises(ValueError):
        training.select_gaussians(g, feats, L.IVECTOR_MAX_GSELECT + 1)
    with pytest.raises(ValueError):
        training.init_diag_ubm(feats, 8, 7)                  # 6 frames cannot seed 7 Gaussians
