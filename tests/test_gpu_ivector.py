"""i-vector extraction on the MI355X (ktf_ivector_post_f32, ktf_ivector_extract, ktf.layers.IvectorExtractor) against the fp64 NumPy
restatement (tests/_ivector_ref.py): stats to solve on supplied posteriors, posteriors on well-posed frames, the whole chain, the
15 Kaldi dummy extractors, mask / lengths, bit stability across runs and batch composition, and PLDA scoring of the output."""

import os

import numpy as np
import pytest
import torch

import _ivector_ref as R
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd.io import KaldiDiagGmmReader, KaldiIvecExtractorReader

pytestmark = pytest.mark.gpu
DUMMIES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ivector_extractor")
DEV = "cuda:0"


def files(tmp_path, rng, I, D, S, tag="m", prior_offset=100.0):
    (w, mi, iv), (M, sig) = R.random_models(rng, I, D, S, prior_offset=prior_offset)
    ie, ubm = str(tmp_path / f"{tag}.ie"), str(tmp_path / f"{tag}.dubm")
    R.write_ivector_extractor(ie, M, sig, prior_offset)
    R.write_diag_gmm(ubm, w, mi, iv)
    return KaldiIvecExtractorReader(ie), KaldiDiagGmmReader(ubm)


def ubm_frames(rng, ubm, n):
    """Frames drawn from the UBM itself (a random component, its mean and variance): realistic posteriors."""
    mean = ubm.means_invvars.astype(np.float64) / ubm.inv_vars
    c = rng.integers(0, ubm.numGauss, n)
    return (mean[c] + rng.standard_normal((n, ubm.featDim)) / np.sqrt(ubm.inv_vars[c])).astype(np.float32)


def batch(rng, ubm, lens):
    T = max(max(lens), 1)
    x = np.zeros((len(lens), T, ubm.featDim), np.float32)
    for b, n in enumerate(lens):
        x[b, :n] = ubm_frames(rng, ubm, n)
    return x


def oracle_ivectors(ie, x, lens, g, p, off, **scales):
    sim, U = np.asarray(ie.sigmaInvM), ie.U
    out = []
    for b, n in enumerate(lens):
        lo, hi = off[b], off[b + 1]
        gamma, F = R.stats(x[b, :n], g[lo:hi], p[lo:hi], ie.numGauss, **scales)
        out.append(R.extract_packed(gamma, F, sim, U, ie.priorOffset))
    return np.array(out)


def random_posts(rng, I, lens, n):
    F = int(sum(lens))
    g = np.full((F, n), -1, np.int32)
    p = np.zeros((F, n), np.float32)
    for t in range(F):
        k = int(rng.integers(1, min(n, I) + 1))
        g[t, :k] = rng.choice(I, k, replace=False)
        q = rng.uniform(0.01, 1.0, k)
        p[t, :k] = np.sort(q / q.sum())[::-1]
    return g, p


@pytest.mark.parametrize("I,D,S", [(37, 24, 4), (2048, 60, 100), (37, 24, 400), (2, 2, 600)])
def test_from_posteriors_matches_oracle(tmp_path, I, D, S):
    rng = np.random.default_rng(I * 7 + D * 3 + S)
    ie, ubm = files(tmp_path, rng, I, D, S)
    layer = ktf.layers.IvectorExtractor(ie, ubm, num_gselect=5)
    lens = [0, 1, 57, 200, 3]
    x = batch(rng, ubm, lens)
    g, p = random_posts(rng, I, lens, 5)
    off = np.concatenate([[0], np.cumsum(lens)])
    kw = dict(posterior_scale=0.5, acoustic_weight=1.0, max_count=60.0)
    layer.posteriorScale, layer.maxCount = kw["posterior_scale"], kw["max_count"]
    want = oracle_ivectors(ie, x, lens, g, p, off, **kw)
    xd = torch.as_tensor(x, device=DEV)
    got64 = layer.from_posteriors(xd, torch.as_tensor(g, device=DEV), torch.as_tensor(p, device=DEV), lengths=lens,
                                  dtype=torch.float64).cpu().numpy()
    got32 = layer.from_posteriors(xd, torch.as_tensor(g, device=DEV), torch.as_tensor(p, device=DEV), lengths=lens).cpu().numpy()
    scale = np.abs(want).max()
    assert np.array_equal(got64[0], np.zeros(S)) and np.array_equal(got32[0], np.zeros(S))
    assert np.abs(got64 - want).max() <= 1e-8 * scale, np.abs(got64 - want).max() / scale
    assert np.abs(got32 - want).max() <= 2e-7 * scale, np.abs(got32 - want).max() / scale
    assert got32.dtype == np.float32 and np.array_equal(got32, got64.astype(np.float32))


@pytest.mark.parametrize("name", [f"dummy_{i:03d}" for i in range(1, 16)])
def test_kaldi_dummy_extractors_end_to_end(tmp_path, name):
    ie = KaldiIvecExtractorReader(os.path.join(DUMMIES, name, "final.ie"))
    rng = np.random.default_rng(int(name[-3:]))
    (w, mi, iv), _ = R.random_models(rng, ie.numGauss, ie.featDim, 2)
    R.write_diag_gmm(str(tmp_path / "u.dubm"), w, mi, iv)
    ubm = KaldiDiagGmmReader(str(tmp_path / "u.dubm"))
    layer = ktf.layers.IvectorExtractor(ie, ubm, num_gselect=3, min_post=0.025)
    lens = [40, 0, 7]
    x = batch(rng, ubm, lens)
    xd = torch.as_tensor(x, device=DEV)
    g, p, off = layer.posteriors(xd, lengths=lens)
    want = oracle_ivectors(ie, x, lens, g.cpu().numpy(), p.cpu().numpy(), off.cpu().numpy())
    got = layer(xd, lengths=lens, dtype=torch.float64).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max()
    assert np.array_equal(got[1], np.zeros(ie.ivecDim))


@pytest.mark.parametrize("I,D", [(2047, 24), (37, 60)])
@pytest.mark.parametrize("n", [1, 5, 20, 50])
@pytest.mark.parametrize("min_post", [0.0, 0.025])
def test_posteriors_on_well_posed_frames(tmp_path, I, D, n, min_post):
    rng = np.random.default_rng(I + n * 13 + int(min_post * 1000))
    ie, ubm = files(tmp_path, rng, I, D, 3)
    layer = ktf.layers.IvectorExtractor(ie, ubm, num_gselect=n, min_post=min_post)
    x = ubm_frames(rng, ubm, 300)
    g, p, off = layer.posteriors(torch.as_tensor(x[None], device=DEV))
    g, p = g.cpu().numpy(), p.cpu().numpy()
    assert g.shape == (300, n) and off.cpu().tolist() == [0, 300]
    gmm = (ubm.gconsts, ubm.means_invvars, ubm.inv_vars)
    wg, wp = R.posteriors(x, gmm, n, min_post)
    ok = R.margins(x, gmm, n, min_post) >= 1e-3
    assert ok.sum() >= 100, ok.sum()
    assert np.array_equal(g[ok], wg[ok])
    assert np.abs(p[ok] - wp[ok]).max() <= 2e-5              # fp32 log-likelihoods, as Kaldi computes them
    assert np.all(p[g == -1] == 0) and np.all(g < I)          # a kept Gaussian may underflow to 0 (min_post 0 keeps it)
    if min_post == 0:
        assert np.all((g >= 0).sum(1) == min(n, I))
    np.testing.assert_allclose(p.sum(1), 1.0, atol=1e-5)
    assert np.all(np.diff(p, axis=1) <= 0)                 # sorted by posterior


def well_posed_batch(rng, ubm, lens, n, min_post):
    gmm = (ubm.gconsts, ubm.means_invvars, ubm.inv_vars)
    pool = ubm_frames(rng, ubm, 4 * sum(lens) + 64)
    pool = pool[R.margins(pool, gmm, n, min_post) >= 1e-3]
    x = np.zeros((len(lens), max(lens), ubm.featDim), np.float32)
    at = 0
    for b, k in enumerate(lens):
        x[b, :k] = pool[at:at + k]
        at += k
    assert at <= len(pool)
    return x


def test_full_call_matches_oracle(tmp_path):
    rng = np.random.default_rng(77)
    ie, ubm = files(tmp_path, rng, 64, 20, 50)
    layer = ktf.layers.IvectorExtractor(ie, ubm)
    lens = [120, 1, 0, 64]
    x = well_posed_batch(rng, ubm, lens, 20, 0.025)
    got = layer(torch.as_tensor(x, device=DEV), lengths=lens).cpu().numpy()
    gmm = (ubm.gconsts, ubm.means_invvars, ubm.inv_vars)
    gs, ps = zip(*[R.posteriors(x[b, :k], gmm, 20, 0.025) for b, k in enumerate(lens)])
    g, p = np.concatenate(gs), np.concatenate(ps)
    want = oracle_ivectors(ie, x, lens, g, p, np.concatenate([[0], np.cumsum(lens)]))
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


def test_mask_and_lengths_agree(tmp_path):
    rng = np.random.default_rng(78)
    ie, ubm = files(tmp_path, rng, 37, 24, 30)
    layer = ktf.layers.IvectorExtractor(ie, ubm)
    lens = [50, 0, 13, 64]
    x = batch(rng, ubm, lens)
    xd = torch.as_tensor(x, device=DEV)
    mask = (np.arange(64)[None] < np.array(lens)[:, None]).astype(np.float32)
    a = layer(xd, lengths=lens)
    b = layer(xd, mask=torch.as_tensor(mask[..., None], device=DEV))
    assert torch.equal(a, b)
    # a mask with holes = select-voiced-frames: the voiced frames moved to the front, counted by lengths
    holes = rng.uniform(size=(4, 64)) < 0.6
    holes[1] = False
    y = np.zeros_like(x)
    cnt = holes.sum(1)
    for i in range(4):
        y[i, :cnt[i]] = x[i, holes[i]]
    c = layer(xd, mask=torch.as_tensor(holes, device=DEV))
    d = layer(torch.as_tensor(y, device=DEV), lengths=cnt)
    assert torch.equal(c, d)
    full = layer(xd)
    assert torch.equal(full[3], a[3])                           # all 64 frames of utterance 3


def test_bits_independent_of_run_and_batch(tmp_path):
    rng = np.random.default_rng(79)
    ie, ubm = files(tmp_path, rng, 300, 24, 100)
    layer = ktf.layers.IvectorExtractor(ie, ubm)
    lens = [90, 3, 0, 150, 77]
    x = batch(rng, ubm, lens)
    xd = torch.as_tensor(x, device=DEV)
    a = layer(xd, lengths=lens, dtype=torch.float64)
    assert torch.equal(a, layer(xd, lengths=lens, dtype=torch.float64))
    order = [4, 0, 3]
    b = layer(xd[order], lengths=[lens[i] for i in order], dtype=torch.float64)
    assert torch.equal(b, a[order])
    for i in range(5):
        assert torch.equal(layer(xd[i:i + 1], lengths=[lens[i]], dtype=torch.float64)[0], a[i])
    small = ktf.layers.IvectorExtractor(ie, ubm, workspace_limit=1)   # one utterance per chunk
    assert torch.equal(small(xd, lengths=lens, dtype=torch.float64), a)


def test_ivectors_feed_plda_scoring(tmp_path):
    rng = np.random.default_rng(80)
    S = 16
    ie, ubm = files(tmp_path, rng, 32, 12, S)
    layer = ktf.layers.IvectorExtractor(ie, ubm)
    lens = [60, 40, 80]
    iv = layer(torch.as_tensor(batch(rng, ubm, lens), device=DEV), lengths=lens)
    T = rng.standard_normal((S, S)) / np.sqrt(S) + np.eye(S)
    plda = ktf.layers.PLDA(S, rng.standard_normal(S) * 0.1, T, np.sort(rng.uniform(0.1, 5.0, S))[::-1].copy())
    tr = plda.transform(iv.to(torch.float64))
    scores = plda.score_trials(tr, tr, np.array([0, 1, 2, 0]), np.array([1, 2, 0, 0]))
    assert scores.shape == (4,) and torch.isfinite(scores).all()
