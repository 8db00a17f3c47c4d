"""Full-covariance UBM posteriors on the MI355X (ktf_fgmm_post_f32, ktf.layers.IvectorExtractor(full_ubm=...)) against the fp64 NumPy
restatement (tests/_fgmm_ref.py) on well-posed frames, the toDiag() path, the whole call, bit stability across runs, batch
composition and chunking, skewed buckets, the position of a frame in the call, and the unchanged diagonal path."""

import numpy as np
import pytest
import torch

import _fgmm_ref as G
import _ivector_ref as R
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import ops
from kaldi_tflite_amd.io import KaldiFullGmmReader, KaldiIvecExtractorReader

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def readers(tmp_path, rng, stored, S, tag="m"):
    """The extractor and full-UBM readers of a random model around the stored full UBM."""
    w, mic, ic = stored
    I, D = mic.shape
    _, (M, sig) = R.random_models(rng, I, D, S)
    ie, ubm = str(tmp_path / f"{tag}.ie"), str(tmp_path / f"{tag}.ubm")
    R.write_ivector_extractor(ie, M, sig, 100.0)
    G.write_full_gmm(ubm, w, mic, ic)
    return KaldiIvecExtractorReader(ie), KaldiFullGmmReader(ubm)


def check_layout(g, p, I):
    assert np.all(p[g == -1] == 0) and np.all(g < I) and np.all(g >= -1)
    assert np.all(p[g >= 0] > 0)                                    # only Gaussians with p != 0 are listed
    used = g >= 0
    assert np.all(used[:, 1:] <= used[:, :-1])                      # unused slots follow the used ones
    np.testing.assert_allclose(p.sum(1), 1.0, atol=1e-5)
    assert np.all(np.diff(p, axis=1) <= 0)                          # sorted by posterior


@pytest.mark.parametrize("k", range(len(G.CONFIGS)))
def test_posteriors_on_well_posed_frames(tmp_path, k):
    I, D, n, min_post = G.CONFIGS[k]
    stored, diag, full, x, sel, ok = G.config_case(k)
    assert 1.0 - ok.mean() <= 0.10 and ok.sum() >= 300
    ie, fr = readers(tmp_path, np.random.default_rng(k), stored, 3)
    assert np.array_equal(fr.gconsts, full[0])
    layer = ktf.layers.IvectorExtractor(ie, full_ubm=fr, num_gselect=n, min_post=min_post)
    g, p, off = layer.posteriors(torch.as_tensor(x[None], device=DEV))
    g, p = g.cpu().numpy(), p.cpu().numpy()
    assert g.shape == (G.FRAMES, n) and off.cpu().tolist() == [0, G.FRAMES]
    wg, wp, _ = G.posteriors(x, full, sel, min_post)
    err = np.abs(p[ok] - wp[ok]).max()
    print(f"config {G.CONFIGS[k]}: {ok.sum()} well-posed frames, max |dpost| = {err:.3e}, gauss equal on "
          f"{np.all(g[ok] == wg[ok], axis=1).sum()}, kept per frame {np.mean((wg >= 0).sum(1)):.1f}")
    assert np.array_equal(g[ok], wg[ok])
    assert err <= 2e-5
    check_layout(g, p, I)
    if min_post == 0:
        assert np.all((g >= 0).sum(1) <= min(n, I))


def test_op_on_given_lists_and_empty_lists():
    """The entry point alone on lists with holes: entries outside [0, I) are skipped, an empty list gives n unused slots, and so
    does a list whose log-likelihoods are all -inf (zero-weight components)."""
    rng = np.random.default_rng(20)
    I, D, n = 50, 33, 7
    stored, (mean, cov) = G.random_full_ubm(rng, I, D)
    gc = G.gconsts(*stored).astype(np.float32)
    gc[:2] = -np.inf                                                # two components of weight zero
    full = (gc, stored[1], stored[2])
    x = G.draw_frames(rng, mean, cov, 200)
    sel = np.stack([rng.choice(I, n, replace=False) for _ in range(200)]).astype(np.int32)
    sel[rng.uniform(size=sel.shape) < 0.3] = -1
    sel[5] = -1
    sel[6, :3] = [I, I + 7, -5]
    sel[7] = [0, 1, -1, 1, -1, 0, -1]
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731
    g, p = ops.fgmm_post(d(x), d(sel), d(full[1]), d(full[2]), d(full[0]), 0.0)
    g, p = g.cpu().numpy(), p.cpu().numpy()
    wg, wp, _ = G.posteriors(x, full, sel, 0.0)
    for t in (5, 7):
        assert np.all(g[t] == -1) and np.all(p[t] == 0)
    assert np.isfinite(p).all()
    for t in range(200):
        # per Gaussian (the order of near-ties is not fixed here). With min_post 0 the kept set is p != 0, and fp32 underflows
        # where fp64 does not: the sets are compared on the Gaussians whose oracle posterior is above 1e-30
        got = dict(zip(g[t][g[t] >= 0].tolist(), p[t][g[t] >= 0].tolist()))
        want = dict(zip(wg[t][wg[t] >= 0].tolist(), wp[t][wg[t] >= 0].tolist()))
        assert set(got) <= set(want)
        assert {k for k, v in want.items() if v > 1e-30} <= set(got)
        assert all(abs(got.get(k, 0.0) - v) <= 2e-5 for k, v in want.items())


def test_to_diag_path_is_the_same_layer(tmp_path):
    rng = np.random.default_rng(21)
    stored, (mean, cov) = G.random_full_ubm(rng, 64, 20)
    ie, fr = readers(tmp_path, rng, stored, 30)
    x = torch.as_tensor(G.draw_frames(rng, mean, cov, 3 * 80).reshape(3, 80, 20), device=DEV)
    a = ktf.layers.IvectorExtractor(ie, full_ubm=fr)
    b = ktf.layers.IvectorExtractor(ie, fr.toDiag(), full_ubm=fr)
    ga, pa, _ = a.posteriors(x)
    gb, pb, _ = b.posteriors(x)
    assert torch.equal(ga, gb) and torch.equal(pa, pb)
    assert torch.equal(a(x, dtype=torch.float64), b(x, dtype=torch.float64))


def test_full_call_with_mask_matches_oracle(tmp_path):
    I, D, n, min_post = G.WHOLE
    S, lens = 50, G.WHOLE_LENS
    stored, diag, full, pool, ok = G.whole_call_case()
    assert 1.0 - ok.mean() <= 0.10 and ok.sum() >= sum(lens)
    pool = pool[ok]
    rng = np.random.default_rng(220)
    ie, fr = readers(tmp_path, rng, stored, S)
    T = 150
    mask = np.zeros((len(lens), T), bool)
    x = rng.standard_normal((len(lens), T, D)).astype(np.float32)        # unvoiced frames: anything
    at = 0
    for b, k in enumerate(lens):
        mask[b, rng.choice(T, k, replace=False)] = True
        x[b, mask[b]] = pool[at:at + k]
        at += k
    layer = ktf.layers.IvectorExtractor(ie, fr.toDiag(), full_ubm=fr)
    got = layer(torch.as_tensor(x, device=DEV), mask=torch.as_tensor(mask, device=DEV)).cpu().numpy()
    sim, U = np.asarray(ie.sigmaInvM), ie.U
    want = []
    for b in range(len(lens)):
        xb = x[b, mask[b]]
        sel = G.gselect(xb, (diag.gconsts, diag.means_invvars, diag.inv_vars), n) if len(xb) else np.zeros((0, n), np.int32)
        g, p, _ = G.posteriors(xb, full, sel, min_post)
        gamma, F = R.stats(xb, g, p, I)
        want.append(R.extract_packed(gamma, F, sim, U, ie.priorOffset))
    want = np.array(want)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"whole call: max |d ivector| / max |ivector| = {err:.3e}")
    assert err <= 1e-5
    assert np.array_equal(got[2], np.zeros(S))


def test_bits_independent_of_run_batch_and_chunks(tmp_path):
    rng = np.random.default_rng(23)
    I, D = 300, 24
    stored, (mean, cov) = G.random_full_ubm(rng, I, D)
    ie, fr = readers(tmp_path, rng, stored, 40)
    layer = ktf.layers.IvectorExtractor(ie, full_ubm=fr)
    lens = [90, 3, 0, 150, 77]
    x = np.zeros((5, 150, D), np.float32)
    for b, k in enumerate(lens):
        x[b, :k] = G.draw_frames(rng, mean, cov, k)
    xd = torch.as_tensor(x, device=DEV)
    a = layer(xd, lengths=lens, dtype=torch.float64)
    g, p, off = layer.posteriors(xd, lengths=lens)
    assert torch.equal(a, layer(xd, lengths=lens, dtype=torch.float64))
    g2, p2, _ = layer.posteriors(xd, lengths=lens)
    assert torch.equal(g, g2) and torch.equal(p, p2)
    order = [4, 0, 3]
    b = layer(xd[order], lengths=[lens[i] for i in order], dtype=torch.float64)
    assert torch.equal(b, a[order])
    off = off.cpu().numpy()
    for i in range(5):
        assert torch.equal(layer(xd[i:i + 1], lengths=[lens[i]], dtype=torch.float64)[0], a[i])
        gi, pi, _ = layer.posteriors(xd[i:i + 1], lengths=[lens[i]])
        assert torch.equal(gi, g[off[i]:off[i + 1]]) and torch.equal(pi, p[off[i]:off[i + 1]])
    limit = ops.fgmm_workspace_bytes(50, I, D, 20)                   # 50 frames per chunk: utterances are cut, too
    small = ktf.layers.IvectorExtractor(ie, full_ubm=fr, workspace_limit=limit)
    assert small._frame_step() < 90
    gs, ps, _ = small.posteriors(xd, lengths=lens)
    assert torch.equal(gs, g) and torch.equal(ps, p)
    assert torch.equal(small(xd, lengths=lens, dtype=torch.float64), a)


def test_one_popular_gaussian_and_empty_ones(tmp_path):
    """All frames drawn from component 3: its bucket holds every frame (several work items), most others hold nothing."""
    I, D, n, min_post = G.POPULAR
    stored, diag, full, x, sel, ok = G.popular_case()
    counts = np.bincount(sel[sel >= 0], minlength=I)
    assert counts[3] == G.POPULAR_FRAMES and (counts == 0).sum() >= 1
    assert 1.0 - ok.mean() <= 0.10 and ok.sum() >= 300
    ie, fr = readers(tmp_path, np.random.default_rng(24), stored, 3)
    assert np.array_equal(fr.gconsts, full[0])
    layer = ktf.layers.IvectorExtractor(ie, fr.toDiag(), full_ubm=fr, num_gselect=n, min_post=min_post)
    g, p, _ = layer.posteriors(torch.as_tensor(x[None], device=DEV))
    g, p = g.cpu().numpy(), p.cpu().numpy()
    wg, wp, _ = G.posteriors(x, full, sel, min_post)
    assert np.array_equal(g[ok], wg[ok])
    assert np.abs(p[ok] - wp[ok]).max() <= 2e-5
    check_layout(g, p, I)


def test_bits_independent_of_frame_position():
    """A frame's posteriors and log-likelihood do not depend on where the frame sits in the call, so not on the order of the pairs
    inside a bucket either: the same frames permuted give the same rows, permuted. 90 % of the frames come from component 2, whose
    bucket spans three 512-row work items; Gaussian 5 is never listed; a few list entries are -1 or outside [0, I)."""
    rng = np.random.default_rng(26)
    I, D, n, F = 6, 33, 3, 1500
    stored, (mean, cov) = G.random_full_ubm(rng, I, D)
    gc = G.gconsts(*stored).astype(np.float32)
    comp = np.where(rng.uniform(size=F) < 0.9, 2, rng.integers(0, I - 1, F))
    x = G.draw_frames(rng, mean, cov, F, comp=comp)
    sel = np.stack([rng.choice(I - 1, n, replace=False) for _ in range(F)]).astype(np.int32)
    sel[(comp == 2) & ~(sel == 2).any(1), 0] = 2
    sel[rng.choice(F, 12, replace=False), rng.integers(0, n, 12)] = np.tile(np.array([-1, I, I + 3, -7], np.int32), 3)
    sel[17] = -1
    counts = np.bincount(sel[(sel >= 0) & (sel < I)], minlength=I)
    assert 2 * 512 < counts[2] <= 3 * 512 and counts[5] == 0
    perm = rng.permutation(F)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731
    model = (d(stored[1]), d(stored[2]), d(gc), 0.025)
    g, p, ll = ops.fgmm_post_ll(d(x), d(sel), *model)
    g2, p2, ll2 = ops.fgmm_post_ll(d(x[perm]), d(sel[perm]), *model)
    at = torch.as_tensor(perm, device=DEV)
    assert (g >= 0).any(1).sum().item() == F - 1 and torch.isfinite(ll).all()
    assert torch.equal(g2, g[at]) and torch.equal(p2, p[at]) and torch.equal(ll2, ll[at])


def test_without_full_ubm_nothing_changes(tmp_path):
    rng = np.random.default_rng(25)
    (w, mi, iv), (M, sig) = R.random_models(rng, 37, 24, 10)
    ie, ubm = str(tmp_path / "d.ie"), str(tmp_path / "d.dubm")
    R.write_ivector_extractor(ie, M, sig, 100.0)
    R.write_diag_gmm(ubm, w, mi, iv)
    layer = ktf.layers.IvectorExtractor(ie, ubm)
    x = torch.as_tensor(rng.standard_normal((2, 70, 24)).astype(np.float32), device=DEV)
    g, p, _ = layer.posteriors(x)
    W, gc = layer._consts(x.device)[:2]
    g0, p0 = ops.ivector_post(x.reshape(-1, 24), W, gc, 20, 0.025)
    assert torch.equal(g, g0) and torch.equal(p, p0)
    assert torch.equal(layer(x), layer.from_posteriors(x, g0, p0))
