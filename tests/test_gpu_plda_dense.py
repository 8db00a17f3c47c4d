"""Dense PLDA scoring with conversation-dependent PCA (PLDA.score_dense, ktf_plda_dense_*) on the MI355X: Kaldi's with-PCA golden,
the fp64 NumPy restatement (tests/_plda_dense_ref.py) on random recordings across the eigensolver's LDS / global and the
Gram / covariance switches, batching, the no-PCA path against PLDA.call, and the edge rules."""

import numpy as np
import pytest
import torch

import _golden as G
import _plda_dense_ref as P
import kaldi_tflite_amd as ktf

pytestmark = pytest.mark.gpu
Ls = ktf.layers
NP = {torch.float64: np.float64, torch.float32: np.float32}


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def model(D, seed=31):
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
    return rng.standard_normal(D) * 0.1, T, np.sort(rng.uniform(0.05, 30.0, D))[::-1].copy()


def recording(seed, n, D):
    """A few speaker centroids plus noise with a decaying spectrum, rows length-normalised to sqrt(D)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    scales = 0.985 ** np.arange(D)
    cent = rng.standard_normal((4, D)) * scales * 3.0
    x = (cent[rng.integers(0, 4, n)] + rng.standard_normal((n, D)) * scales) @ q.T
    return x * (np.sqrt(D) / np.linalg.norm(x, axis=1, keepdims=True))


def well_posed(x, target, floor):
    """d is not on a knife edge: the energy fractions stay 1e-6 away from the target and the eigengap at d is >= 1 %."""
    n, D = x.shape
    xc = x - x.mean(0)
    lam = np.linalg.eigvalsh(xc @ xc.T / n if n <= D else xc.T @ xc / n)[::-1]
    d = min(P.kaldi_pca_dim(lam, target), int(np.sum(lam > floor * lam[0])))
    frac = np.cumsum(lam) / np.sum(lam)
    return np.min(np.abs(frac[:d + 1] - target)) > 1e-6 and (d >= len(lam) or lam[d - 1] - lam[d] >= 0.01 * lam[d - 1])


def recordings(ns, D, target, floor, base):
    out = []
    for n in ns:
        seed = base + 1000 * n + D
        while not well_posed(recording(seed, n, D), target, floor):
            seed += 1
        out.append(recording(seed, n, D))
    return out


# ----------------------------------------------------------------------------- Kaldi golden
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-6), (torch.float32, 2e-5)])
def test_score_dense_reproduces_kaldi_with_pca_golden(dtype, tol):
    z, g = G.load("plda.npz"), G.load("plda_dense.npz")
    p = ktf.io.KaldiPldaReader(G.GOLDEN + "/plda.bin", True)
    layer = Ls.PLDA(512, p.mean, p.transformMat, p.psi, dtype=dtype)
    s = layer.score_dense(z["plda_input"], target_energy=float(g["target_energy"]))
    assert tuple(s.shape) == (29, 29) and s.dtype == dtype
    assert layer.last_dense_dims.cpu().tolist() == [2]
    assert G.rmse(g["plda_dense_scores"], host(s)) <= tol           # (the reference's own PLDA bar is 2e-4, plda_test.py:30)
    # one recording among others: the same block
    blocks = layer.score_dense(np.concatenate([z["plda_input"][:7], z["plda_input"]]), lengths=[7, 29])
    assert torch.equal(blocks[1], s) and layer.last_dense_dims.cpu().tolist()[1] == 2


# ----------------------------------------------------------------------------- against the restatement
NS = [2, 3, 17, 29, 128, 129, 300, 512, 513, 800]           # 128 / 129: the LDS limit of the eigensolver; 512 / 513: Gram / covariance


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D", [128, 512])
@pytest.mark.parametrize("target", [0.1, 0.5, 0.9])
def test_score_dense_matches_restatement(dtype, D, target):
    floor = P.RANK_FLOOR[NP[dtype]]
    mean, T, psi = model(D)
    xs = [x.astype(NP[dtype]) for x in recordings(NS, D, target, floor, base=7)]
    layer = Ls.PLDA(D, mean, T, psi, dtype=dtype)
    got = layer.score_dense(np.concatenate(xs), lengths=[len(x) for x in xs], target_energy=target)
    dims = layer.last_dense_dims.cpu().tolist()
    lim = 1e-8 if dtype == torch.float64 else 1e-4
    pm, pT, pp = (np.asarray(a, NP[dtype]) for a in (mean, T, psi))      # the parameters as the layer holds them
    for x, s, d in zip(xs, got, dims):
        want, wd = P.score_dense(x, pm, pT, pp, target, floor)
        assert d == wd, (len(x), d, wd)
        assert tuple(s.shape) == want.shape
        err = np.abs(host(s) - want).max()
        assert err <= lim * max(1.0, np.abs(want).max()), (len(x), d, err)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D", [30, 150])
@pytest.mark.parametrize("target", [0.1, 0.9])
def test_score_dense_matches_restatement_off_the_tile_edges(dtype, D, target):
    # D and the row counts around it are no multiples of the 32-wide moment tile: covariance mode (n > D) with a partly filled
    # tile of P, Gram mode (n <= D) with a partly filled K = D, as dense scoring after an LDA to 150 has them
    ns = [2, D - 1, D, D + 1, 2 * D + 3]
    floor = P.RANK_FLOOR[NP[dtype]]
    mean, T, psi = model(D)
    xs = [x.astype(NP[dtype]) for x in recordings(ns, D, target, floor, base=7)]
    layer = Ls.PLDA(D, mean, T, psi, dtype=dtype)
    got = layer.score_dense(np.concatenate(xs), lengths=ns, target_energy=target)
    dims = layer.last_dense_dims.cpu().tolist()
    lim = 1e-8 if dtype == torch.float64 else 1e-4
    pm, pT, pp = (np.asarray(a, NP[dtype]) for a in (mean, T, psi))      # the parameters as the layer holds them
    for x, s, d in zip(xs, got, dims):
        want, wd = P.score_dense(x, pm, pT, pp, target, floor)
        assert d == wd, (len(x), d, wd)
        assert tuple(s.shape) == want.shape
        err = np.abs(host(s) - want).max()
        assert err <= lim * max(1.0, np.abs(want).max()), (len(x), d, err)


# ----------------------------------------------------------------------------- batching and the no-PCA path
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_batched_blocks_equal_separate_calls_bit_for_bit(dtype):
    D = 128
    mean, T, psi = model(D, seed=4)
    layer = Ls.PLDA(D, mean, T, psi, dtype=dtype)
    xs = [recording(50 + i, n, D) for i, n in enumerate([5, 140, 2, 1, 64, 17, 300])]
    alone, d_alone = [], []
    for x in xs:
        alone.append(layer.score_dense(x, target_energy=0.5).clone())
        d_alone.append(int(layer.last_dense_dims.item()))
    for order in ([0, 1, 2, 3, 4, 5, 6], [6, 3, 0, 5, 1, 4, 2]):
        got = layer.score_dense(np.concatenate([xs[i] for i in order]), lengths=[len(xs[i]) for i in order], target_energy=0.5)
        assert layer.last_dense_dims.cpu().tolist() == [d_alone[i] for i in order]
        for k, i in enumerate(order):
            assert torch.equal(got[k], alone[i]), (order, i)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("simple", [False, True])
def test_no_pca_blocks_are_plda_call_bit_for_bit(dtype, simple):
    D = 512
    mean, T, psi = model(D, seed=9)
    layer = Ls.PLDA(D, mean, T, psi, dtype=dtype, simple_length_norm=simple, return_transformed=False)
    xs = [recording(70 + i, n, D) for i, n in enumerate([33, 1, 200, 64, 65])]
    got = layer.score_dense(np.concatenate(xs), lengths=[len(x) for x in xs], target_energy=None)
    assert layer.last_dense_dims.cpu().tolist() == [0] * len(xs)
    for x, s in zip(xs, got):
        assert torch.equal(s, layer(x))
    one = layer.score_dense(xs[0], target_energy=None)
    assert torch.equal(one, layer(xs[0]))


# ----------------------------------------------------------------------------- edge rules
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_edge_rules(dtype):
    D = 128
    mean, T, psi = model(D, seed=11)
    floor = P.RANK_FLOOR[NP[dtype]]
    pm, pT, pp = (np.asarray(a, NP[dtype]) for a in (mean, T, psi))
    layer = Ls.PLDA(D, mean, T, psi, dtype=dtype, return_transformed=False)
    rng = np.random.default_rng(12)
    one = recording(13, 1, D)
    pair = recording(14, 2, D)
    same = np.tile(recording(15, 1, D), (10, 1))
    # three exact centroids at equal distances and equal counts (a repeated eigenvalue) plus tiny noise
    q, _ = np.linalg.qr(rng.standard_normal((D, 3)))
    trio = np.repeat(q.T * 4.0, 20, axis=0) + rng.standard_normal((60, D)) * 1e-7
    xs = [one, pair, same, trio]
    got = layer.score_dense(np.concatenate(xs).astype(NP[dtype]), lengths=[len(x) for x in xs], target_energy=0.9)
    dims = layer.last_dense_dims.cpu().tolist()
    assert dims[:3] == [0, 1, 0]                                   # rank 0, Kaldi's d = 2 clamped to the rank 1, rank 0
    assert torch.equal(got[0], layer(one.astype(NP[dtype])))       # scored without PCA: PLDA.call's bits
    assert torch.equal(got[2], layer(same.astype(NP[dtype])))
    lim = 1e-8 if dtype == torch.float64 else 1e-4
    for x, s, d in zip(xs, got, dims):
        want, wd = P.score_dense(x.astype(NP[dtype]), pm, pT, pp, 0.9, floor)
        assert d == wd
        assert np.abs(host(s) - want).max() <= lim * max(1.0, np.abs(want).max())
    assert dims[3] == 2


def test_more_than_one_call_shape_on_one_layer():
    # the per-stream workspace grows and re-slices between calls of different sizes
    D = 64
    mean, T, psi = model(D, seed=21)
    layer = Ls.PLDA(D, mean, T, psi)
    for ns in ([40], [3, 90, 7], [2]):
        xs = [recording(90 + n, n, D) for n in ns]
        got = layer.score_dense(np.concatenate(xs), lengths=ns, target_energy=0.5)
        for x, s in zip(xs, got):
            want, _ = P.score_dense(x, mean, T, psi, 0.5)
            assert np.abs(host(s) - want).max() <= 1e-8 * max(1.0, np.abs(want).max())
