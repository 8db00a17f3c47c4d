"""CPU half of VBx: the NumPy oracle (_vbx_ref) checks itself on a planted recording -- the ELBO never falls, it
converges, the surplus speakers die out, zero-padded speakers change nothing -- and the host logic of ktf.diarization.VBx (the start
from labels, label compaction, from_plda, argument validation) is exercised without a kernel."""

import functools
import inspect

import numpy as np
import pytest
import torch

import _golden as G
import _vbx_ref as X
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L
from kaldi_tflite_amd.diarization import VBx, vbx_init, vbx_labels


# ------------------------------------------------------------------------------------------------ the oracle
@functools.lru_cache(maxsize=None)
def planted_run(K):
    """planted(1, D=30, K=4, T=300, seg=12) started at 6 speakers from the true labels modulo 6, 25 % of them replaced at random,
    in the first 6 of K columns, with the defaults."""
    phi, x, truth = X.planted(1, 30, 4, 300, 12)
    lab = X.noisy_start(truth, 6, 0.25, 4)
    return (truth,) + X.run(x, phi, *X.init(lab, K))


def test_oracle_elbo_never_falls_and_converges():
    _, gamma, pi, elbo = planted_run(6)
    steps = np.diff(elbo)
    print(f"vbx oracle: {len(elbo)} iterations, smallest ELBO step {steps.min():.2e}")
    assert (steps >= 0).all() and len(elbo) < 40


def test_oracle_finds_the_planted_speakers():
    truth, gamma, pi, elbo = planted_run(6)
    labels, count = X.labels_of(gamma)
    purity = sum(np.bincount(truth[labels == c]).max() for c in np.unique(labels)) / truth.size
    top = np.sort(gamma, 1)
    close = float((top[:, -1] - top[:, -2] <= 1e-5).mean())
    print(f"vbx oracle: {count} speakers, purity {purity:.4f}, share of windows with a top-two margin <= 1e-5: {close:.4f}")
    assert count == 4 and purity == 1.0 and close == 0.0


def test_oracle_padded_speakers_change_nothing():
    """Zero-padded to K = 16. (_vb_ref.forward_backward normalises pi with np.sum, which adds 16 numbers in blocks of 8 and 6 in a
    row, so the last bit of pi can depend on the padding for other starts; with this one the sums agree.)"""
    _, gamma, pi, elbo = planted_run(6)
    _, g16, p16, e16 = planted_run(16)
    assert np.isfinite(g16).all() and np.isfinite(p16).all() and np.isfinite(e16).all()
    assert len(e16) == len(elbo) and np.abs(np.array(e16) - np.array(elbo)).max() == 0
    assert np.abs(g16[:, :6] - gamma).max() == 0 and np.abs(p16[:6] - pi).max() == 0
    assert not g16[:, 6:].any() and not p16[6:].any()


# ------------------------------------------------------------------------------------------------ start from labels
def test_init_from_labels_matches_the_oracle_rule():
    lab = np.array([7, 7, 3, 9, 3, 7, 2, 2, 2, 5])
    gamma, pi = vbx_init(lab, [0, 6, 6, 10], 4, 5.0)
    g0, p0 = X.init(lab[:6], 4)
    g2, p2 = X.init(lab[6:], 4)
    assert np.array_equal(gamma[:6], g0) and np.array_equal(pi[0], p0) and np.array_equal(gamma[6:], g2) and np.array_equal(pi[2], p2)
    # recording 0: labels 3, 7, 9 -> columns 0, 1, 2; column 3 unused
    e = np.exp(5.0)
    assert np.allclose(gamma[0], [1 / (e + 2), e / (e + 2), 1 / (e + 2), 0]) and gamma[2, 0] == e / (e + 2) and not gamma[:6, 3].any()
    assert pi[0].tolist() == [1 / 3, 1 / 3, 1 / 3, 0] and pi[2].tolist() == [0.5, 0.5, 0, 0]
    assert np.allclose(gamma.sum(1), 1)
    # torch labels as agglomerative_cluster returns them, and smoothing 0: uniform over the recording's own columns
    gamma, _ = vbx_init(torch.as_tensor(lab, dtype=torch.int32), [0, 10], 16, 0.0)
    assert np.allclose(gamma[:, :5], 0.2) and not gamma[:, 5:].any()


def test_init_keeps_the_largest_clusters():
    # sizes: label 1 x3, 4 x2, 6 x2, 8 x1, 9 x3 -> K = 3 keeps 1, 9 and, of the tie 4 / 6, the lower label 4
    lab = np.array([9, 1, 4, 6, 8, 1, 9, 4, 6, 1, 9])
    gamma, pi = vbx_init(lab, [0, 11], 3, 5.0)
    e = np.exp(5.0)
    hot, cold = e / (e + 2), 1 / (e + 2)
    col = {1: 0, 4: 1, 9: 2}
    for t, l in enumerate(lab):
        want = [1 / 3] * 3 if l not in col else [hot if k == col[l] else cold for k in range(3)]
        assert np.allclose(gamma[t], want), (t, l)
    assert pi[0].tolist() == [1 / 3] * 3


def test_init_rejects_bad_labels():
    with pytest.raises(ValueError):
        vbx_init(np.zeros(4, np.int64), [0, 5], 3, 5.0)
    with pytest.raises(ValueError):
        vbx_init(np.zeros(5), [0, 5], 3, 5.0)


# ------------------------------------------------------------------------------------------------ labels and counts
def test_label_compaction_and_counts():
    gamma = torch.tensor([[0.1, 0.2, 0.7, 0.0], [0.5, 0.0, 0.5, 0.0], [0.0, 0.0, 0.1, 0.9],       # recording 0: columns 2, 0, 3
                          [0.0, 1.0, 0.0, 0.0], [0.0, 0.6, 0.4, 0.0],                             # recording 2: column 1 only
                          [0.25, 0.25, 0.25, 0.25]], dtype=torch.float64)                          # recording 3: a full tie
    labels, counts = vbx_labels(gamma, [0, 3, 3, 5, 6])
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32
    assert labels.tolist() == [2, 1, 3, 1, 1, 1] and counts.tolist() == [3, 0, 1, 1]
    want, k = X.labels_of(gamma[:3].numpy())
    assert want.tolist() == labels[:3].tolist() and k == 3
    labels, counts = vbx_labels(torch.zeros((0, 4), dtype=torch.float64), [0, 0])
    assert labels.shape == (0,) and counts.tolist() == [0]


# ------------------------------------------------------------------------------------------------ from_plda
def _plda(psi=None, **kw):
    p = ktf.io.KaldiPldaReader(G.GOLDEN + "/plda.bin", True)       # the model of tests/golden/plda.npz
    return ktf.layers.PLDA(len(p.psi), p.mean, p.transformMat, p.psi if psi is None else psi, **kw)


def test_from_plda_takes_the_affine_transform_and_truncates():
    p = _plda(normalize_length=True, simple_length_norm=True)
    dim = p.psi.size
    assert (np.diff(p.psi) <= 0).all()                              # Kaldi writes psi in descending order
    v = VBx.from_plda(p, max_speakers=7)
    assert v.dim == v.inputDim == dim and v.maxSpeakers == 7 and np.array_equal(v.phi, p.psi.astype(np.float64))
    assert np.array_equal(v._A, p.transformMat) and np.array_equal(v._b, p.offset)
    v = VBx.from_plda(p, lda_dim=11)
    assert v.dim == 11 and v.inputDim == dim and np.array_equal(v.phi, p.psi[:11])
    assert np.array_equal(v._A[:11], p.transformMat[:11]) and not v._A[11:].any() and np.array_equal(v._b[:11], p.offset[:11])
    up = p.psi[::-1].copy()
    assert VBx.from_plda(_plda(up)).dim == dim                      # no truncation: any order is taken
    with pytest.raises(ValueError, match="descend"):
        VBx.from_plda(_plda(up), lda_dim=dim - 1)
    for bad in (0, dim + 1, 2.5, True):
        with pytest.raises(ValueError):
            VBx.from_plda(p, lda_dim=bad)


# ------------------------------------------------------------------------------------------------ validation
@pytest.mark.parametrize("kw", [dict(loop_prob=-0.01), dict(loop_prob=1.01), dict(loop_prob="x"), dict(Fa=0.0), dict(Fa=-1.0), dict(Fb=0.0),
                                dict(Fb=float("inf")), dict(max_speakers=0), dict(max_speakers=17), dict(max_speakers=2.0),
                                dict(max_iters=0), dict(max_iters=1.5), dict(epsilon=float("nan")), dict(init_smoothing=-1.0)])
def test_constructor_rejects(kw):
    with pytest.raises(ValueError):
        VBx(np.ones(4), **kw)


def test_constructor_checks_phi_and_the_transform():
    for phi in (np.zeros(3), np.array([1.0, -1.0]), np.array([1.0, np.nan]), np.array([1.0, np.inf]), np.ones((2, 2)), np.ones(0),
                np.ones(L.VBX_MAX_DIM + 1)):
        with pytest.raises(ValueError):
            VBx(phi)
    assert VBx(np.ones(L.VBX_MAX_DIM)).dim == L.VBX_MAX_DIM == 512 and L.VB_MAX_SPEAKERS == 16
    for kw in (dict(transform=np.ones((2, 5))), dict(transform=np.ones((3, 2))), dict(transform=np.ones(3)), dict(offset=np.ones(3)),
               dict(transform=np.eye(3), offset=np.ones(4)), dict(transform=np.full((3, 3), np.nan)),
               dict(transform=np.ones((3, L.PLDA_DENSE_MAX_DIM + 1)))):
        with pytest.raises(ValueError):
            VBx(np.ones(3), **kw)
    v = VBx(np.ones(3), transform=np.ones((3, 5)), loop_prob=0.0, max_speakers=16)
    assert (v.dim, v.inputDim, v.maxSpeakers, v.maxIters, v.epsilon, v.Fa, v.Fb, v.initSmoothing) == (3, 5, 16, 40, 1e-6, 0.3, 17.0, 5.0)
    assert VBx(np.ones(3)).loopProb == 0.99 and VBx(np.ones(3)).maxSpeakers == 10


def test_call_checks_its_inputs_before_any_launch():
    v = VBx(np.ones(3), max_speakers=2)
    with pytest.raises(ValueError, match="GPU"):
        v(torch.zeros((4, 3)), [4])
    with pytest.raises(ValueError):
        v(np.zeros((4, 3)), [4])
    off = np.array([0, 3, 4])
    for kw in (dict(init_labels=[0, 1, 0, 1], gamma0=np.full((4, 2), 0.5)), dict(init_labels=[0, 1, 0, 1], pi0=[0.5, 0.5]),
               dict(init_labels=[0, 1, 0]), dict(gamma0=np.full((4, 3), 0.5)), dict(gamma0=np.full((4, 2), -0.5)),
               dict(pi0=[0.5, 0.6]), dict(pi0=[[0.5, 0.5]] * 3), dict(pi0=[1.5, -0.5])):
        with pytest.raises(ValueError):
            v._start(off, kw.get("init_labels"), kw.get("gamma0"), kw.get("pi0"), 0)
    g, p = v._start(off, None, None, None, 3)
    want = np.random.default_rng(3).gamma(1.0, size=(4, 2))
    assert np.array_equal(g, want / want.sum(1, keepdims=True)) and np.array_equal(p, np.full((2, 2), 0.5))
    g, p = v._start(off, None, np.full((4, 2), 0.5), [0.25, 0.75], 0)
    assert np.array_equal(p, [[0.25, 0.75]] * 2)


def test_diarize_takes_a_vbx():
    sig = inspect.signature(ktf.diarization.diarize)
    assert "vbx" in sig.parameters and sig.parameters["vbx"].default is None
    with pytest.raises(ValueError, match="VBx"):
        ktf.diarization.diarize(None, None, None, vbx="not one")
    d = ktf.diarization.Diarization(None, None, None, [])
    assert d.ahc_labels is None and d.vbx is None
