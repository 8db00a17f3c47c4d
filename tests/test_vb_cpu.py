"""CPU half of the VB-HMM resegmentation: the fp64 oracle (_vb_ref) against facts that do not come from it (path enumeration, the
monotone bound, a planted-speaker recording), the host helpers frame_labels / frame_rttm on hand-written cases, and the rejected
inputs of the C-ABI and of VBResegmenter, which are refused before any launch and so need no GPU."""

import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import _vb_ref as V
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L
from kaldi_tflite_amd.io import DiagGmmModel, IvecExtractorModel

PLANTED = dict(seed=7, I=8, D=6, R=4, K=3, T=1500)          # the case of test_gpu_vb's loop test


@pytest.mark.parametrize("T,K,lp", [(1, 1, 0.9), (1, 3, 0.5), (2, 2, 0.9), (4, 3, 0.99), (6, 3, 0.5), (6, 2, 0.0), (5, 3, 1.0)])
def test_forward_backward_equals_path_enumeration(T, K, lp):
    rng = np.random.default_rng(100 * T + K)
    lls = rng.standard_normal((T, K)) * 3.0
    sp = rng.dirichlet(np.full(K, 2.0))
    q, tll, spn = V.forward_backward(lls, sp, lp)
    qb, tb, spb = V.brute_force(lls, sp, lp)
    assert np.abs(q - qb).max() < 1e-12 and abs(tll - tb) < 1e-12 * max(1.0, abs(tb))
    assert np.abs(spn - spb).max() < 1e-12                          # the sp update: the enumerated re-entry probabilities
    assert np.abs(q.sum(1) - 1.0).max() < 1e-12 and abs(spn.sum() - 1.0) < 1e-12 and (spn >= 0).all()


@functools.lru_cache(maxsize=None)
def planted_case():
    c = PLANTED
    (w, mi, iv), M, x, truth = V.planted(c["seed"], c["I"], c["D"], c["R"], c["K"], c["T"])
    rng = np.random.default_rng(1)
    lab = truth.copy()
    bad = rng.random(c["T"]) < 0.2
    lab[bad] = rng.integers(0, c["K"], int(bad.sum()))
    return (w, mi, iv), M, x, truth, lab


def test_bound_never_decreases():
    (w, mi, iv), M, x, truth, lab = planted_case()
    x = x[:400]
    m, _, B, UU = V.consts(mi, iv, M)
    g, p, G, _, over = V.posteriors(x, V.gconsts(w, mi, iv), mi, iv, PLANTED["I"], 1.0, 1.0, 0.0)
    assert over == 0
    q0 = np.random.default_rng(0).gamma(100.0, size=(400, 3))
    _, _, bound = V.run(x, g, p, G, m, B, UU, q0 / q0.sum(1, keepdims=True), np.full(3, 1 / 3), max_iters=8, epsilon=-np.inf)
    assert len(bound) == 8
    for a, b in zip(bound, bound[1:]):
        assert b - a >= -1e-9 * abs(a), bound


def test_planted_speakers_are_recovered():
    (w, mi, iv), M, x, truth, lab = planted_case()
    K, T = PLANTED["K"], PLANTED["T"]
    assert 0.1 < (lab != truth).mean() < 0.2                       # 20 % corrupted, a third of them by their own label
    m, _, B, UU = V.consts(mi, iv, M)
    g, p, G, _, _ = V.posteriors(x, V.gconsts(w, mi, iv), mi, iv, 8, 1.0, 1.0, 1e-3)
    q, sp, bound = V.run(x, g, p, G, m, B, UU, V.init_q(lab, T, 1, K), np.full(K, 1.0 / K), max_iters=10)
    assert (q.argmax(1) == truth).mean() >= 0.95
    # the GPU loop test excuses frames whose two largest q are within 1e-5: the oracle alone stays under its 1 % cap
    q3, _, _ = V.run(x, g, p, G, m, B, UU, V.init_q(lab, T, 1, K), np.full(K, 1.0 / K), max_iters=3)
    s = np.sort(q3, 1)
    assert (s[:, -1] - s[:, -2] <= 1e-5).mean() <= 0.01


def test_init_q_and_blocks():
    q = V.init_q(np.array([0, 1, 1, 5, 2, -1, 2]), 7, 3, 3)
    assert q.shape == (3, 3) and np.array_equal(q[0], [1, 0, 0]) and np.allclose(q[1], 1 / 3) and np.array_equal(q[2], [0, 0, 1])


def _res(windows, R, shift=0.01):
    return types.SimpleNamespace(windows=torch.as_tensor(np.asarray(windows, np.int32)), lengths=[sum(1 for w in windows if w[0] == r) for r in range(R)],
                                 frame_shift=shift)


def test_frame_labels_midpoint_rule():
    # recording 0: windows [0, 150) and [75, 225) overlap -> cut at 112.5; [300, 400) stands apart; recording 1 has no window
    res = _res([[0, 0, 150], [0, 75, 225], [0, 300, 400]], 2)
    out = ktf.diarization.frame_labels(res, [1, 2, 1], [420, 5])
    assert len(out) == 2 and out[0].shape == (420,) and (out[1] == -1).all()
    want = np.full(420, -1)
    want[:113], want[113:225], want[300:400] = 0, 1, 0            # frame 112 starts before 112.5, frame 113 after
    assert np.array_equal(out[0], want)
    half = ktf.diarization.frame_labels(res, [1, 2, 1], 210, frame_shift=0.02)     # coarser frames of the caller
    assert np.array_equal(half[0][:58], [0] * 57 + [1]) and half[0][112] == 1 and half[0][113] == -1 and half[0][150] == 0 and half[0][200] == -1
    with pytest.raises(ValueError):
        ktf.diarization.frame_labels(res, [1, 2], [420, 5])
    with pytest.raises(ValueError):
        ktf.diarization.frame_labels(res, [1, 2, 1], [420])


def test_frame_rttm_merges_runs():
    labels = [0, 0, 1, 1, 1, -1, 0, 2, 2]
    lines = ktf.diarization.frame_rttm(labels, [0, 7, 7, 9], reco_ids=["a", "b", "c"])
    assert lines == ["SPEAKER a 1 0.000 0.020 <NA> <NA> 1 <NA> <NA>", "SPEAKER a 1 0.020 0.030 <NA> <NA> 2 <NA> <NA>",
                     "SPEAKER a 1 0.060 0.010 <NA> <NA> 1 <NA> <NA>", "SPEAKER c 1 0.000 0.020 <NA> <NA> 3 <NA> <NA>"]
    # a mask dropped frames 2 .. 9 of the first recording: the run of label 0 is cut there
    lines = ktf.diarization.frame_rttm([0, 0, 0, 0], [0, 4], frame_index=[0, 1, 10, 11], channel=2)
    assert lines == ["SPEAKER reco0 2 0.000 0.020 <NA> <NA> 1 <NA> <NA>", "SPEAKER reco0 2 0.100 0.020 <NA> <NA> 1 <NA> <NA>"]
    with pytest.raises(ValueError):
        ktf.diarization.frame_rttm(labels, [0, 7, 8])
    with pytest.raises(ValueError):
        ktf.diarization.frame_rttm(labels, [0, 9], frame_index=[0, 1])


def test_vb_abi_argument_validation_without_gpu():
    lib = L.load()
    buf = (C.c_double * 64)()
    ws = C.c_void_p(256)                                            # aligned, never dereferenced: every call below is refused first
    assert lib.ktf_vb_post_workspace_bytes(10, 0) == -1 and "Gaussians" in L.last_error()
    rc = lib.ktf_vb_post_f32(buf, 4, 5, 5, buf, buf, 8, 65, 1.0, 1.0, 0.001, buf, buf, buf, buf, ws, 1 << 20, None)
    assert rc == -1 and "num_slots" in L.last_error()
    rc = lib.ktf_vb_post_f32(buf, 4, 5, 5, buf, buf, 8, 4, 1.0, 1.0, -0.5, buf, buf, buf, buf, ws, 1 << 20, None)
    assert rc == -1 and "sparsity_thr" in L.last_error()
    rc = lib.ktf_vb_post_f32(buf, 4, 5, 5, buf, buf, 8, 4, 1.0, 1.0, 0.001, buf, buf, buf, buf, ws, 16, None)
    assert rc == -1 and "workspace" in L.last_error()
    rc = lib.ktf_vb_speaker_stats(buf, 4, 5, 5, buf, buf, 1, 4, 0, buf, 3, buf, buf, 8, buf, buf, 3, buf, buf, None)
    assert rc == -1 and "downsample" in L.last_error()
    rc = lib.ktf_vb_speaker_stats(buf, 4, 5, 5, buf, buf, 1, 4, 1, buf, 3, buf, buf, 8, buf, buf, 17, buf, buf, None)
    assert rc == -1 and "speakers" in L.last_error()
    rc = lib.ktf_vb_speaker_stats(buf, 4, 5, 5, buf, buf, 1, 9, 1, buf, 3, buf, buf, 8, buf, buf, 3, buf, buf, None)
    assert rc == -1 and "blocks" in L.last_error()
    assert lib.ktf_vb_update_workspace_bytes(3, 8, 5, 1025) == -1 and "i-vector dim" in L.last_error()
    rc = lib.ktf_vb_speaker_update(buf, buf, 3, 8, 5, 4, buf, buf, buf, buf, buf, buf, buf, C.c_void_p(264), 1 << 30, None)
    assert rc == -1 and "aligned" in L.last_error()
    rc = lib.ktf_vb_block_loglike(buf, 4, 129, 129, buf, buf, 1, 4, 1, buf, buf, 3, 8, buf, buf, buf, 3, buf, None)
    assert rc == -1 and "feature dim" in L.last_error()
    rc = lib.ktf_vb_forward_backward(buf, buf, 1, 4, 17, buf, 0.9, buf, buf, buf, ws, 1 << 20, None)
    assert rc == -1 and "speakers" in L.last_error()
    rc = lib.ktf_vb_forward_backward(buf, buf, 1, 4, 3, buf, 1.5, buf, buf, buf, ws, 1 << 20, None)
    assert rc == -1 and "loop_prob" in L.last_error()
    rc = lib.ktf_vb_forward_backward(buf, None, 1, 4, 3, buf, 0.9, buf, buf, buf, ws, 1 << 20, None)
    assert rc == -1 and "null" in L.last_error()
    rc = lib.ktf_vb_forward_backward_serial(buf, buf, 1, 4, 17, buf, 0.9, buf, buf, buf, ws, 1 << 20, None)
    assert rc == -1 and "speakers" in L.last_error()
    rc = lib.ktf_vb_forward_backward_serial(buf, buf, 1, 4, 3, buf, 0.9, buf, buf, buf, ws, 16, None)
    assert rc == -1 and "workspace" in L.last_error()
    assert lib.ktf_vb_loglike_sums(buf, buf, 0, 4, buf, None) == -1 and "recordings" in L.last_error()
    assert lib.ktf_vb_bound(buf, buf, None, 1, 3, 0.2, buf, None) == -1 and "null" in L.last_error()
    with pytest.raises(ValueError):
        L.check(rc, "x")
    assert L.VB_FB_CHUNK == 128 and L.VB_MAX_SPEAKERS == 16 and lib.ktf_version() == 117


def test_resegmenter_rejects_bad_configuration():
    rng = np.random.default_rng(3)
    (w, mi, iv), M = V.random_model(rng, 4, 3, 2)
    ubm = DiagGmmModel(w, mi, iv)
    ie = IvecExtractorModel(M, np.stack([np.eye(3)] * 4), 0.0)
    ktf.diarization.VBResegmenter(ie, ubm)
    for kw in (dict(max_speakers=17), dict(max_speakers=0), dict(num_slots=65), dict(downsample=0), dict(loop_prob=1.5),
               dict(loop_prob=-0.1), dict(sparsity_thr=1.0), dict(stat_scale=0.0), dict(max_iters=0)):
        with pytest.raises(ValueError):
            ktf.diarization.VBResegmenter(ie, ubm, **kw)
    with pytest.raises(NotImplementedError):
        ktf.diarization.VBResegmenter(ie, ubm, min_dur=2)
    (w2, mi2, iv2), _ = V.random_model(rng, 5, 3, 2)
    with pytest.raises(ValueError):
        ktf.diarization.VBResegmenter(ie, DiagGmmModel(w2, mi2, iv2))
