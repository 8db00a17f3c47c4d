"""Speaker verification on the MI355X: speaker means (ktf_spk_mean_f32) bit-exact against the NumPy loop, the count-aware PLDA
transform / block / trial-list scoring against the fp64 restatement (tests/_verif_ref.py) and bit for bit against the count-free
path at n = 1, trial-list order invariance, raw x-vectors of the extractor, and verification.score end to end."""

import numpy as np
import pytest
import torch

import _golden as G
import _verif_ref as V
import synth
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import ops
from oracle import ktf_oracle as O

pytestmark = pytest.mark.gpu
Ls = ktf.layers
ver = ktf.verification


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def model(D, seed=31):
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
    return rng.standard_normal(D) * 0.1, T, np.sort(rng.uniform(0.05, 30.0, D))[::-1].copy()


def speakers(S, per, D, seed):
    """Vectors around S speaker centroids."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((S, D)) * 2.0
    return (np.repeat(c, per, axis=0) + rng.standard_normal((S * per, D))).astype(np.float64)


def tol(dtype):
    return 1e-12 if dtype == torch.float64 else 1e-5


def tol_tr(dtype):                                   # transformed vectors: a dim-long fp32 dot product per element
    return 1e-12 if dtype == torch.float64 else 5e-5


# ----------------------------------------------------------------------------- speaker means
def test_speaker_means_bit_exact():
    rng = np.random.default_rng(7)
    raw = (rng.standard_normal((40, 512)) * 3).astype(np.float32)
    d = torch.as_tensor(raw, device="cuda")
    cases = [[[0, 1, 2], [5], [7, 7, 7, 3], list(range(40)), [39]],     # one utterance, repeated indices
             [[4, 2]]]                                                   # S = 1
    for spk in cases:
        want, wn = V.ivector_mean(raw, spk)
        m, n = ver.speaker_means(d, spk)
        assert np.array_equal(m.cpu().numpy(), want) and n.cpu().numpy().tolist() == wn.tolist()
        off = np.cumsum([0] + [len(u) for u in spk])
        utt = np.concatenate(spk)
        m2, n2 = ver.speaker_means(d, (torch.as_tensor(off, device="cuda"), torch.as_tensor(utt, device="cuda")))
        assert torch.equal(m, m2) and torch.equal(n, n2)
        m3, _ = ver.speaker_means(d, (off, utt))
        assert torch.equal(m, m3)
    for bad in ([[0], []], [[0, 40]], [[-1]]):
        with pytest.raises(ValueError):
            ver.speaker_means(d, bad)
    with pytest.raises(ValueError):
        ver.speaker_means(d, (torch.tensor([0, 1, 1], device="cuda"), torch.tensor([0], device="cuda")))
    with pytest.raises(ValueError):
        ver.speaker_means(d, (torch.tensor([0, 1], device="cuda"), torch.tensor([40], device="cuda")))


# ----------------------------------------------------------------------------- PLDA with counts
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D", [128, 200])
def test_transform_and_scores_with_counts_match_restatement(dtype, D):
    mean, T, psi = model(D, seed=D)
    layer = Ls.PLDA(D, mean, T, psi, dtype=dtype)
    e = speakers(70, 1, D, seed=1)
    y = speakers(90, 1, D, seed=2)
    n = np.random.default_rng(3).integers(1, 51, size=70).astype(np.float64)
    n[:3] = [1, 50, 2]
    e_tr = layer.transform(e, num_examples=n)
    y_tr = layer.transform(y)
    want_e = V.transform(e, mean, T, psi, n)
    want_y = V.transform(y, mean, T, psi)
    assert np.abs(host(e_tr) - want_e).max() <= tol_tr(dtype) * np.abs(want_e).max()
    assert np.abs(host(y_tr) - want_y).max() <= tol_tr(dtype) * np.abs(want_y).max()
    # scores on the device's own transformed vectors (the transform's rounding is checked above)
    want = V.llr(host(y_tr), host(e_tr), psi, n)
    scale = np.abs(want).max()
    blk = layer.score(y_tr, e_tr, enroll_num_examples=n)
    assert blk.shape == (90, 70) and np.abs(host(blk) - want).max() <= tol(dtype) * scale
    rng = np.random.default_rng(4)
    tj, ti = rng.integers(0, 70, 3000), rng.integers(0, 90, 3000)
    tr = layer.score_trials(y_tr, e_tr, tj, ti, enroll_num_examples=n)
    assert tr.shape == (3000,) and np.abs(host(tr) - want[ti, tj]).max() <= tol(dtype) * scale
    # the same counts as a scalar, a device tensor and an int32 device tensor
    n_dev = torch.as_tensor(n, device="cuda")
    assert torch.equal(layer.transform(e, num_examples=n_dev), e_tr)
    assert torch.equal(layer.score(y_tr, e_tr, enroll_num_examples=n_dev.to(torch.int32)), blk)
    assert torch.equal(layer.transform(e, num_examples=3), layer.transform(e, num_examples=np.full(70, 3.0)))
    for bad in (0, -1.0, np.r_[n[:-1], 0.0], torch.as_tensor(np.r_[n[:-1], np.nan], device="cuda"), np.ones(3)):
        with pytest.raises(ValueError):
            layer.transform(e, num_examples=bad)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_golden_plda_with_pseudo_speakers(dtype):
    z = G.load("plda.npz")
    p = ktf.io.KaldiPldaReader(G.GOLDEN + "/plda.bin", True)
    x = z["plda_input"][:, 0, :].astype(np.float64)                       # the 29 golden x-vectors, 512-dim
    spk = [list(range(i, min(i + 4, 29))) for i in range(0, 29, 4)]         # 8 pseudo-speakers of 1 .. 4 rows
    means = np.stack([x[u].mean(0) for u in spk])
    n = np.array([len(u) for u in spk], np.float64)
    layer = Ls.PLDA(512, p.mean, p.transformMat, p.psi, dtype=dtype)
    e_tr = layer.transform(means, num_examples=n)
    y_tr = layer.transform(x)
    want_e = V.transform(means, p.mean, p.transformMat, p.psi, n)
    assert np.abs(host(e_tr) - want_e).max() <= tol_tr(dtype) * 10 * np.abs(want_e).max()
    want = V.llr(host(y_tr), host(e_tr), p.psi, n)
    s = layer.score(y_tr, e_tr, enroll_num_examples=n)
    assert np.abs(host(s) - want).max() <= tol(dtype) * np.abs(want).max()
    tj, ti = np.meshgrid(np.arange(8), np.arange(29))
    st = layer.score_trials(y_tr, e_tr, tj.ravel(), ti.ravel(), enroll_num_examples=n)
    assert np.abs(host(st) - want.ravel()).max() <= tol(dtype) * np.abs(want).max()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("simple", [False, True])
def test_count_one_is_the_count_free_path_bit_for_bit(dtype, simple):
    D = 160
    mean, T, psi = model(D, seed=5)
    layer = Ls.PLDA(D, mean, T, psi, dtype=dtype, simple_length_norm=simple)
    e, y = speakers(67, 1, D, seed=8), speakers(130, 1, D, seed=9)
    e_tr, y_tr = layer.transform(e), layer.transform(y)
    A, off, ps = layer._dev
    ones_e = torch.ones(67, dtype=dtype, device="cuda")
    x = torch.as_tensor(e, device="cuda").to(dtype).contiguous()
    assert torch.equal(ops.plda_transform_n(x, A, off, ps, ones_e, True, simple), e_tr)
    assert torch.equal(layer.transform(e, num_examples=1), e_tr)
    assert torch.equal(ops.plda_score_n(y_tr, e_tr, ps, ones_e), layer.score(y_tr, e_tr))
    assert torch.equal(layer.score(y_tr, e_tr, enroll_num_examples=np.ones(67)), layer.score(y_tr, e_tr))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_trial_list_order_invariance_and_edges(dtype):
    D = 128
    mean, T, psi = model(D, seed=12)
    layer = Ls.PLDA(D, mean, T, psi, dtype=dtype)
    M, N = 300, 400
    n = np.random.default_rng(13).integers(1, 51, M).astype(np.float64)
    e_tr = layer.transform(speakers(M, 1, D, 14), num_examples=n)
    y_tr = layer.transform(speakers(N, 1, D, 15))
    blk = host(layer.score(y_tr, e_tr, enroll_num_examples=n))
    rng = np.random.default_rng(16)
    Tn = 600_000                                     # > 8192 workgroups x 16 trials: the grid-stride loop turns over
    tj, ti = rng.integers(0, M, Tn).astype(np.int32), rng.integers(0, N, Tn).astype(np.int32)
    s = layer.score_trials(y_tr, e_tr, tj, ti, enroll_num_examples=n)
    perm = rng.permutation(Tn)
    sp = layer.score_trials(y_tr, e_tr, tj[perm], ti[perm], enroll_num_examples=n)
    assert torch.equal(sp, s[torch.as_tensor(perm, device="cuda")])
    assert np.abs(host(s) - blk[ti, tj]).max() <= (1e-12 if dtype == torch.float64 else 1e-5) * np.abs(blk).max()
    # device indices: the same bits
    sd = layer.score_trials(y_tr, e_tr, torch.as_tensor(tj, device="cuda"), torch.as_tensor(ti, device="cuda").long(),
                            enroll_num_examples=torch.as_tensor(n, device="cuda"))
    assert torch.equal(sd, s)
    # a single trial, and T = 0
    one = layer.score_trials(y_tr, e_tr, [tj[5]], [ti[5]], enroll_num_examples=n)
    assert one.shape == (1,) and torch.equal(one, s[5:6])
    assert layer.score_trials(y_tr, e_tr, [], [], enroll_num_examples=n).shape == (0,)
    for bad in (([M], [0]), ([0], [N]), ([-1], [0]), ([0, 1], [0])):
        with pytest.raises(ValueError):
            layer.score_trials(y_tr, e_tr, *bad, enroll_num_examples=n)
    with pytest.raises(ValueError):
        layer.score_trials(y_tr, e_tr, torch.tensor([M], device="cuda"), torch.tensor([0], device="cuda"))


def test_trials_kernel_writes_nan_for_pairs_outside_the_arrays():
    """The Python checks skipped (ops directly): an out-of-range pair scores NaN, its neighbours are unaffected."""
    D = 64
    mean, T, psi = model(D, seed=20)
    layer = Ls.PLDA(D, mean, T, psi)
    e_tr, y_tr = layer.transform(speakers(5, 1, D, 21)), layer.transform(speakers(6, 1, D, 22))
    pairs = torch.tensor([[0, 0], [5, 0], [0, 6], [-1, 2], [4, 5]], dtype=torch.int32, device="cuda")
    s = ops.plda_trials(y_tr, e_tr, layer._dev[2], torch.ones(5, dtype=torch.float64, device="cuda"), pairs)
    h = host(s)
    assert np.isnan(h[1:4]).all() and np.isfinite(h[[0, 4]]).all()
    blk = host(layer.score(y_tr, e_tr))
    assert abs(h[0] - blk[0, 0]) < 1e-12 * abs(blk).max() and abs(h[4] - blk[5, 4]) < 1e-12 * abs(blk).max()


# ----------------------------------------------------------------------------- raw x-vectors of the extractor
_ext = {}


def extractor(gemm):
    if gemm not in _ext:
        w = synth.make_weights(seed=4321)
        _ext[gemm] = (synth.build_extractor(ktf, synth.extractor_cfg(), w, gemm=gemm), w)
    return _ext[gemm]


def wavs():
    whole, two = synth.speech_wavs()
    return np.concatenate([two, synth.make_wav(2, 160000, seed=5, ragged=True)], 0)


@pytest.mark.parametrize("gemm", ["f32", "f16mx"])
def test_embeddings_postprocess_is_call(gemm):
    ext, w = extractor(gemm)
    x = torch.as_tensor(wavs(), device="cuda")
    raw = ext.embeddings(x)
    y = ext(x)
    assert raw.shape == (4, 512) and raw.dtype == torch.float32
    dev = (ext.postprocess(raw) - y).abs().max().item()
    assert dev <= 1e-5, dev
    # one utterance, and the three-launch tail
    assert ext.embeddings(x[:1]).shape == (1, 512)
    ext.fuse_tail = False
    try:
        raw3 = ext.embeddings(x)
        assert (ext.postprocess(raw3) - ext(x)).abs().max().item() <= 1e-5
    finally:
        ext.fuse_tail = True
    # against the fp64 oracle's tdnn6 output, relative to the embedding's scale (the x-vector bound is 1e-4 in every mode)
    _, inter = O.xvector_forward(wavs(), synth.extractor_cfg(), synth.oracle_layers(w), w["mean"], w["lda"], dtype=np.float64,
                                 return_intermediates=True)
    want = np.stack([it["tdnn6"] for it in inter])
    err = np.abs(host(raw) - want).max() / np.abs(want).max()
    assert err <= 1e-4, err


def test_verification_score_end_to_end():
    ext, _ = extractor("f32")
    mean, T, psi = model(128, seed=40)
    plda = Ls.PLDA(128, mean, T, psi)
    enroll = torch.as_tensor(wavs(), device="cuda")
    test = torch.as_tensor(synth.make_wav(3, 48000, seed=9), device="cuda")
    spk2utt = [[0, 1], [2], [3, 1, 0]]
    trials = (np.array([0, 1, 2, 0, 2]), np.array([0, 1, 2, 2, 0]))
    got = ver.score(ext, plda, enroll, spk2utt, test, trials)
    raw = ext.embeddings(enroll)
    means, nu = ver.speaker_means(raw, spk2utt)
    e_tr = plda.transform(ext.postprocess(means), num_examples=nu)
    y_tr = plda.transform(ext(test))
    want = plda.score_trials(y_tr, e_tr, trials[0], trials[1], enroll_num_examples=nu)
    assert got.shape == (5,) and torch.equal(got, want)
    ref = V.chain(host(raw), spk2utt, host(ext(test)), ext.xvecGlobalMean, np.c_[ext.ldaMat.T, ext.ldaOffset.T], mean, T, psi,
                  *trials)
    assert np.abs(host(got) - ref).max() <= 1e-4 * np.abs(ref).max()
