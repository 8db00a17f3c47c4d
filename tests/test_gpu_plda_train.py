"""PLDA back-end training on the MI355X (ktf.training, csrc/plda_train.hip) against the fp64 oracle tests/_plda_train_ref.py (Kaldi's
literal per-count EM): compute_plda, compute_lda and est_pca at D = 32, 128, 512 on ragged speakers (single-utterance ones
included), determinism, order invariance, Kaldi's preconditions, and the sitw chain x-vectors -> mean -> LDA -> PLDA -> Kaldi files
-> reload -> trial scores. The measured worst cases are printed (run with -s) and recorded in INTEGRATION.md §2g."""

import numpy as np
import pytest
import torch

import _plda_train_ref as R
import synth
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import io as kio
from kaldi_tflite_amd import training as tr
from kaldi_tflite_amd import verification as ver

pytestmark = pytest.mark.gpu

ROW_F64 = 1e-8            # fp64 transform rows, relative to the row norm, after sign alignment
ROW_F32 = 2.0 ** -23      # fp32 outputs (LDA, PCA): the rounding of the result, relative to the row norm
PSI = 1e-9
MEAN = 1e-12
SCORE = 1e-7


def spd(rng, spectrum):
    Q, _ = np.linalg.qr(rng.standard_normal((len(spectrum),) * 2))
    return (Q * spectrum) @ Q.T


def geom(top, D, ratio):
    return top * ratio ** np.arange(D)          # eigen-gaps of 1 / ratio - 1 >= 1 % relative


_DATA, _REF = {}, {}


def data(D, seed=1):
    """fp32 rows of a PLDA model with well separated spectra: S speakers with 1..8 rows each."""
    if (D, seed) not in _DATA:
        rng = np.random.default_rng(seed * 1000 + D)
        S = {32: 400, 128: 800, 512: 1500}[D]
        phi_b = spd(rng, geom(20.0, D, 0.985))
        phi_w = spd(rng, geom(2.0, D, 0.99))
        x, spk = R.sample_plda(rng, D, S, 1, 8, phi_w, phi_b, rng.standard_normal(D) * 3.0)
        _DATA[(D, seed)] = (x.astype(np.float32), spk, phi_w, phi_b)
    return _DATA[(D, seed)]


def ref_plda(D):
    if ("plda", D) not in _REF:
        x, spk, *_ = data(D)
        _REF[("plda", D)] = R.compute_plda(x.astype(np.float64), spk)
    return _REF[("plda", D)]


def dev(x):
    return torch.as_tensor(x, device="cuda")


def row_err(got, want):
    """max over rows of |got_i - s_i want_i| / |want_i|, s_i = the sign that aligns the rows."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    s = np.where(np.sum(got * want, axis=1) < 0, -1.0, 1.0)[:, None]
    return float((np.linalg.norm(got - s * want, axis=1) / np.linalg.norm(want, axis=1)).max())


def heldout_scores(models, D, seed=5, S=60, per=3):
    """Scores of a held-out trial set (every class against every test row) under each (mean, transform, psi)."""
    _, _, phi_w, phi_b = data(D)
    rng = np.random.default_rng(seed)
    x, spk = R.sample_plda(rng, D, S, per + 1, per + 1, phi_w, phi_b, np.zeros(D))
    enroll = [u[:per] for u in spk]
    test = np.array([u[per] for u in spk])
    ei, ti = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    out = []
    for mean, T, psi in models:
        p = ktf.layers.PLDA(D, mean, T, psi)
        e = p.transform(dev(np.stack([x[u].mean(0) for u in enroll])), num_examples=per)
        t = p.transform(dev(x[test]))
        out.append(p.score_trials(t, e, ei.reshape(-1), ti.reshape(-1), enroll_num_examples=per).cpu().numpy())
    return out


def plda_arrays(p):
    return p.mean, p.transformMat, p.psi


# ----------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("D", [32, 128, 512])
def test_compute_plda_matches_the_oracle(D):
    x, spk, *_ = data(D)
    got = tr.compute_plda(dev(x), spk)
    mean, T, psi = ref_plda(D)
    assert got.transformMat.dtype == np.float64 and got.transformMat.shape == (D, D)
    e_mean = np.abs(got.mean - mean).max() / np.abs(mean).max()
    e_psi = float((np.abs(got.psi - psi) / psi).max())
    e_row = row_err(got.transformMat, T)
    s_got, s_ref = heldout_scores([plda_arrays(got), (mean, T, psi)], D)
    e_score = np.abs(s_got - s_ref).max() / np.abs(s_ref).max()
    print(f"\nplda D={D}: mean {e_mean:.2e} psi {e_psi:.2e} rows {e_row:.2e} scores {e_score:.2e} "
          f"(psi {psi[0]:.3g} .. {psi[-1]:.3g})")
    assert e_mean <= MEAN and e_psi <= PSI and e_row <= ROW_F64 and e_score <= SCORE, (e_mean, e_psi, e_row, e_score)
    assert np.all(np.diff(got.psi) <= 0) and np.all(got.psi >= 0)


@pytest.mark.parametrize("D", [32, 128, 512])
@pytest.mark.parametrize("f", [0.0, 0.1])
def test_compute_lda_matches_the_oracle(D, f):
    x, spk, *_ = data(D)
    for dim in (D // 4, D):
        got = tr.compute_lda(dev(x), spk, dim, total_covariance_factor=f)
        want = R.compute_lda(x.astype(np.float64), spk, dim, total_covariance_factor=f)
        assert got.dtype == np.float32 and got.shape == (dim, D + 1)
        e = row_err(got, want)
        print(f"\nlda D={D} f={f} dim={dim}: rows {e:.2e}")
        assert e <= ROW_F32, e


@pytest.mark.parametrize("D", [32, 128, 512])
@pytest.mark.parametrize("normalize_mean", [False, True])
@pytest.mark.parametrize("normalize_variance", [False, True])
def test_est_pca_matches_the_oracle(D, normalize_mean, normalize_variance):
    x, *_ = data(D)
    for dim in (-1, D // 2):
        got = tr.est_pca(dev(x), dim, normalize_mean=normalize_mean, normalize_variance=normalize_variance)
        want = R.est_pca(x.astype(np.float64), dim, normalize_mean, normalize_variance)
        assert got.dtype == np.float32 and got.shape == want.shape
        e = row_err(got, want)
        print(f"\npca D={D} mean={normalize_mean} var={normalize_variance} dim={dim}: rows {e:.2e}")
        assert e <= ROW_F32, e


# ----------------------------------------------------------------------------- determinism, order, map forms
def test_outputs_are_bit_identical_run_to_run_and_for_a_device_map():
    x, spk, *_ = data(128)
    xd = dev(x)
    a, b = tr.compute_plda(xd, spk), tr.compute_plda(xd, spk)
    for u, v in zip(plda_arrays(a), plda_arrays(b)):
        assert np.array_equal(u, v)
    off = np.cumsum([0] + [len(u) for u in spk])
    csr = (dev(off), dev(np.concatenate(spk)))
    c = tr.compute_plda(xd, csr)
    for u, v in zip(plda_arrays(a), plda_arrays(c)):
        assert np.array_equal(u, v)
    assert np.array_equal(tr.compute_lda(xd, spk, 64), tr.compute_lda(xd, spk, 64))
    assert np.array_equal(tr.compute_lda(xd, spk, 64), tr.compute_lda(xd, csr, 64))
    assert np.array_equal(tr.est_pca(xd, 32, True, True), tr.est_pca(xd, 32, True, True))


def test_permuting_speakers_or_rows_changes_only_rounding():
    x, spk, *_ = data(128)
    xd = dev(x)
    rng = np.random.default_rng(3)
    perm = [list(rng.permutation(spk[s])) for s in rng.permutation(len(spk))]
    a, b = tr.compute_plda(xd, spk), tr.compute_plda(xd, perm)
    assert np.abs(a.mean - b.mean).max() <= MEAN * np.abs(a.mean).max()
    assert (np.abs(a.psi - b.psi) / a.psi).max() <= PSI
    assert row_err(a.transformMat, b.transformMat) <= ROW_F64
    assert row_err(tr.compute_lda(xd, spk, 64), tr.compute_lda(xd, perm, 64)) <= 2 * ROW_F32


def test_kaldis_preconditions_raise_before_launching():
    x, spk, *_ = data(32)
    xd = dev(x)
    with pytest.raises(ValueError, match="no within-class data"):
        tr.compute_plda(xd, [[i] for i in range(10)])
    with pytest.raises(ValueError, match="no within-class data"):
        tr.compute_lda(xd, [[i] for i in range(10)], 4)
    with pytest.raises(ValueError, match="dim"):
        tr.compute_lda(xd, spk, 33)
    with pytest.raises(ValueError, match="dim"):
        tr.est_pca(xd, 33)
    with pytest.raises(ValueError, match="at least one utterance"):
        tr.compute_plda(xd, (np.array([0, 2, 2, 4]), np.array([0, 1, 2, 3])))
    with pytest.raises(ValueError, match="without utterances"):
        tr.compute_plda(xd, (dev(np.array([0, 2, 2, 4])), dev(np.array([0, 1, 2, 3]))))
    with pytest.raises(ValueError, match="outside"):
        tr.compute_plda(xd, [[0, 1], [2, x.shape[0]]])
    with pytest.raises(ValueError, match="outside"):
        tr.compute_lda(xd, (dev(np.array([0, 2, 4])), dev(np.array([0, 1, 2, -1]))), 4)
    with pytest.raises(ValueError, match="two speakers"):
        tr.compute_plda(xd, [[0, 1, 2]])
    with pytest.raises(ValueError, match="1 <= D <= 1024"):
        tr.compute_plda(torch.zeros((8, 1025), device="cuda"), [[0, 1], [2, 3]])
    with pytest.raises(ValueError, match="fp32"):
        tr.compute_lda(xd.double(), spk, 4)
    with pytest.raises(ValueError, match="fp32"):
        tr.est_pca(xd[0])


# ----------------------------------------------------------------------------- the sitw chain
def test_sitw_chain_without_kaldi(tmp_path):
    D = 512
    x0, _, phi_w, phi_b = data(D)
    mean0 = x0.astype(np.float64).mean(0)
    phi_b = phi_b * 0.002                       # speakers this close give an EER of a few percent on the held-out trials
    x, spk = R.sample_plda(np.random.default_rng(11), D, 1500, 2, 8, phi_w, phi_b, mean0)
    x = x.astype(np.float32)
    xd = dev(x)
    seq = synth.build_sequential(ktf, synth.make_weights(seed=4321, narrow=True), "f32")
    cfg = synth.extractor_cfg()
    # 1. global mean (ivector-mean without spk2utt), 2. LDA on the mean-subtracted rows, 3. postprocess, 4. PLDA
    mean = ver.speaker_means(xd, [np.arange(x.shape[0])])[0][0]
    mean_h = mean.cpu().numpy()
    lda = tr.compute_lda(xd - mean, spk, 128)
    ext = ktf.models.XvectorExtractor.from_parts(cfg, seq, mean_h, lda)
    plda = tr.compute_plda(ext.postprocess(xd), spk)
    # the same chain with the oracle's estimators
    lda_ref = R.compute_lda((x - mean_h).astype(np.float64), spk, 128).astype(np.float32)
    ext_ref = ktf.models.XvectorExtractor.from_parts(cfg, seq, mean_h, lda_ref)
    plda_ref = ktf.layers.PLDA(128, *R.compute_plda(ext_ref.postprocess(xd).cpu().numpy().astype(np.float64), spk))

    # held-out speakers: 3 enrollment rows and 2 test rows each; every class against every test row
    rng = np.random.default_rng(77)
    H, per = 200, 5
    xh, hspk = R.sample_plda(rng, D, H, per, per, phi_w, phi_b, mean0)
    xh = dev(xh.astype(np.float32))
    enroll = [u[:3] for u in hspk]
    test = torch.as_tensor(np.concatenate([u[3:] for u in hspk]), device="cuda")
    tspk = np.repeat(np.arange(H), per - 3)
    ei, ti = np.meshgrid(np.arange(H), np.arange(len(tspk)), indexing="ij")
    ei, ti = ei.reshape(-1), ti.reshape(-1)
    labels = tspk[ti] == ei

    def scores(e, p):
        means, nu = ver.speaker_means(xh, enroll)
        et = p.transform(e.postprocess(means), num_examples=nu)
        tt = p.transform(e.postprocess(xh[test]))
        return p.score_trials(tt, et, ei, ti, enroll_num_examples=nu)

    want = scores(ext, plda)
    # 5. Kaldi files, read back with the existing readers; 6. the same trial scores
    kio.WriteKaldiPlda(tmp_path / "plda", plda.mean, plda.transformMat, plda.psi)
    p2 = kio.KaldiPldaReader(str(tmp_path / "plda"), True)
    plda2 = ktf.layers.PLDA(128, p2.mean, p2.transformMat, p2.psi)
    for binary in (True, False):
        sfx = "" if binary else ".txt"
        kio.WriteKaldiArray(tmp_path / f"mean.vec{sfx}", mean_h, binary=binary)
        kio.WriteKaldiArray(tmp_path / f"transform.mat{sfx}", lda, binary=binary)
        m2 = kio.ReadKaldiArray(str(tmp_path / f"mean.vec{sfx}"), binary)
        l2 = kio.ReadKaldiArray(str(tmp_path / f"transform.mat{sfx}"), binary)
        got = scores(ktf.models.XvectorExtractor.from_parts(cfg, seq, m2, l2), plda2)
        if binary:
            assert torch.equal(got, want)
        else:
            e = ((got - want).abs().max() / want.abs().max()).item()
            print(f"\nchain: text mean / LDA, scores {e:.2e} of max |score|")
            assert e <= 1e-5, e
    eer = ver.eer(want, labels)
    eer_ref = ver.eer(scores(ext_ref, plda_ref), labels)
    print(f"\nchain: EER {eer:.4f}, oracle-trained {eer_ref:.4f}")
    assert eer_ref > 0.01 and abs(eer - eer_ref) <= 0.005, (eer, eer_ref)
