"""GPU half of VBx: every stage of ktf_vbx_* against the fp64 oracle (_vbx_ref), then the loop, the padded
speakers, the bits and the PLDA / diarize plumbing. Bounds as in test_gpu_vb: every fp64 stage output within 1e-8 of its array's
largest magnitude, the multi-iteration loop within 1e-6 on gamma and 1e-6 relative on the ELBO. Every test prints its measured
deviations before it asserts (pytest -s)."""

import functools

import numpy as np
import pytest
import torch

import _golden as G
import _vbx_ref as X
import synth
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L
from kaldi_tflite_amd import ops
from kaldi_tflite_amd.diarization import VBx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# an empty recording in the middle, lengths on both sides of the 16-row tile and of the forward-backward's 128-block chunk, and one
# recording of more than two workgroups of the speaker update
STAGE_T = (15, 1, 0, 17, 129, 2 * L.VBX_UPDATE_ROWS + 88)


def d(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-300)) if want.size else 0.0


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ stages
@functools.lru_cache(maxsize=None)
def stage_inputs(D, K):
    rng = np.random.default_rng(100 * D + K)
    phi = rng.uniform(0.05, 8.0, D)
    xs = [rng.standard_normal((T, D)) * 1.5 for T in STAGE_T]
    gs = [rng.dirichlet(np.full(K, 1.0), T).reshape(T, K) for T in STAGE_T]
    return phi, xs, gs


@pytest.mark.parametrize("Fa,Fb", [(0.3, 17.0), (1.0, 1.0)])
@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("D", [5, 30, 128])
def test_stages_against_the_oracle(D, K, Fa, Fb):
    phi, xs, gs = stage_inputs(D, K)
    off = d(offsets(STAGE_T))
    want = {k: [] for k in ("rho", "G", "alpha", "invL", "c", "kl", "lls")}
    for x, g in zip(xs, gs):
        rho, Gt = X.prepare(x, phi)
        if len(x):
            alpha, invL, c, kl = X.speaker_update(g, rho, phi, Fa / Fb)
        else:                                                       # a recording without windows: nothing written, c = kl = 0
            alpha, invL, c, kl = np.zeros((K, D)), np.zeros((K, D)), np.zeros(K), np.zeros(K)
        for k, v in zip(want, (rho, Gt, alpha[None], invL[None], c[None], kl[None], X.loglike(rho, Gt, alpha, c, Fa))):
            want[k].append(v)
    want = {k: np.concatenate(v) for k, v in want.items()}

    def run():
        rho, Gt = ops.vbx_prepare(d(np.concatenate(xs)), d(phi))
        alpha, invL, c, kl = ops.vbx_speaker_update(d(np.concatenate(gs)), rho, d(phi), Fa / Fb, off)
        lls = ops.vbx_loglike(rho, Gt, alpha, c, Fa, off)
        return {k: v.cpu().numpy() for k, v in zip(want, (rho, Gt, alpha, invL, c, kl, lls))}
    got, again = run(), run()
    errs = {k: rel(got[k], want[k]) for k in want}
    print(f"vbx stages D={D} K={K} Fa={Fa} Fb={Fb}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()) + " (bound 1e-8)")
    for k in want:
        assert got[k].shape == want[k].shape, k
        assert np.isfinite(got[k]).all() and errs[k] <= 1e-8, (k, errs[k])
        assert np.array_equal(got[k], again[k]), k
    assert not got["c"][2].any() and not got["kl"][2].any() and not got["alpha"][2].any()


def test_entry_points_refuse_shapes_outside_the_limits():
    z = torch.zeros((4, 17), dtype=torch.float64, device=DEV)
    off = d(offsets([4]))
    with pytest.raises(ValueError, match="speakers"):
        ops.vbx_speaker_update(z, z, d(np.ones(17)), 1.0, off)
    wide = torch.zeros((1, L.VBX_MAX_DIM + 1), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="dim"):
        ops.vbx_prepare(wide, d(np.ones(L.VBX_MAX_DIM + 1)))
    with pytest.raises(ValueError, match="dim"):
        ops.vbx_loglike(wide, z[:1, 0], wide[None], z[:1, :1], 1.0, d(offsets([1])))


# ------------------------------------------------------------------------------------------------ the loop
@functools.lru_cache(maxsize=None)
def planted_case():
    """test_vbx_cpu's recording and start, a second recording of another length (its first 170 windows backwards), their oracle runs
    at the default K = 10."""
    phi, x, truth = X.planted(1, 30, 4, 300, 12)
    lab = X.noisy_start(truth, 6, 0.25, 4)
    recs = [(x, lab), (x[:170][::-1].copy(), lab[:170][::-1].copy())]
    return phi, recs, [X.run(xx, phi, *X.init(ll, 10)) for xx, ll in recs]


def test_loop_follows_the_oracle():
    phi, recs, refs = planted_case()
    v = VBx(phi)
    x = d(np.concatenate([recs[0][0], recs[1][0]]))
    res = v(x, [300, 0, 170], init_labels=np.concatenate([recs[0][1], recs[1][1]]))
    assert res.offsets.tolist() == [0, 300, 300, 470] and res.gamma.shape == (470, 10) and res.elbo.shape == (3, 40)
    gamma, pi, elbo, labels = (t.cpu().numpy() for t in (res.gamma, res.pi, res.elbo, res.labels))
    for r, lo, hi, (gw, pw, ew) in ((0, 0, 300, refs[0]), (2, 300, 470, refs[1])):
        eg, ee = float(np.abs(gamma[lo:hi] - gw).max()), rel(elbo[r, :len(ew)], ew)
        top = np.sort(gw, 1)
        clear = top[:, -1] - top[:, -2] > 1e-5
        lw, kw = X.labels_of(gw)
        print(f"vbx loop recording {r}: gamma {eg:.2e} (bound 1e-6), elbo {ee:.2e} (1e-6 relative), pi {np.abs(pi[r] - pw).max():.2e}, "
              f"{len(ew)} iterations, excused {(~clear).mean():.4f}")
        assert eg <= 1e-6 and ee <= 1e-6 and np.abs(pi[r] - pw).max() <= 1e-6
        assert int(res.iters[r]) == len(ew) and np.isnan(elbo[r, len(ew):]).all()
        assert (~clear).mean() <= 0.01 and np.array_equal(labels[lo:hi][clear], lw[clear]) and int(res.counts[r]) == kw
    assert res.iters[1] == 0 and int(res.counts[1]) == 0 and np.isnan(elbo[1]).all() and res.labels.dtype == torch.int32
    with pytest.raises(ValueError):
        v(x, [300, 170], init_labels=np.zeros(10, np.int64))
    with pytest.raises(ValueError):
        v(x, [300, 171])
    with pytest.raises(ValueError):
        v(x[:, :7], [300, 170])


def test_padded_speakers_stay_at_zero():
    """Recordings that use 2, 5 and 16 of K = 16 columns: gamma0 and pi0 are zero on the rest."""
    used, lens = (2, 5, 16), (90, 141, 200)
    rng = np.random.default_rng(11)
    phi = np.sort(rng.uniform(0.05, 8.0, 30))[::-1].copy()
    xs, g0, p0, refs = [], [], [], []
    for Kr, T in zip(used, lens):
        means = rng.standard_normal((Kr, 30)) * np.sqrt(phi)
        truth = np.repeat(np.arange(T // 5 + 1) % Kr, 5)[:T]
        xs.append(means[truth] + rng.standard_normal((T, 30)))
        lab = X.noisy_start(truth, Kr, 0.2, Kr)
        assert np.unique(lab).size == Kr
        refs.append(X.run(xs[-1], phi, *X.init(lab, Kr), max_iters=4))
        g, p = X.init(lab, 16)
        g0.append(g)
        p0.append(p)
    res = VBx(phi, max_speakers=16, max_iters=4)(d(np.concatenate(xs)), lens, gamma0=np.concatenate(g0), pi0=np.stack(p0))
    gamma, pi, elbo = (t.cpu().numpy() for t in (res.gamma, res.pi, res.elbo))
    assert np.isfinite(gamma).all() and np.isfinite(pi).all()
    off = offsets(lens)
    for r, (Kr, (gw, pw, ew)) in enumerate(zip(used, refs)):
        g = gamma[off[r]:off[r + 1]]
        eg, ee = float(np.abs(g[:, :Kr] - gw).max()), rel(elbo[r, :len(ew)], ew)
        print(f"vbx padded: {Kr} of 16 columns: gamma {eg:.2e} (bound 1e-6), elbo {ee:.2e} (1e-6 relative)")
        assert not g[:, Kr:].any() and not pi[r, Kr:].any()
        assert eg <= 1e-6 and ee <= 1e-6 and np.abs(pi[r, :Kr] - pw).max() <= 1e-6
        assert int(res.iters[r]) == len(ew) and np.isfinite(elbo[r, :len(ew)]).all()


def test_bits_do_not_depend_on_the_offset():
    phi, recs, _ = planted_case()
    x, lab = recs[0]
    v = VBx(phi, max_iters=3)
    alone = v(d(x), [300], init_labels=lab)
    for lead in (1, 37):
        res = v(d(np.concatenate([recs[1][0][:lead], x])), [lead, 300], init_labels=np.concatenate([recs[1][1][:lead], lab]))
        assert torch.equal(res.gamma[lead:], alone.gamma) and torch.equal(res.pi[1], alone.pi[0]), lead
        assert np.array_equal(res.elbo.cpu().numpy()[1], alone.elbo.cpu().numpy()[0], equal_nan=True), lead
        assert torch.equal(res.labels[lead:], alone.labels)


# ------------------------------------------------------------------------------------------------ PLDA and diarize
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_from_plda_agrees_with_the_oracle(dtype):
    p = ktf.io.KaldiPldaReader(G.GOLDEN + "/plda.bin", True)       # the model of tests/golden/plda.npz
    plda = ktf.layers.PLDA(len(p.psi), p.mean, p.transformMat, p.psi)
    x = G.load("plda.npz")["plda_input"][:, 0, :].astype(dtype)
    lab = np.arange(len(x)) // 5 % 3
    A, b, psi = (np.asarray(a, np.float64) for a in (plda.transformMat, plda.offset, plda.psi))
    for lda_dim in (None, 10):
        n = len(psi) if lda_dim is None else lda_dim
        res = VBx.from_plda(plda, lda_dim=lda_dim, max_speakers=4, max_iters=5)(d(x), [len(x)], init_labels=lab)
        gw, pw, ew = X.run((x.astype(np.float64) @ A.T + b)[:, :n], psi[:n], *X.init(lab, 4), max_iters=5)
        eg, ee = float(np.abs(res.gamma.cpu().numpy() - gw).max()), rel(res.elbo.cpu().numpy()[0, :len(ew)], ew)
        print(f"vbx from_plda {np.dtype(dtype).name} lda_dim={lda_dim}: gamma {eg:.2e} (bound 1e-6), elbo {ee:.2e} (1e-6 relative)")
        assert eg <= 1e-6 and ee <= 1e-6 and int(res.iters[0]) == len(ew)


def test_diarize_with_vbx():
    w = synth.make_weights(seed=4321, feat_dim=30)
    ext = synth.build_extractor(ktf, synth.extractor_cfg(), w, gemm="f32")
    odim = ext.ldaMat.shape[1]
    rng = np.random.default_rng(5)
    T = rng.standard_normal((odim, odim)) / np.sqrt(odim) + np.eye(odim)
    plda = ktf.layers.PLDA(odim, rng.standard_normal(odim) * 0.1, T, np.sort(rng.uniform(0.05, 30.0, odim))[::-1].copy(), dtype="float32")
    whole, _ = synth.speech_wavs()
    wavs = [whole[0], np.zeros(20000, np.float32), synth.coloured_am_noise(1, 160000)[0]]
    before = ktf.diarization.diarize(ext, plda, wavs, threshold=0.0)               # before any VBx exists
    assert before.ahc_labels is None and before.vbx is None
    v = VBx.from_plda(plda, lda_dim=odim // 2)
    out = ktf.diarization.diarize(ext, plda, wavs, threshold=0.0, vbx=v)
    after = ktf.diarization.diarize(ext, plda, wavs, threshold=0.0)
    assert torch.equal(after.labels, before.labels) and torch.equal(after.counts, before.counts) and after.rttm == before.rttm
    assert torch.equal(out.ahc_labels, before.labels) and out.labels.shape == before.labels.shape and out.labels.dtype == torch.int32
    lengths, counts, labels = out.windows.lengths, out.counts.cpu().tolist(), out.labels.cpu().numpy()
    assert lengths[1] == 0 and counts[1] == 0 and out.vbx.iters[1] == 0
    o = 0
    for r, n in enumerate(lengths):
        if n:
            assert sorted(set(labels[o:o + n].tolist())) == list(range(1, counts[r] + 1)), r
        o += n
    same = v(out.windows.xvectors, lengths, init_labels=before.labels)
    assert torch.equal(same.labels, out.labels) and torch.equal(same.gamma, out.vbx.gamma)
    assert out.rttm == ktf.diarization.rttm(out.windows, out.labels)
