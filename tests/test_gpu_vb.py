"""GPU half of the VB-HMM resegmentation: every stage of ktf_vb_* against the fp64 oracle (_vb_ref) on supplied inputs, so that no
threshold decision can flip, then the loop and the model round trip. Bounds: post 1e-5 absolute (test_gpu_fgmm's), loglike 8 x the
gap between the oracle in fp64 and in float32 measured here (test_gpu_ubm_train's rule), every fp64 output 1e-8 of its array's
largest magnitude, the forward-backward 1e-8 absolute (tll relative), the three-iteration loop 1e-6 (test_gpu_ivector_train's).
Every test prints its measured deviations before it asserts (pytest -s); INTEGRATION.md §2j is where they are recorded."""

import functools

import numpy as np
import pytest
import torch

import _vb_ref as V
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L
from kaldi_tflite_amd import ops, training
from kaldi_tflite_amd.io import (DiagGmmModel, IvecExtractorModel, KaldiDiagGmmReader, KaldiIvecExtractorReader, WriteKaldiDiagGmm,
                                 WriteKaldiIvecExtractor)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C_ = L.VB_FB_CHUNK


def d(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-300)) if want.size else 0.0


# ------------------------------------------------------------------------------------------------ posteriors
@functools.lru_cache(maxsize=None)
def post_case(D, I, n, F, thr=1e-3, flat=False):
    rng = np.random.default_rng(D * 1000 + I)
    (w, mi, iv), _ = V.random_model(rng, I, D, 2, spread=0.05 if flat else 1.0)
    ubm = DiagGmmModel(w, mi, iv)
    x = (rng.standard_normal((F, D)) * (0.1 if flat else 1.5)).astype(np.float32)
    W = np.concatenate([ubm.means_invvars.T, (np.float32(-0.5) * ubm.inv_vars).T]).astype(np.float32)
    ref64 = V.posteriors(x, ubm.gconsts, ubm.means_invvars, ubm.inv_vars, n, 0.9, 0.2, thr)
    ref32 = V.posteriors(x, ubm.gconsts, ubm.means_invvars, ubm.inv_vars, n, 0.9, 0.2, thr, dtype=np.float32)
    return ubm, x, W, ref64, ref32


@pytest.mark.parametrize("D,I,n,F", [(5, 8, 3, 203), (16, 33, 4, 1001), (40, 70, 8, 517)])
def test_posteriors(D, I, n, F):
    ubm, x, W, (g64, p64, G64, dense, over), ref32 = post_case(D, I, n, F)
    trunc = torch.zeros(1, dtype=torch.int32, device=DEV)
    g, p, ll = ops.vb_post(d(x), d(W), d(ubm.gconsts), n, 0.9, 0.2, 1e-3, trunc)
    g, p, ll = g.cpu().numpy(), p.cpu().numpy(), ll.cpu().numpy()
    gap = float(np.abs(ref32[2].astype(np.float64) - G64).max())
    err_ll = float(np.abs(ll - G64).max())
    # per frame: the dense posterior of every kept Gaussian, and the kept set wherever the oracle is clear of the threshold
    err_p, checked = 0.0, 0
    for t in range(F):
        kept = g[t][g[t] >= 0]
        assert len(set(kept.tolist())) == len(kept) and (np.diff(p[t][:len(kept)]) <= 0).all() and (p[t][len(kept):] == 0).all()
        err_p = max(err_p, float(np.abs(p[t][:len(kept)] - dense[t, kept]).max()) if len(kept) else 0.0)
        clear = np.abs(dense[t] - 1e-3) > 1e-5
        srt = np.sort(dense[t])[::-1]
        if clear.all() and (len(srt) <= n or srt[n - 1] - srt[n] > 1e-5 or srt[n] < 1e-3 - 1e-5):
            assert set(kept.tolist()) == set(g64[t][g64[t] >= 0].tolist()), t
            checked += 1
    print(f"vb_post D={D} I={I} n={n}: post {err_p:.3e} (bound 1e-5), loglike {err_ll:.3e} (fp32 oracle gap {gap:.3e}), sets checked "
          f"{checked}/{F}, truncated {int(trunc.item())} (oracle {over})")
    assert err_p <= 1e-5 and err_ll <= 8 * gap and checked > F // 2
    # a frame's bits depend on its own row alone
    g2, p2, ll2 = ops.vb_post(d(x[7:60]), d(W), d(ubm.gconsts), n, 0.9, 0.2, 1e-3, trunc)
    assert np.array_equal(g2.cpu().numpy(), g[7:60]) and np.array_equal(p2.cpu().numpy(), p[7:60]) and np.array_equal(ll2.cpu().numpy(), ll[7:60])


def test_posteriors_overflow_counter():
    ubm, x, W, (g64, p64, G64, dense, over), _ = post_case(40, 70, 8, 517, thr=1e-4, flat=True)
    cand = (dense >= 1e-4).sum(1)
    clear = (np.abs(dense - 1e-4) > 1e-5).all(1)
    assert over > 400 and clear.all()                               # built to overflow, and no candidate near the threshold
    trunc = torch.zeros(1, dtype=torch.int32, device=DEV)
    g, p, _ = ops.vb_post(d(x), d(W), d(ubm.gconsts), 8, 0.9, 0.2, 1e-4, trunc)
    assert int(trunc.item()) == int((cand > 8).sum()) == over
    assert (g.cpu().numpy() >= 0).sum(1).min() == min(8, cand.min())
    ops.vb_post(d(x), d(W), d(ubm.gconsts), 8, 0.9, 0.2, 1e-4, trunc)
    assert int(trunc.item()) == 2 * over                            # the counter is increased, not set


# ------------------------------------------------------------------------------------------------ statistics, update, lls
@functools.lru_cache(maxsize=None)
def stage_case(R, K, ds, I=6, D=5):
    n, lens = 3, [37, 0, 58]
    rng = np.random.default_rng(R * 100 + K * 10 + ds)
    (w, mi, iv), M = V.random_model(rng, I, D, R)
    m, iE, B, UU = V.consts(mi, iv, M)
    recs = []
    for T in lens:
        x = (rng.standard_normal((T, D)) * 1.5).astype(np.float32)
        g = np.array([rng.permutation(I)[:n] for _ in range(T)], dtype=np.int32).reshape(T, n)
        p = rng.uniform(0.0, 0.2, (T, n)).astype(np.float32)
        drop = rng.random((T, n)) < 0.2
        g[drop], p[drop] = -1, 0.0
        q = rng.dirichlet(np.full(K, 1.0), V.blocks(T, ds)).reshape(V.blocks(T, ds), K)
        st = V.speaker_stats(x, g, p, q, ds, m)
        up = V.speaker_update(*st, B, UU)
        recs.append(dict(x=x, g=g, p=p, q=q, st=st, up=up, lls=V.block_loglike(x, g, p, ds, m, up[3], up[4])))
    return dict(I=I, D=D, n=n, lens=lens, m=m, B=B, UU=UU, recs=recs)


def run_stages(c, K, ds):
    recs, I, D = c["recs"], c["I"], c["D"]
    off = np.concatenate([[0], np.cumsum(c["lens"])]).astype(np.int32)
    boff = np.concatenate([[0], np.cumsum([V.blocks(T, ds) for T in c["lens"]])]).astype(np.int32)
    x, g, p = (d(np.concatenate([r[k] for r in recs])) for k in ("x", "g", "p"))
    q = d(np.concatenate([r["q"] for r in recs]))
    R = c["B"].shape[1]
    U = np.stack([V.tril_pack(u) for u in c["UU"]])
    start, pairs = ops.vb_bucket(g, I)
    Nst, Fst = ops.vb_speaker_stats(x, d(off), d(boff), ds, p, start, pairs, d(c["m"]), q)
    a, Wp, kl, h, gg = ops.vb_speaker_update(Nst, Fst, d(c["B"]), d(U))
    lls = ops.vb_block_loglike(x, d(off), d(boff), ds, int(boff[-1]), g, p, d(c["m"]), h, gg, K)
    return dict(N=Nst, F=Fst, a=a, W=Wp, kl=kl, h=h, g=gg, lls=lls)


def check_stages(R, K, ds, **shape):
    c = stage_case(R, K, ds, **shape)
    got = {k: v.cpu().numpy() for k, v in run_stages(c, K, ds).items()}
    again = {k: v.cpu().numpy() for k, v in run_stages(c, K, ds).items()}
    recs, I, D = c["recs"], c["I"], c["D"]
    want = dict(N=np.concatenate([r["st"][0] for r in recs]), F=np.concatenate([r["st"][1].reshape(K, I * D) for r in recs]),
                a=np.concatenate([r["up"][0] for r in recs]),
                W=np.concatenate([np.stack([V.tril_pack(w) for w in r["up"][1]]) for r in recs]),
                kl=np.concatenate([r["up"][2] for r in recs]), h=np.concatenate([r["up"][3].reshape(K, I * D) for r in recs]),
                g=np.concatenate([r["up"][4] for r in recs]), lls=np.concatenate([r["lls"] for r in recs]))
    errs = {k: rel(got[k], want[k]) for k in want}
    print(f"vb stages I={I} D={D} R={R} K={K} downsample={ds}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()) + " (bound 1e-8)")
    for k in want:
        assert got[k].shape == want[k].shape, k
        assert errs[k] <= 1e-8, (k, errs[k])
        assert np.array_equal(got[k], again[k]), k
    # the recording without frames: zero statistics, the prior's update
    assert not got["N"][K:2 * K].any() and not got["F"][K:2 * K].any() and not got["a"][K:2 * K].any() and not got["kl"][K:2 * K].any()


@pytest.mark.parametrize("ds", [1, 7])
@pytest.mark.parametrize("K", [1, 3, 10])
@pytest.mark.parametrize("R", [4, 33, 100])
def test_stats_update_loglike(R, K, ds):
    check_stages(R, K, ds)


def test_stats_update_loglike_two_workgroups_along_n():
    # h = a B^T has N = I D = 275 columns: two workgroups of the A B^T product along N, the second with one ragged wave and three
    # that exit (the shapes above have N = 30: one workgroup, one wave); M = 9 speaker rows
    check_stages(5, 3, 1, I=11, D=25)


# ------------------------------------------------------------------------------------------------ forward-backward
FB_T = (1, 2, C_ - 1, C_, C_ + 1, 3 * C_ + 7)


@functools.lru_cache(maxsize=None)
def fb_case(K, lp, spread):
    rng = np.random.default_rng(K * 1000 + int(lp * 100) + spread)
    recs = []
    for T in FB_T:
        lls = rng.uniform(0.0, float(spread), (T, K)) - 40.0
        sp = rng.dirichlet(np.full(K, 2.0))
        recs.append((lls, sp) + V.forward_backward(lls, sp, lp))
    return recs


def fb_run(recs, lp):
    boff = np.concatenate([[0], np.cumsum([r[0].shape[0] for r in recs])]).astype(np.int32)
    q, sp, tll = ops.vb_forward_backward(d(np.concatenate([r[0] for r in recs])), d(boff), d(np.stack([r[1] for r in recs])), lp)
    return q.cpu().numpy(), sp.cpu().numpy(), tll.cpu().numpy(), boff


@pytest.mark.parametrize("spread", [1, 200])
@pytest.mark.parametrize("lp", [0.5, 0.99])
@pytest.mark.parametrize("K", [1, 2, 10, 16])
def test_forward_backward(K, lp, spread):
    recs = fb_case(K, lp, spread)
    q, sp, tll, boff = fb_run(recs, lp)
    eq, es, et = 0.0, 0.0, 0.0
    for r, (lls, sp0, qw, tw, sw) in enumerate(recs):
        eq = max(eq, float(np.abs(q[boff[r]:boff[r + 1]] - qw).max()))
        es = max(es, float(np.abs(sp[r] - sw).max()))
        et = max(et, abs(tll[r] - tw) / abs(tw))
    print(f"vb fb K={K} loop_prob={lp} spread={spread}: q {eq:.2e}, sp {es:.2e} (bound 1e-8 absolute), tll {et:.2e} (1e-8 relative)")
    assert np.isfinite(q).all() and eq <= 1e-8 and es <= 1e-8 and et <= 1e-8
    # a recording's outputs have the same bits alone and inside a batch of 5
    five = [recs[4], recs[0], recs[1], recs[5], recs[3]]
    qb, sb, tb, bo = fb_run(five, lp)
    qa, sa, ta, _ = fb_run([recs[5]], lp)
    assert np.array_equal(qb[bo[3]:bo[4]], qa) and np.array_equal(sb[3], sa[0]) and tb[3] == ta[0]
    assert np.array_equal(qb[bo[3]:bo[4]], q[boff[5]:boff[6]])


def test_forward_backward_empty_recording_keeps_sp():
    recs = fb_case(2, 0.5, 1)
    boff = np.array([0, 0, 2], np.int32)
    sp0 = np.array([[0.3, 0.7], recs[1][1]])
    q, sp, tll = ops.vb_forward_backward(d(recs[1][0]), d(boff), d(sp0), 0.5)
    assert np.array_equal(sp.cpu().numpy()[0], sp0[0]) and float(tll[0]) == 0.0
    assert np.abs(q.cpu().numpy() - recs[1][2]).max() <= 1e-8


@pytest.mark.parametrize("K,lp,spread", [(1, 0.5, 1), (2, 0.99, 1), (10, 0.99, 200), (16, 0.5, 200)])
def test_serial_form_matches_oracle(K, lp, spread):
    """The serial form that tools/bench_vb.py times the chunked scan against computes the same thing, to the same bounds."""
    recs = fb_case(K, lp, spread)
    boff = np.concatenate([[0], np.cumsum([r[0].shape[0] for r in recs])]).astype(np.int32)
    q, sp, tll = (t.cpu().numpy() for t in ops.vb_forward_backward_serial(d(np.concatenate([r[0] for r in recs])), d(boff),
                                                                          d(np.stack([r[1] for r in recs])), lp))
    eq, es, et = 0.0, 0.0, 0.0
    for r, (lls, sp0, qw, tw, sw) in enumerate(recs):
        eq = max(eq, float(np.abs(q[boff[r]:boff[r + 1]] - qw).max()))
        es = max(es, float(np.abs(sp[r] - sw).max()))
        et = max(et, abs(tll[r] - tw) / abs(tw))
    print(f"vb fb serial K={K} loop_prob={lp} spread={spread}: q {eq:.2e}, sp {es:.2e} (bound 1e-8 absolute), tll {et:.2e} (1e-8 relative)")
    assert np.isfinite(q).all() and eq <= 1e-8 and es <= 1e-8 and et <= 1e-8
    if K == 2:                                                      # a recording without blocks keeps its sp
        empty = ops.vb_forward_backward_serial(d(recs[1][0]), d(np.array([0, 0, 2], np.int32)), d(np.array([[0.3, 0.7], recs[1][1]])), lp)
        assert np.array_equal(empty[1].cpu().numpy()[0], [0.3, 0.7]) and float(empty[2][0]) == 0.0


# ------------------------------------------------------------------------------------------------ the loop
@functools.lru_cache(maxsize=None)
def planted():
    (w, mi, iv), M, x, truth = V.planted(7, 8, 6, 4, 3, 1500)
    rng = np.random.default_rng(1)
    lab = truth.copy()
    bad = rng.random(1500) < 0.2
    lab[bad] = rng.integers(0, 3, int(bad.sum()))
    return DiagGmmModel(w, mi, iv), IvecExtractorModel(M, np.stack([np.eye(6)] * 8), 0.0), x, truth, lab


def test_loop_follows_the_oracle():
    ubm, ie, x, truth, lab = planted()
    vb = ktf.diarization.VBResegmenter(ie, ubm, max_speakers=3, max_iters=3, stat_scale=1.0, downsample=1, num_slots=8)
    feats = d(np.stack([x, np.zeros_like(x), x[::-1]]))
    res = vb(feats, lengths=[1500, 0, 700], init_labels=np.concatenate([lab, lab[:700]]))
    assert res.offsets.tolist() == [0, 1500, 1500, 2200] and res.iters[0] == 3 and res.iters[1] == 0 and res.truncated_frames == 0
    g, p, ll, _ = vb.posteriors(d(x))
    m, _, B, UU = V.consts(ubm.means_invvars, ubm.inv_vars, np.asarray(ie.M))
    qw, sw, bw = V.run(x, g.cpu().numpy(), p.cpu().numpy(), ll.cpu().numpy(), m, B, UU, V.init_q(lab, 1500, 1, 3), np.full(3, 1 / 3),
                       max_iters=3)
    q = res.q.cpu().numpy()[:1500]
    bound = res.bound.cpu().numpy()
    eq, eb = float(np.abs(q - qw).max()), rel(bound[0], bw)
    s = np.sort(qw, 1)
    clear = s[:, -1] - s[:, -2] > 1e-5
    labels = res.labels.cpu().numpy()[:1500]
    print(f"vb loop: q {eq:.2e} (bound 1e-6), bound {eb:.2e} (1e-6 relative), excused {(~clear).mean():.4f}, "
          f"accuracy {(labels == truth).mean():.4f}")
    assert eq <= 1e-6 and eb <= 1e-6 and (~clear).mean() <= 0.01
    assert np.array_equal(labels[clear], qw.argmax(1)[clear])
    assert np.abs(res.sp.cpu().numpy()[0] - sw).max() <= 1e-6 and np.isnan(bound[1]).all()
    assert np.array_equal(res.sp.cpu().numpy()[1], np.full(3, 1 / 3)) and res.frame_q.shape == (2200, 3)
    # the first recording alone: the same bits
    alone = vb(feats[:1], init_labels=lab)
    assert np.array_equal(alone.q.cpu().numpy(), res.q.cpu().numpy()[:1500]) and np.array_equal(alone.bound.cpu().numpy()[0], bound[0])
    # from_posteriors is the same path; frame chunking changes no bit
    small = ktf.diarization.VBResegmenter(ie, ubm, max_speakers=3, max_iters=3, stat_scale=1.0, downsample=1, num_slots=8,
                                          workspace_limit=ops.vb_post_workspace_bytes(1, 8) * 333)
    again = small(feats[:1], init_labels=lab)
    fp = vb.from_posteriors(feats[:1], g, p, ll, init_labels=lab)
    assert np.array_equal(again.q.cpu().numpy(), alone.q.cpu().numpy()) and np.array_equal(fp.q.cpu().numpy(), alone.q.cpu().numpy())
    with pytest.raises(ValueError):
        vb(feats[:1], init_labels=lab[:10])
    with pytest.raises(ValueError):
        vb(feats[:1], q0=np.full((1500, 2), 0.5))
    with pytest.raises(ValueError):
        vb(feats[:1], sp0=np.array([0.5, 0.6, -0.1]))


def test_bits_do_not_depend_on_the_offset():
    """A recording that starts at an odd frame of the packed arrays, behind another one: the bits of it alone, the bound included."""
    ubm, ie, x, truth, lab = planted()
    vb = ktf.diarization.VBResegmenter(ie, ubm, max_speakers=3, max_iters=2, stat_scale=0.3, downsample=3, num_slots=8)
    alone = vb(d(x[None]), init_labels=lab)
    for lead in (701, 1, 2, 3):
        feats = d(np.stack([x[::-1], x]))
        res = vb(feats, lengths=[lead, 1500], init_labels=np.concatenate([lab[:lead], lab]))
        nb = (lead + 2) // 3
        assert res.offsets.tolist() == [0, lead, lead + 1500]
        assert np.array_equal(res.bound.cpu().numpy()[1], alone.bound.cpu().numpy()[0]), lead
        assert np.array_equal(res.q.cpu().numpy()[nb:], alone.q.cpu().numpy()) and np.array_equal(res.sp.cpu().numpy()[1], alone.sp.cpu().numpy()[0])
        assert np.array_equal(res.labels.cpu().numpy()[lead:], alone.labels.cpu().numpy())


def test_downsampled_blocks_and_random_start():
    ubm, ie, x, truth, lab = planted()
    vb = ktf.diarization.VBResegmenter(ie, ubm, max_speakers=3, max_iters=4, stat_scale=1.0, downsample=25, num_slots=8)
    res = vb(d(x[None, :1490]), init_labels=lab[:1490])
    assert res.q.shape == (60, 3) and np.array_equal(res.frame_q.cpu().numpy(), np.repeat(res.q.cpu().numpy(), 25, 0)[:1490])
    assert (res.labels.cpu().numpy() == truth[:1490]).mean() > 0.9
    b = res.bound.cpu().numpy()[0, :int(res.iters[0])]
    assert np.isfinite(b).all()
    rnd = vb(d(x[None, :1490]), seed=5)
    q0 = np.random.default_rng(5).gamma(100.0, size=(60, 3))
    same = vb(d(x[None, :1490]), q0=q0 / q0.sum(1, keepdims=True))
    assert np.array_equal(rnd.q.cpu().numpy(), same.q.cpu().numpy())


def test_trained_model_round_trip(tmp_path):
    _, _, x, _, lab = planted()
    feats = d(x[None])
    dubm, _ = training.init_diag_ubm(feats, 4, num_iters=2, seed=3)
    dubm, _ = training.train_diag_ubm(dubm, [(feats,)], gselect_n=3, num_iters=1)
    ie, _ = training.train_ivector_extractor(dict(diag_ubm=dubm, num_gselect=3), training.diag_to_full(dubm), [(feats[:, :750],), (feats[:, 750:],)],
                                             1, ivector_dim=3)
    WriteKaldiDiagGmm(str(tmp_path / "final.dubm"), dubm)
    WriteKaldiIvecExtractor(str(tmp_path / "final.ie"), ie)
    kw = dict(max_speakers=3, max_iters=2, downsample=5, num_slots=4)
    a = ktf.diarization.VBResegmenter(ie, dubm, **kw)(feats, init_labels=lab)
    b = ktf.diarization.VBResegmenter(str(tmp_path / "final.ie"), str(tmp_path / "final.dubm"), **kw)(feats, init_labels=lab)
    c = ktf.diarization.VBResegmenter(KaldiIvecExtractorReader(str(tmp_path / "final.ie")), KaldiDiagGmmReader(str(tmp_path / "final.dubm")),
                                      **kw)(feats, init_labels=lab)
    for r in (b, c):
        assert np.array_equal(r.q.cpu().numpy(), a.q.cpu().numpy()) and np.array_equal(r.bound.cpu().numpy(), a.bound.cpu().numpy(), equal_nan=True)
        assert np.array_equal(r.labels.cpu().numpy(), a.labels.cpu().numpy())
