"""Sliding-window x-vectors for diarization (XvectorExtractor.extract_windows, csrc/diar_windows.hip) and the wav -> RTTM chain on
the MI355X: segment and window tables equal the NumPy restatement (tests/_diar_ref.py) exactly, the MFCC and the per-segment CMN
equal the existing layers bit for bit, window x-vectors are within 1e-4 of the fp64 restatement in every compliant mode, exact fp32
does not depend on the pass or the batch, and diarize equals the composition of its steps."""

import os

import numpy as np
import pytest
import torch

import _diar_ref as R
import synth
import kaldi_tflite_amd as ktf
from oracle import ktf_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4
DEV = "cuda:0"
COMPLIANT = ["f32", "bf16x3"] + (["f16mx"] if "f16mx" in ktf.layers._GEMM else [])
SEEDS = [4321, 1]
WPM = (150, 75, 50)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_ext = {}


def extractor(gemm="f32", seed=4321, cfg=None, feat_dim=30):
    key = (gemm, seed, None if cfg is None else repr(cfg), feat_dim)
    if key not in _ext:
        w = synth.make_weights(seed=seed, feat_dim=feat_dim)
        _ext[key] = (synth.build_extractor(ktf, cfg or synth.extractor_cfg(), w, gemm=gemm), w)
    return _ext[key]


def inputs():
    whole, _ = synth.speech_wavs()
    return {"speech_22s": whole[0], "speech_3s": synth.second_speech_wav(), "coloured_am_noise": synth.coloured_am_noise(1, 160000)[0]}


def tables(res):
    return res.segments.cpu().numpy().tolist(), res.windows.cpu().numpy().tolist()


def want_tables(wavs, cfg=None, pairs=None):
    cfg = cfg or synth.extractor_cfg()
    segs, wins, lengths = [], [], []
    for r, wav in enumerate(wavs):
        _, s, w = R.recording(wav, cfg, *WPM, pairs=None if pairs is None else pairs[r])
        segs += [[r, a, b] for a, b in s]
        wins += [[r, a, b] for a, b in w]
        lengths.append(len(w))
    return segs, wins, lengths


def ws_view(ext, role, n, dtype=torch.float32):
    """The call's workspace buffer `role` (the same view extract_windows used: same shape and dtype)."""
    return ext._ws.get(role, (n,), dtype, torch.device(DEV), padded=False)


def test_librispeech_vad_segments_and_whole_recording_fixture():
    ext, _ = extractor()
    wav = inputs()["speech_22s"]
    res = ext.extract_windows(wav)
    segs, wins = tables(res)
    assert [b - a for _, a, b in segs] == [193, 136, 322, 311, 133, 180, 115, 54, 301, 68]
    ws, ww, wl = want_tables([wav])
    assert segs == ws and wins == ww and res.lengths == wl == [16]
    assert res.xvectors.shape == (16, ext.ldaMat.shape[1]) and res.windows.dtype == torch.int32
    # one caller segment over the whole recording: the reference's 29 subsegments, the last end clamped to 2246
    names = open(os.path.join(GOLDEN, "subsegments_librispeech_2.txt")).read().split()
    fixture = [[0, int(n.split("-")[1]), min(int(n.split("-")[2]), 2246)] for n in names]
    res2 = ext.extract_windows(wav, segments=[[(0.0, 22.48)]])
    assert tables(res2) == ([[0, 0, 2246]], fixture) and res2.lengths == [29]


def test_batch_of_three_recordings_vad_and_caller_segments():
    ext, _ = extractor()
    x = inputs()
    wavs = [x["speech_3s"], x["speech_22s"][:250000], x["coloured_am_noise"]]
    res = ext.extract_windows(wavs)
    ws, ww, wl = want_tables(wavs)
    assert tables(res) == (ws, ww) and res.lengths == wl
    pairs = [[(0.1, 1.2), (1.2, 2.9)], [], [(0.0, 0.013), (0.5, 4.37), (5.0, 99.0)]]
    res2 = ext.extract_windows(wavs, segments=pairs)
    ws, ww, wl = want_tables(wavs, pairs=pairs)
    assert tables(res2) == (ws, ww) and res2.lengths == wl and wl[1] == 0


def test_device_window_rule_hand_cases():
    """The device windows kernel on caller segments of hand-worked lengths: L = 1, W + M, W + M + 1, and P not dividing L - W."""
    ext, _ = extractor()
    wav = inputs()["speech_22s"]
    res = ext.extract_windows(wav, segments=[[(0.0, 0.01), (0.5, 2.5), (3.0, 5.01), (6.0, 9.0)]])
    assert tables(res)[1] == [[0, 0, 1], [0, 50, 250], [0, 300, 450], [0, 375, 501],
                              [0, 600, 750], [0, 675, 825], [0, 750, 900]]
    assert res.lengths == [7]
    res = ext.extract_windows(wav, window=1.0, period=0.3, min_segment=0.2, segments=[[(6.0, 9.0), (10.0, 11.71)]])
    assert tables(res)[1] == [[0, 600, 700], [0, 630, 730], [0, 660, 760], [0, 690, 790], [0, 720, 820], [0, 750, 850], [0, 780, 900],
                              [0, 1000, 1100], [0, 1030, 1130], [0, 1060, 1171]]
    assert res.lengths == [10]
    check_xvectors("f32", 4321, [wav], res)


def test_mfcc_and_segment_cmn_bits():
    """The call's MFCC stream equals features() of each recording alone and its CMN'd stream equals ktf.layers.CMVN on each
    segment's rows, bit for bit (and the fp32 oracle's CMVN of those rows within 1e-5 of their scale: its
    window sums are differences of cumulative sums); snip_edges=False too, where padding would move the last frames."""
    for snip in (True, False):
        cfg = synth.extractor_cfg()
        cfg["framing"]["snip_edges"] = snip
        ext, _ = extractor(cfg=cfg)
        x = inputs()
        wavs = [x["speech_3s"][:47950], x["speech_22s"][:160000], x["coloured_am_noise"][:99999]]
        res = ext.extract_windows(wavs)
        frames = [ext.framing.numFrames(len(w)) for w in wavs]
        F, D = sum(frames), ext.mfcc.numMfccs
        mf = ws_view(ext, "dw_mfcc", F * D + 4)[:F * D].view(F, D).clone()
        cm = ws_view(ext, "dw_cmn", F * D + 4)[:F * D].view(F, D).clone()
        cmvn = ktf.layers.CMVN(**cfg["cmvn"])
        off = np.concatenate([[0], np.cumsum(frames)])
        ws, ww, _ = want_tables(wavs, cfg=cfg)
        assert tables(res) == (ws, ww)
        for r, wav in enumerate(wavs):
            want = ext.features(torch.as_tensor(wav[None], device=DEV))[0][0]
            assert torch.equal(mf[off[r]:off[r + 1]], want), (snip, r)
            segs = [(a, b) for rr, a, b in ws if rr == r]
            ref = R.cmn(want.cpu().numpy(), segs, cfg)             # (the oracle's CMVN of the same MFCC rows)
            for a, b in segs:
                got = cm[off[r] + a:off[r] + b]
                assert torch.equal(got, cmvn(mf[off[r] + a:off[r] + b][None])[0]), (snip, r, a, b)
                assert np.abs(got.cpu().numpy() - ref[a:b]).max() <= 1e-5 * max(1.0, float(np.abs(ref[a:b]).max()))


def check_xvectors(gemm, seed, wavs, res, cfg=None, pairs=None, tol=TOL):
    cfg = cfg or synth.extractor_cfg()
    _, w = extractor(gemm, seed, None, w_dim(cfg))
    layers = synth.oracle_layers(w)
    got = res.xvectors.cpu().numpy()
    win = res.windows.cpu().numpy()
    worst = 0.0
    for r, wav in enumerate(wavs):
        m = R.mfcc(wav, cfg, dtype=np.float64)
        segs = [(a, b) for rr, a, b in res.segments.cpu().numpy().tolist() if rr == r]
        c = R.cmn(m, segs, cfg, dtype=np.float64)
        sel = np.nonzero(win[:, 0] == r)[0]
        want = R.xvectors(c, [(int(a), int(b)) for _, a, b in win[sel]], layers, w["mean"], w["lda"])
        if sel.size:
            worst = max(worst, float(np.abs(got[sel] - want).max()))
    assert np.isfinite(got).all()
    assert worst <= tol, (gemm, seed, worst)
    return worst


def w_dim(cfg):
    return cfg["mfcc"]["num_mfccs"]


@pytest.mark.parametrize("gemm", COMPLIANT)
@pytest.mark.parametrize("seed", SEEDS)
def test_window_xvectors_against_fp64(gemm, seed):
    ext, _ = extractor(gemm, seed)
    for name, wav in inputs().items():
        res = ext.extract_windows(wav)
        assert res.lengths[0] > 0, name
        check_xvectors(gemm, seed, [wav], res)


def test_short_caller_segments_and_silent_recording():
    ext, _ = extractor("f32")
    x = inputs()
    wavs = [x["speech_3s"], np.zeros(32000, np.float32), x["speech_22s"][:100000]]
    pairs = [[(0.5, 0.51), (0.6, 0.62), (0.7, 0.73), (1.0, 2.6)], [(0.0, 1.0)], [(0.2, 0.21), (1.0, 6.0)]]
    res = ext.extract_windows(wavs, segments=pairs)
    assert [b - a for _, a, b in res.windows.cpu().numpy().tolist()[:3]] == [1, 2, 3]
    check_xvectors("f32", 4321, wavs, res)
    res2 = ext.extract_windows(wavs)                                    # VAD: the silent recording has no segment
    assert res2.lengths[1] == 0 and res2.lengths[0] > 0 and res2.lengths[2] > 0
    assert int((res2.windows[:, 0] == 1).sum()) == 0 and int((res2.segments[:, 0] == 1).sum()) == 0
    check_xvectors("f32", 4321, wavs, res2)
    empty = ext.extract_windows(np.zeros(16000, np.float32))
    assert empty.lengths == [0] and empty.xvectors.shape == (0, ext.ldaMat.shape[1]) and empty.windows.shape == (0, 3)


def test_exact_fp32_is_independent_of_the_pass_and_the_batch():
    ext, _ = extractor("f32")
    x = inputs()
    wavs = [x["speech_22s"], x["coloured_am_noise"], x["speech_3s"]]
    base = ext.extract_windows(wavs)
    for k in (1, 7):
        assert torch.equal(ext.extract_windows(wavs, max_windows_per_pass=k).xvectors, base.xvectors), k
    single = torch.cat([ext.extract_windows(w).xvectors for w in wavs])
    assert torch.equal(single, base.xvectors)
    same = torch.as_tensor(np.stack([x["speech_22s"][:160000], x["coloured_am_noise"]]), device=DEV)   # (R, N): one front-end launch
    both = ext.extract_windows(same)
    assert torch.equal(both.xvectors, torch.cat([ext.extract_windows(same[0]).xvectors, ext.extract_windows(same[1]).xvectors]))


def test_8khz_front_end_whole_path():
    cfg = synth.extractor_cfg_8k()
    ext, _ = extractor("f32", 4321, cfg, 23)
    wav = np.round(inputs()["speech_22s"][::2]).astype(np.float32)
    res = ext.extract_windows(torch.as_tensor(wav.astype(np.int16), device=DEV))
    ws, ww, wl = want_tables([wav], cfg=cfg)
    assert tables(res) == (ws, ww) and res.lengths == wl and wl[0] > 0
    check_xvectors("f32", 4321, [wav], res, cfg=cfg)


def test_invalid_arguments():
    ext, _ = extractor("f32")
    wav = inputs()["speech_3s"]
    for kw in ({"window": 0}, {"period": 2.0}, {"min_segment": -1}, {"max_windows_per_pass": 0},
               {"segments": [[(1.0, 0.5)]]}, {"segments": [[(0.0, 1.0), (0.5, 2.0)]]}, {"segments": [[(5.0, 6.0)]]}):
        with pytest.raises(ValueError):
            ext.extract_windows(wav, **kw)


def test_diarize_equals_its_steps():
    ext, _ = extractor("f32")
    odim = ext.ldaMat.shape[1]
    rng = np.random.default_rng(5)
    T = rng.standard_normal((odim, odim)) / np.sqrt(odim) + np.eye(odim)
    plda = ktf.layers.PLDA(odim, rng.standard_normal(odim) * 0.1, T, np.sort(rng.uniform(0.05, 30.0, odim))[::-1].copy(), dtype="float32")
    x = inputs()
    wavs = [x["speech_22s"], np.zeros(20000, np.float32), x["coloured_am_noise"]]
    out = ktf.diarization.diarize(ext, plda, wavs, threshold=0.0, reco_ids=["a", "b", "c"])
    res = ext.extract_windows(wavs)
    assert torch.equal(out.windows.xvectors, res.xvectors) and out.windows.lengths == res.lengths and res.lengths[1] == 0
    live = [n for n in res.lengths if n]
    labels, counts = ktf.diarization.agglomerative_cluster(plda.score_dense(res.xvectors, lengths=live, target_energy=0.1), threshold=0.0)
    assert torch.equal(out.labels, torch.cat(labels)) and out.counts.cpu().tolist() == [counts.cpu().tolist()[0], 0, counts.cpu().tolist()[1]]
    assert out.rttm == ktf.diarization.rttm(res, labels, reco_ids=["a", "b", "c"])
    assert not any(l.split()[1] == "b" for l in out.rttm)
    one = ktf.diarization.diarize(ext, plda, wavs, num_speakers=1)
    assert one.counts.cpu().tolist() == [1, 0, 1] and set(one.labels.cpu().tolist()) == {1}
    win = res.windows.cpu().numpy()
    for r, reco in ((0, "reco0"), (2, "reco2")):
        # the lines are the union of the recording's windows: touching or overlapping windows merged, gaps kept
        iv = sorted((int(a), int(b)) for rr, a, b in win if rr == r)
        union = []
        for a, b in iv:
            if union and a <= union[-1][1]:
                union[-1][1] = max(union[-1][1], b)
            else:
                union.append([a, b])
        want = ["SPEAKER %s 1 %.3f %.3f <NA> <NA> 1 <NA> <NA>" % (reco, a * 0.01, (b - a) * 0.01) for a, b in union]
        assert [l for l in one.rttm if l.split()[1] == reco] == want
