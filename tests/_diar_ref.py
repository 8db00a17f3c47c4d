"""NumPy restatement of sliding-window x-vector extraction for diarization, built from oracle/ktf_oracle.py:
whole-recording framing + MFCC, energy VAD -> runs of voiced frames, CMVN per segment, the window rule, sequential_forward +
xvector_post per window, and the RTTM rule of Kaldi's make_rttm.py. Independent of the package on purpose."""

import math

import numpy as np

from oracle import ktf_oracle as O


def frames_of(x, shift):
    return int(math.floor(x / shift + 0.5))


def window_rule(s, e, W, P, M):
    """The windows [a, b) of segment [s, e), by the loop."""
    out, a, L = [], s, e - s
    while L > W + M:
        out.append((a, a + W))
        a += P
        L -= P
    out.append((a, e))
    return out


def window_count(L, W, P, M):
    return 1 + max(0, math.ceil((L - W - M) / P))


def runs(mask):
    """Maximal runs of True -> [(start, end)]."""
    m = np.concatenate([[False], np.asarray(mask, bool), [False]])
    d = np.diff(m.astype(np.int8))
    return list(zip(np.nonzero(d == 1)[0].tolist(), np.nonzero(d == -1)[0].tolist()))


def mfcc(wav, cfg, dtype=np.float32):
    """(T, D) MFCC of one whole recording (snip_edges=False: mirror-padded first, as the framing layer does)."""
    fcfg = {k: v for k, v in cfg["framing"].items() if k not in ("dynamic_input_shape", "snip_edges")}
    x = np.asarray(wav, dtype)[None]
    if cfg["framing"].get("snip_edges", True) is False:
        size, shift, _ = O.frame_params(**fcfg)
        half = size // 2
        x = O.pad_waveform(x, 2 * half, shift)
    return O.mfcc(O.framing(x, **fcfg), **cfg["mfcc"], dtype=dtype)[0]


def vad_segments(m, cfg, dtype=np.float32):
    vcfg = dict(cfg["vad"])
    vcfg["return_indexes"] = False
    mask = O.vad(np.asarray(m, dtype)[None], **vcfg, dtype=dtype)[0, :, 0] > 0
    return runs(mask)


def caller_segments(pairs, T, shift):
    return [(frames_of(a, shift), min(frames_of(b, shift), T)) for a, b in pairs]


def windows(segs, W, P, M):
    return [w for s, e in segs for w in window_rule(s, e, W, P, M)]


def cmn(m, segs, cfg, dtype=np.float32):
    """CMVN of each segment's rows, written at the same frames (rows outside every segment: NaN)."""
    out = np.full(np.shape(m), np.nan, dtype)
    for s, e in segs:
        out[s:e] = O.cmvn(np.asarray(m[s:e], dtype)[None], **cfg["cmvn"], dtype=dtype)[0]
    return out


def xvectors(c, wins, layers, mean, lda, dtype=np.float64):
    """One x-vector per window [a, b) of the CMN'd frames c."""
    out = []
    for a, b in wins:
        h = O.sequential_forward(layers, np.asarray(c[a:b], dtype)[None], dtype=dtype)
        out.append(O.xvector_post(h, mean, lda, dtype=dtype)[0])
    return np.stack(out, 0) if out else np.zeros((0, lda.shape[0]), dtype)


def recording(wav, cfg, W, P, M, pairs=None):
    """fp32 tables of one recording: (T, segments, windows)."""
    shift = cfg["framing"]["frame_shift_ms"] / 1000.0
    m = mfcc(wav, cfg)
    T = m.shape[0]
    segs = vad_segments(m, cfg) if pairs is None else caller_segments(pairs, T, shift)
    return T, segs, windows(segs, W, P, M)


def rttm_pieces(starts, ends, labels):
    st, en = [float(v) for v in starts], [float(v) for v in ends]
    for i in range(len(st) - 1):
        if en[i] > st[i + 1]:
            st[i + 1] = en[i] = (en[i] + st[i + 1]) / 2
    out = []
    for a, b, k in zip(st, en, labels):
        if out and out[-1][1] == a and out[-1][2] == k:
            out[-1] = (out[-1][0], b, k)
        else:
            out.append((a, b, k))
    return out


def rttm_line(reco, a, b, k, shift, channel=1):
    return "SPEAKER %s %d %.3f %.3f <NA> <NA> %d <NA> <NA>" % (reco, channel, a * shift, (b - a) * shift, k)
