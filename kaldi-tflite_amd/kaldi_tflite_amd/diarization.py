"""Extension: x-vector diarization on the device. Kaldi's `agglomerative-cluster` (single pass) over the blocks `PLDA.score_dense`
returns, batched over recordings; RTTM lines from window labels and the wav -> RTTM composition `diarize`
(INTEGRATION.md §2d)."""

import numbers

import numpy as np
import torch

from . import _lib as L
from . import ops
from .models import _Workspace

_ws = _Workspace()


def _blocks(scores):
    single = isinstance(scores, torch.Tensor)
    blocks = [scores] if single else list(scores) if isinstance(scores, (list, tuple)) else None
    if not blocks:
        raise ValueError(f"scores must be one (n, n) tensor or a non-empty list of them, got {type(scores).__name__}")
    for b in blocks:
        if not isinstance(b, torch.Tensor):
            raise ValueError(f"every block must be a torch tensor, got {type(b).__name__}")
        if b.dim() != 2 or b.shape[0] != b.shape[1] or b.shape[0] < 1:
            raise ValueError(f"every block must be square (n, n) with n >= 1, got {tuple(b.shape)}")
        if b.shape[0] > L.AHC_MAX_N:
            raise ValueError(f"a block has {b.shape[0]} rows, at most {L.AHC_MAX_N} per recording")
    dt = blocks[0].dtype
    if dt not in (torch.float32, torch.float64) or any(b.dtype != dt for b in blocks):
        raise ValueError(f"the blocks must all be float32 or all float64, got {sorted({str(b.dtype) for b in blocks})}")
    return single, blocks


def _packed(blocks):
    """The blocks as one 1-D tensor, n_r^2 values each: in place when they are consecutive views of one contiguous buffer
    (score_dense's output), otherwise one device copy."""
    b0 = blocks[0]
    ptr, es = b0.data_ptr(), b0.element_size()
    st = b0.untyped_storage().data_ptr()
    o = 0
    for b in blocks:
        if not b.is_contiguous() or b.untyped_storage().data_ptr() != st or b.data_ptr() != ptr + o * es:
            return torch.cat([b.reshape(-1) for b in blocks])
        o += b.numel()
    return torch.as_strided(b0, (o,), (1,), b0.storage_offset())


def _real(v):
    return isinstance(v, numbers.Real) and not isinstance(v, (bool, np.bool_))


def agglomerative_cluster(scores, threshold=None, num_speakers=None, max_spk_fraction=1.0, read_costs=False):
    """Kaldi's `agglomerative-cluster` (AgglomerativeClusterer, single pass) on the device.

    scores: one (n, n) tensor, or a list of R (n_r, n_r) tensors (e.g. `PLDA.score_dense(..., lengths=...)`'s output), all
    float32 or all float64 on one GPU. Costs are -scores (read_costs=False, Kaldi's default) or the scores themselves; only the
    strict upper triangle is read. The pair of clusters with the smallest average cost is merged while
    - threshold mode (num_speakers None): that average is <= threshold (None: 0.0, Kaldi's default), down to one cluster;
    - num_speakers mode (an int, or R ints: Kaldi's reco2num_spk): until num_speakers[r] clusters remain, no merged cluster
      larger than ceil(n * max_spk_fraction) (which can leave more clusters, as in Kaldi).
    -> (labels, counts): labels 1 .. K per row, int32 on the device, (n,) for one tensor or a list of R (n_r,) views of one
    allocation; counts (R,) int32 = K per recording. Nothing is read back to the host."""
    single, blocks = _blocks(scores)
    R = len(blocks)
    if not isinstance(read_costs, (bool, np.bool_)):
        raise ValueError(f"read_costs must be a bool, got {read_costs!r}")
    if not _real(max_spk_fraction) or not 0.0 < float(max_spk_fraction) <= 1.0:
        raise ValueError(f"max_spk_fraction must be in (0, 1], got {max_spk_fraction!r}")
    if num_speakers is None:
        if float(max_spk_fraction) != 1.0:
            raise ValueError("max_spk_fraction applies with num_speakers only (Kaldi's threshold mode has no size limit)")
        if threshold is None:
            threshold = 0.0
        if not _real(threshold) or np.isnan(float(threshold)):
            raise ValueError(f"threshold must be a number, got {threshold!r}")
        min_clusters = None
    else:
        if threshold is not None:
            raise ValueError("give threshold or num_speakers, not both")
        if isinstance(num_speakers, (numbers.Integral, np.integer)) and not isinstance(num_speakers, (bool, np.bool_)):
            ns = [int(num_speakers)] * R
        else:
            arr = np.asarray(num_speakers.tolist() if isinstance(num_speakers, torch.Tensor) else num_speakers)
            if arr.ndim != 1 or arr.size != R or arr.dtype.kind not in "iu":
                raise ValueError(f"num_speakers must be an int or {R} ints, got {num_speakers!r}")
            ns = [int(v) for v in arr]
        if min(ns) < 1 or max(ns) > np.iinfo(np.int32).max:
            raise ValueError(f"num_speakers must be >= 1, got {ns}")
        min_clusters = ns
        threshold = float(np.finfo(np.float64 if blocks[0].dtype == torch.float64 else np.float32).max)
    dev = blocks[0].device
    if dev.type != "cuda" or any(b.device != dev for b in blocks):
        raise ValueError(f"the blocks must all be on one GPU, got {sorted({str(b.device) for b in blocks})}")
    lens = [int(b.shape[0]) for b in blocks]
    packed = _packed(blocks)
    labels, counts = ops.ahc(packed, lens, threshold, min_clusters, float(max_spk_fraction), bool(read_costs),
                             scratch=lambda role, shp, dt: _ws.get(role, shp, dt, dev, padded=False))
    if single:
        return labels, counts
    out, o = [], 0
    for n in lens:
        out.append(labels[o:o + n])
        o += n
    return out, counts


def _labels_host(labels, S):
    """labels: one (S,) tensor / array, or a list of per-recording ones laid end to end -> (S,) host int64."""
    parts = list(labels) if isinstance(labels, (list, tuple)) else [labels]
    arrs = [np.asarray(p.cpu() if isinstance(p, torch.Tensor) else p).reshape(-1) for p in parts]
    out = np.concatenate(arrs) if arrs else np.zeros(0, np.int64)
    if out.size != S:
        raise ValueError(f"{out.size} labels for {S} windows")
    if out.size and out.dtype.kind not in "iu":
        raise ValueError(f"labels must be integers, got {out.dtype}")
    return out.astype(np.int64)


def rttm_pieces(starts, ends, labels):
    """Kaldi make_rttm.py's rule on one recording's windows in start order (times in any unit): where a window ends after the next
    one starts, both boundaries move to the midpoint (a window whose start already moved keeps that start); then consecutive pieces
    that touch (end == next start) and carry the same label merge. -> [(start, end, label)]."""
    st = [float(v) for v in starts]
    en = [float(v) for v in ends]
    for i in range(len(st) - 1):
        if en[i] > st[i + 1]:
            mid = (en[i] + st[i + 1]) / 2.0
            en[i] = st[i + 1] = mid
    out = []
    for a, b, lab in zip(st, en, labels):
        if out and out[-1][1] == a and out[-1][2] == lab:
            out[-1][1] = b
        else:
            out.append([a, b, lab])
    return [tuple(p) for p in out]


def rttm(res, labels, reco_ids=None, channel=1):
    """RTTM lines of `res` (XvectorExtractor.extract_windows' result) and one label per window: one (S,) tensor, or per-recording
    tensors laid end to end (agglomerative_cluster's list). Per recording, windows in start order, rttm_pieces' rule, then one line
    `SPEAKER <reco> <channel> <start> <duration> <NA> <NA> <label> <NA> <NA>` per piece, seconds with three decimals. reco_ids: R
    names (default reco0, reco1, ...). Reads the window table and the labels back to the host; returns a list of str."""
    R = len(res.lengths)
    if reco_ids is None:
        reco_ids = [f"reco{r}" for r in range(R)]
    reco_ids = list(reco_ids)
    if len(reco_ids) != R:
        raise ValueError(f"{len(reco_ids)} reco_ids for {R} recordings")
    win = res.windows.cpu().numpy().astype(np.int64).reshape(-1, 3)
    lab = _labels_host(labels, win.shape[0])
    shift = float(res.frame_shift)
    lines = []
    for r in range(R):
        sel = np.nonzero(win[:, 0] == r)[0]
        if sel.size == 0:
            continue
        order = sel[np.argsort(win[sel, 1], kind="stable")]
        for a, b, k in rttm_pieces(win[order, 1], win[order, 2], lab[order]):
            lines.append(f"SPEAKER {reco_ids[r]} {channel} {a * shift:.3f} {(b - a) * shift:.3f} <NA> <NA> {int(k)} <NA> <NA>")
    return lines


class Diarization:
    """diarize's result: windows (extract_windows' WindowXvectors), labels (S,) int32 and counts (R,) int32 (speakers per recording, 0
    for a recording without windows) on the GPU, rttm (list of str)."""

    def __init__(self, windows, labels, counts, rttm_lines):
        self.windows, self.labels, self.counts, self.rttm = windows, labels, counts, rttm_lines


def diarize(ext, plda, wavs, target_energy=0.1, threshold=None, num_speakers=None, max_spk_fraction=1.0, segments=None, window=1.5,
            period=0.75, min_segment=0.5, reco_ids=None):
    """wav -> RTTM: ext.extract_windows -> plda.score_dense (the recordings with windows) -> agglomerative_cluster -> rttm.
    num_speakers: None (threshold mode), an int, or R ints (one per recording of wavs). Recordings without windows are left out of
    scoring and clustering and produce no lines."""
    res = ext.extract_windows(wavs, window=window, period=period, min_segment=min_segment, segments=segments)
    R = len(res.lengths)
    live = [r for r in range(R) if res.lengths[r] > 0]
    dev = res.xvectors.device
    counts = torch.zeros((R,), dtype=torch.int32, device=dev)
    if not live:
        labels = torch.zeros((0,), dtype=torch.int32, device=dev)
        return Diarization(res, labels, counts, [])
    ns = num_speakers
    if ns is not None and not isinstance(ns, (numbers.Integral, np.integer)):
        arr = list(ns.tolist() if isinstance(ns, torch.Tensor) else ns)
        if len(arr) != R:
            raise ValueError(f"num_speakers must be an int or {R} ints, got {num_speakers!r}")
        ns = [arr[r] for r in live]
    scores = plda.score_dense(res.xvectors, lengths=[res.lengths[r] for r in live], target_energy=target_energy)
    labels, cnt = agglomerative_cluster(scores, threshold=threshold, num_speakers=ns, max_spk_fraction=max_spk_fraction)
    labels = torch.cat(labels) if len(labels) > 1 else labels[0]
    counts[torch.as_tensor(live, device=dev)] = cnt
    return Diarization(res, labels, counts, rttm(res, labels, reco_ids))
