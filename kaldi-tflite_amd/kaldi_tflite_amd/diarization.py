"""Extension: x-vector diarization on the device. Kaldi's `agglomerative-cluster` (single pass) over the blocks `PLDA.score_dense`
returns, batched over recordings; RTTM lines from window labels and the wav -> RTTM composition `diarize`
(INTEGRATION.md §2d); the VB-HMM resegmentation of frames (§2j) and VBx, the VB-HMM over the window x-vectors (§2k)."""

import numbers

import numpy as np
import torch

from . import _lib as L
from . import ops
from ._host import chunks, host, is_int, is_real, per_device
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
    if not is_real(max_spk_fraction) or not 0.0 < float(max_spk_fraction) <= 1.0:
        raise ValueError(f"max_spk_fraction must be in (0, 1], got {max_spk_fraction!r}")
    if num_speakers is None:
        if float(max_spk_fraction) != 1.0:
            raise ValueError("max_spk_fraction applies with num_speakers only (Kaldi's threshold mode has no size limit)")
        if threshold is None:
            threshold = 0.0
        if not is_real(threshold) or np.isnan(float(threshold)):
            raise ValueError(f"threshold must be a number, got {threshold!r}")
        min_clusters = None
    else:
        if threshold is not None:
            raise ValueError("give threshold or num_speakers, not both")
        if is_int(num_speakers):
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
    arrs = [host(p).reshape(-1) for p in parts]
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
    for a recording without windows) on the GPU, rttm (list of str). With diarize(vbx=...) labels, counts and rttm are VBx's,
    ahc_labels (S,) keeps the clustering's labels and vbx the VBxResult; otherwise both are None."""

    def __init__(self, windows, labels, counts, rttm_lines, ahc_labels=None, vbx=None):
        self.windows, self.labels, self.counts, self.rttm = windows, labels, counts, rttm_lines
        self.ahc_labels, self.vbx = ahc_labels, vbx


def diarize(ext, plda, wavs, target_energy=0.1, threshold=None, num_speakers=None, max_spk_fraction=1.0, segments=None, window=1.5,
            period=0.75, min_segment=0.5, reco_ids=None, vbx=None):
    """wav -> RTTM: ext.extract_windows -> plda.score_dense (the recordings with windows) -> agglomerative_cluster -> rttm.
    num_speakers: None (threshold mode), an int, or R ints (one per recording of wavs). Recordings without windows are left out of
    scoring and clustering and produce no lines. vbx: a VBx to run on the window x-vectors from the clustering's labels (the windows
    of a recording must be in time order, as extract_windows lists them); the result's labels, counts and rttm are then VBx's."""
    if vbx is not None and not isinstance(vbx, VBx):
        raise ValueError(f"vbx must be a VBx, got {type(vbx).__name__}")
    res = ext.extract_windows(wavs, window=window, period=period, min_segment=min_segment, segments=segments)
    R = len(res.lengths)
    live = [r for r in range(R) if res.lengths[r] > 0]
    dev = res.xvectors.device
    counts = torch.zeros((R,), dtype=torch.int32, device=dev)
    if not live:
        labels = torch.zeros((0,), dtype=torch.int32, device=dev)
        return Diarization(res, labels, counts, [], ahc_labels=None if vbx is None else labels)
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
    if vbx is not None:
        out = vbx(res.xvectors, res.lengths, init_labels=labels)
        return Diarization(res, out.labels, out.counts, rttm(res, out.labels, reco_ids), ahc_labels=labels, vbx=out)
    return Diarization(res, labels, counts, rttm(res, labels, reco_ids))


# =============================================================================== VB-HMM resegmentation
def frame_labels(res, labels, num_frames, frame_shift=0.01):
    """Per-frame initial labels for VBResegmenter from `res` (XvectorExtractor.extract_windows' result) and one label per window
    (agglomerative_cluster's, 1 .. K): per recording the windows in start order under rttm_pieces' midpoint rule; frame t (its start,
    t * frame_shift seconds) takes the label of the piece that holds it, minus 1 (the resegmenter counts speakers from 0), and -1
    outside every piece. num_frames: R frame counts (or one int for all). -> a list of R host int32 arrays."""
    R = len(res.lengths)
    nf = [int(num_frames)] * R if isinstance(num_frames, (numbers.Integral, np.integer)) else [int(v) for v in num_frames]
    if len(nf) != R or min(nf, default=0) < 0:
        raise ValueError(f"num_frames must be an int or {R} non-negative ints, got {num_frames!r}")
    if not is_real(frame_shift) or not float(frame_shift) > 0:
        raise ValueError(f"frame_shift must be > 0, got {frame_shift!r}")
    win = res.windows.cpu().numpy().astype(np.int64).reshape(-1, 3)
    lab = _labels_host(labels, win.shape[0])
    scale = float(res.frame_shift) / float(frame_shift)         # window units -> frames of the caller
    out = []
    for r in range(R):
        o = np.full(nf[r], -1, np.int32)
        sel = np.nonzero(win[:, 0] == r)[0]
        order = sel[np.argsort(win[sel, 1], kind="stable")]
        for a, b, k in rttm_pieces(win[order, 1], win[order, 2], lab[order]):
            lo, hi = int(np.ceil(a * scale - 1e-9)), int(np.ceil(b * scale - 1e-9))     # frames with a <= t < b
            o[max(lo, 0):max(min(hi, nf[r]), 0)] = int(k) - 1
        out.append(o)
    return out


def frame_rttm(labels, offsets, frame_index=None, frame_shift=0.01, reco_ids=None, channel=1):
    """RTTM lines from per-frame labels (VBResult.labels): labels (F,) for the recordings' rows end to end, recording r owning rows
    [offsets[r], offsets[r + 1]). frame_index (F,): the original frame of every row within its recording when a mask selected the
    rows (default: row - offsets[r]). Runs of equal labels over consecutive frame indices merge into one line in rttm's format,
    speaker = label + 1 (agglomerative_cluster's numbering); rows with a negative label give no line."""
    lab = host(labels).reshape(-1).astype(np.int64)
    off = host(offsets).reshape(-1).astype(np.int64)
    if off.size < 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != lab.size:
        raise ValueError(f"offsets must ascend from 0 to {lab.size}, got {off.tolist()}")
    R = off.size - 1
    if frame_index is None:
        idx = np.arange(lab.size, dtype=np.int64) - np.repeat(off[:-1], np.diff(off))
    else:
        idx = host(frame_index).reshape(-1).astype(np.int64)
        if idx.size != lab.size:
            raise ValueError(f"{idx.size} frame indices for {lab.size} labels")
    reco_ids = [f"reco{r}" for r in range(R)] if reco_ids is None else list(reco_ids)
    if len(reco_ids) != R:
        raise ValueError(f"{len(reco_ids)} reco_ids for {R} recordings")
    shift = float(frame_shift)
    lines = []
    for r in range(R):
        l, i = lab[off[r]:off[r + 1]], idx[off[r]:off[r + 1]]
        if l.size == 0:
            continue
        cut = np.nonzero((l[1:] != l[:-1]) | (i[1:] != i[:-1] + 1))[0] + 1
        for a, b in zip(np.concatenate([[0], cut]), np.concatenate([cut, [l.size]])):
            if l[a] < 0:
                continue
            st, en = i[a], i[b - 1] + 1
            lines.append(f"SPEAKER {reco_ids[r]} {channel} {st * shift:.3f} {(en - st) * shift:.3f} <NA> <NA> {int(l[a]) + 1} <NA> <NA>")
    return lines


def _vb_iterate(step, q, sp, row_offsets, max_iters, epsilon):
    """The VB-HMM outer loop of VBResegmenter and VBx. q (rows, K) and sp (N, K) on the device are the start; recording r owns the
    rows row_offsets[r] .. row_offsets[r + 1] (host ints) and runs while it has any. step(q, sp) -> (q_new, sp_new, bound (N,) on
    the device) is one iteration for all recordings; a recording is frozen after the iteration whose bound gains less than epsilon
    (that iteration's q and sp are kept) or after max_iters. One device -> host read per iteration; `step` is never called when no
    recording has rows. -> (q, sp, bound (N, max_iters) NaN-padded, iters (N,) int64), the last two on the host."""
    counts = np.diff(row_offsets)
    N = counts.size
    bound = np.full((N, max_iters), np.nan)
    iters = np.zeros(N, np.int64)
    active = counts > 0
    prev = np.full(N, np.nan)
    if not active.any():
        return q, sp, bound, iters
    rec_of_row = torch.as_tensor(np.repeat(np.arange(N), counts), device=q.device)
    for it in range(max_iters):
        qn, spn, Ld = step(q, sp)
        Lr = Ld.cpu().numpy()                                   # the iteration's one device -> host read
        if active.all():
            q, sp = qn, spn
        else:
            act = torch.as_tensor(active, device=q.device)
            q = torch.where(act[rec_of_row][:, None], qn, q)
            sp = torch.where(act[:, None], spn, sp)
        bound[active, it] = Lr[active]
        iters[active] = it + 1
        if it > 0:
            active = active & ~(Lr - prev < epsilon)
        prev = np.where(active, Lr, prev)
        if not active.any():
            break
    return q, sp, bound, iters


class VBResult:
    """VBResegmenter's result: q (sum T', K) fp64 block posteriors packed over the recordings, frame_q (F, K) the block rows
    repeated per frame, labels (F,) int32 (arg-max, ties to the lower index), sp (N, K), bound (N, max_iters) NaN-padded, all on the
    GPU; iters (N,) and offsets (N + 1) host int64 (recording r owns frames offsets[r] .. offsets[r + 1]); truncated_frames int."""

    def __init__(self, q, frame_q, labels, sp, bound, iters, truncated_frames, offsets):
        self.q, self.frame_q, self.labels, self.sp, self.bound = q, frame_q, labels, sp, bound
        self.iters, self.truncated_frames, self.offsets = iters, truncated_frames, offsets


class VBResegmenter:
    """Extension: the VB-HMM resegmentation of Kaldi's diarization/VB_resegmentation.sh (VB_diarization.py, Diez / Burget) on the
    GPU, at any frame rate and batched over recordings. `ie`: a path to `final.ie`, an io.KaldiIvecExtractorReader or the
    io.IvecExtractorModel training returns; `dubm`: a path to `final.dubm`, an io.KaldiDiagGmmReader or an io.DiagGmmModel. As in
    Kaldi's wrapper the means and diagonal precisions come from the diagonal UBM and only M comes from the extractor (its SigmaInv,
    prior offset and <w> are not used). The defaults are those of VB_resegmentation.sh as remembered (the script is not pinned
    here): max_speakers 10, max_iters 10, epsilon 1e-6, loop_prob 0.9, stat_scale 0.2, ll_scale 1.0, alpha_q_init 100.0, downsample
    25, sparsity_thr 0.001, min_dur 1; num_slots (at most 64 kept Gaussians per frame) is this implementation's. min_dur != 1 raises
    NotImplementedError. The rules are those of include/ktf_hip.h (ktf_vb_*) and INTEGRATION.md §2j."""

    def __init__(self, ie, dubm, max_speakers=10, max_iters=10, epsilon=1e-6, loop_prob=0.9, stat_scale=0.2, ll_scale=1.0,
                 alpha_q_init=100.0, downsample=25, sparsity_thr=0.001, num_slots=32, min_dur=1, workspace_limit=1 << 30):
        from . import io as kio
        if int(min_dur) != 1:
            raise NotImplementedError("VBResegmenter implements min_dur = 1 only")
        ie = ie if isinstance(ie, kio.KaldiIvecExtractorReader) else kio.KaldiIvecExtractorReader(ie, binary=True)
        ubm = dubm if isinstance(dubm, kio.KaldiDiagGmmReader) else kio.KaldiDiagGmmReader(dubm, binary=True)
        if ubm.numGauss != ie.numGauss or ubm.featDim != ie.featDim:
            raise ValueError(f"UBM ({ubm.numGauss} Gaussians, dim {ubm.featDim}) does not match the extractor "
                             f"({ie.numGauss} Gaussians, dim {ie.featDim})")
        I, D, R = ie.numGauss, ie.featDim, ie.ivecDim
        if not (1 <= I <= L.IVECTOR_MAX_GAUSS and 1 <= D <= L.IVECTOR_MAX_FEAT_DIM and 1 <= R <= L.IVECTOR_MAX_DIM):
            raise ValueError(f"model shape (I={I}, D={D}, R={R}) outside I <= {L.IVECTOR_MAX_GAUSS}, D <= {L.IVECTOR_MAX_FEAT_DIM}, "
                             f"R <= {L.IVECTOR_MAX_DIM}")
        if not 1 <= int(max_speakers) <= L.VB_MAX_SPEAKERS:
            raise ValueError(f"max_speakers {max_speakers} outside 1 .. {L.VB_MAX_SPEAKERS}")
        if not 1 <= int(num_slots) <= L.IVECTOR_MAX_GSELECT:
            raise ValueError(f"num_slots {num_slots} outside 1 .. {L.IVECTOR_MAX_GSELECT}")
        if int(downsample) < 1:
            raise ValueError(f"downsample {downsample} < 1")
        if int(max_iters) < 1:
            raise ValueError(f"max_iters {max_iters} < 1")
        if not 0.0 <= float(loop_prob) <= 1.0:
            raise ValueError(f"loop_prob {loop_prob} outside [0, 1]")
        if not 0.0 <= float(sparsity_thr) < 1.0:
            raise ValueError(f"sparsity_thr {sparsity_thr} outside [0, 1)")
        if not (float(stat_scale) > 0 and float(ll_scale) > 0 and float(alpha_q_init) > 0):
            raise ValueError("stat_scale, ll_scale and alpha_q_init must be > 0")
        self.numGauss, self.featDim, self.ivecDim = I, D, R
        self.maxSpeakers, self.maxIters, self.epsilon = int(max_speakers), int(max_iters), float(epsilon)
        self.loopProb, self.statScale, self.llScale = float(loop_prob), float(stat_scale), float(ll_scale)
        self.alphaQInit, self.downsample, self.sparsityThr = float(alpha_q_init), int(downsample), float(sparsity_thr)
        self.numSlots, self.workspaceLimit = int(num_slots), int(workspace_limit)
        iv = ubm.inv_vars.astype(np.float64)
        self._W = np.ascontiguousarray(np.concatenate([ubm.means_invvars.astype(np.float32).T,
                                                       (np.float32(-0.5) * ubm.inv_vars.astype(np.float32)).T]))
        self._gconst = np.ascontiguousarray(ubm.gconsts, dtype=np.float32)
        self._means = np.ascontiguousarray(ubm.means_invvars.astype(np.float64) / iv)
        M = np.asarray(ie.M, dtype=np.float64)                                  # (I, D, R)
        self._B = np.ascontiguousarray((iv[:, :, None] * M).reshape(I * D, R))
        r, c = np.tril_indices(R)
        self._U = np.zeros((I, R * (R + 1) // 2), dtype=np.float64)
        for i0 in range(0, I, 64):
            tmp = np.matmul(np.swapaxes(M[i0:i0 + 64], 1, 2), iv[i0:i0 + 64, :, None] * M[i0:i0 + 64])
            self._U[i0:i0 + 64] = tmp[:, r, c]

    def _consts(self, device):
        return per_device(self, device, lambda: tuple(torch.as_tensor(a, device=device)
                                                      for a in (self._W, self._gconst, self._means, self._B, self._U)))

    def posteriors(self, x):
        """Step 1 on packed frames x (F, D): -> (gauss, post, loglike, truncated (1,) device int32). The frames run in chunks whose
        workspace stays under workspace_limit; a frame's bits depend on its own row alone."""
        W, gc = self._consts(x.device)[:2]
        F = x.shape[0]
        trunc = torch.zeros((1,), dtype=torch.int32, device=x.device)
        step = max(1, self.workspaceLimit // max(1, ops.vb_post_workspace_bytes(1, self.numGauss)))
        if F <= step:
            return ops.vb_post(x, W, gc, self.numSlots, self.llScale, self.statScale, self.sparsityThr, trunc) + (trunc,)
        g = torch.empty((F, self.numSlots), dtype=torch.int32, device=x.device)
        p = torch.empty((F, self.numSlots), dtype=torch.float32, device=x.device)
        ll = torch.empty((F,), dtype=torch.float32, device=x.device)
        for lo, hi in chunks(F, step):
            g[lo:hi], p[lo:hi], ll[lo:hi] = ops.vb_post(x[lo:hi], W, gc, self.numSlots, self.llScale, self.statScale, self.sparsityThr,
                                                        trunc)
        return g, p, ll, trunc

    def _frames(self, feats, lengths, mask):
        from .layers import select_frames
        return select_frames(feats, self.featDim, lengths, mask)

    def __call__(self, feats, lengths=None, mask=None, init_labels=None, q0=None, sp0=None, seed=0):
        """feats (N, T, D) fp32 on a GPU; lengths / mask as IvectorExtractor takes them. Initialisation: init_labels (F,) ints over
        the selected frames (one-hot rows, a block takes the label of its first frame, a label outside [0, K) gives a uniform row),
        or q0 packed (sum T', K), or neither: rows of np.random.default_rng(seed).gamma(alpha_q_init, size=(sum T', K)) normalised.
        sp0 (K,) or (N, K), default uniform. -> VBResult."""
        x, off = self._frames(feats, lengths, mask)
        self._check_init(x, off, init_labels, q0, sp0)
        with L.on_device(x.device):
            g, p, ll, trunc = self.posteriors(x)
            return self._run(x, off, g, p, ll, trunc, init_labels, q0, sp0, seed)

    def from_posteriors(self, feats, gauss, post, loglike, lengths=None, mask=None, init_labels=None, q0=None, sp0=None, seed=0):
        """`__call__` on posteriors the caller supplies: gauss / post (F, n) and loglike (F) aligned with the selected frames."""
        x, off = self._frames(feats, lengths, mask)
        F = x.shape[0]
        if gauss.shape != post.shape or gauss.dim() != 2 or gauss.shape[0] != F or tuple(loglike.shape) != (F,):
            raise ValueError(f"gauss / post must both be ({F}, n) and loglike ({F},), got {tuple(gauss.shape)} / {tuple(post.shape)} / "
                             f"{tuple(loglike.shape)}")
        if not 1 <= gauss.shape[1] <= L.IVECTOR_MAX_GSELECT:
            raise ValueError(f"{gauss.shape[1]} slots per frame outside 1 .. {L.IVECTOR_MAX_GSELECT}")
        if any(t.device != x.device for t in (gauss, post, loglike)):
            raise ValueError("feats, gauss, post and loglike must be on one device")
        self._check_init(x, off, init_labels, q0, sp0)
        g = gauss.to(dtype=torch.int32).contiguous()
        p = post.to(dtype=torch.float32).contiguous()
        with L.on_device(x.device):
            return self._run(x, off, g, p, loglike.to(torch.float32).contiguous(), torch.zeros((1,), dtype=torch.int32, device=x.device), init_labels, q0,
                             sp0, seed)

    def _blocks(self, off):
        d = self.downsample
        T = np.diff(off)
        return np.concatenate([[0], np.cumsum((T + d - 1) // d)]).astype(np.int64)

    def _check_init(self, x, off, init_labels, q0, sp0):
        K, N, F = self.maxSpeakers, len(off) - 1, x.shape[0]
        TB = int(self._blocks(off)[-1])
        if init_labels is not None and q0 is not None:
            raise ValueError("pass init_labels or q0, not both")
        for t in (init_labels, q0, sp0):
            if isinstance(t, torch.Tensor) and t.is_cuda and t.device != x.device:
                raise ValueError("every input must be on the device of feats")
        if init_labels is not None and int(np.prod(np.shape(init_labels))) != F:
            raise ValueError(f"init_labels must hold {F} values, got shape {tuple(np.shape(init_labels))}")
        if q0 is not None:
            if tuple(q0.shape) != (TB, K):
                raise ValueError(f"q0 must be ({TB}, {K}), got {tuple(q0.shape)}")
            qh = host(q0, np.float64)
            if not np.isfinite(qh).all() or (qh < 0).any() or (qh > 1 + 1e-9).any():
                raise ValueError("q0 must hold probabilities")
        if sp0 is not None:
            sh = host(sp0, np.float64)
            if sh.shape not in ((K,), (N, K)) or not np.isfinite(sh).all() or (sh < 0).any() or (sh > 1 + 1e-9).any() or \
                    (np.abs(sh.sum(-1) - 1) > 1e-6).any():
                raise ValueError(f"sp0 must be ({K},) or ({N}, {K}) probabilities that sum to 1")

    def _init_q(self, off, boff, init_labels, q0, seed, device):
        K, d = self.maxSpeakers, self.downsample
        TB = int(boff[-1])
        if q0 is not None:
            return torch.as_tensor(host(q0, np.float64), device=device).contiguous()
        if init_labels is None:
            q = np.random.default_rng(seed).gamma(self.alphaQInit, size=(TB, K))
            return torch.as_tensor(q / q.sum(1, keepdims=True), device=device)
        lab = host(init_labels).reshape(-1).astype(np.int64)
        first = np.concatenate([off[r] + d * np.arange(boff[r + 1] - boff[r]) for r in range(len(off) - 1)] + [np.zeros(0, np.int64)])
        lb = lab[first.astype(np.int64)]
        q = np.full((TB, K), 1.0 / K)
        ok = (lb >= 0) & (lb < K)
        q[ok] = 0.0
        q[np.nonzero(ok)[0], lb[ok]] = 1.0
        return torch.as_tensor(q, device=device)

    def _run(self, x, off, g, p, ll, trunc, init_labels, q0, sp0, seed):
        dev = x.device
        K, N, d = self.maxSpeakers, len(off) - 1, self.downsample
        off = np.asarray(off, dtype=np.int64)
        boff = self._blocks(off)
        TB, F = int(boff[-1]), x.shape[0]
        _, _, means, Bm, U = self._consts(dev)
        q = self._init_q(off, boff, init_labels, q0, seed, dev)
        sh = np.full((N, K), 1.0 / K) if sp0 is None else host(sp0, np.float64)
        sp = torch.as_tensor(np.ascontiguousarray(np.broadcast_to(sh, (N, K))), device=dev)
        step = None
        if TB:
            o32 = torch.as_tensor(off.astype(np.int32), device=dev)
            b32 = torch.as_tensor(boff.astype(np.int32), device=dev)
            start, pairs = ops.vb_bucket(g, self.numGauss)
            gsum = ops.vb_loglike_sums(ll, o32)                 # sum_t G_t per recording, in an order of the recording's own

            def step(q, sp):
                Nst, Fst = ops.vb_speaker_stats(x, o32, b32, d, p, start, pairs, means, q)
                _, _, kl, h, gg = ops.vb_speaker_update(Nst, Fst, Bm, U)
                lls = ops.vb_block_loglike(x, o32, b32, d, TB, g, p, means, h, gg, K)
                qn, spn, tll = ops.vb_forward_backward(lls, b32, sp, self.loopProb)
                return qn, spn, ops.vb_bound(gsum, tll, kl, self.statScale)
        q, sp, bound, iters = _vb_iterate(step, q, sp, boff, self.maxIters, self.epsilon)
        block_of_frame = np.concatenate([boff[r] + np.arange(off[r + 1] - off[r]) // d for r in range(N)] + [np.zeros(0, np.int64)])
        fq = q[torch.as_tensor(block_of_frame.astype(np.int64), device=dev)] if F else torch.zeros((0, K), dtype=torch.float64, device=dev)
        labels = fq.argmax(1).to(torch.int32) if F else torch.zeros((0,), dtype=torch.int32, device=dev)
        return VBResult(q, fq, labels, sp, torch.as_tensor(bound, device=dev), iters, int(trunc.item()), off)


# =============================================================================== VBx
def vbx_init(init_labels, offsets, K, smoothing):
    """VBx's start from one integer label per window (host logic, no kernel): with the distinct labels of recording r in ascending
    order as columns 0 .. K_r - 1, gamma0 = softmax(smoothing * onehot) over those columns and 0 on the rest, pi0 = 1 / K_r on them.
    When K_r > K only the K clusters with the most windows are kept (ties to the lower label; columns still in ascending label
    order) and a window of a dropped cluster gets a row uniform over the kept columns. -> gamma0 (S, K), pi0 (N, K) fp64 arrays."""
    off = np.asarray(offsets, dtype=np.int64)
    lab = host(init_labels).reshape(-1)
    if lab.size and lab.dtype.kind not in "iu":
        raise ValueError(f"init_labels must be integers, got {lab.dtype}")
    if lab.size != off[-1]:
        raise ValueError(f"init_labels must hold {int(off[-1])} values, got {lab.size}")
    N = len(off) - 1
    gamma, pi = np.zeros((lab.size, K)), np.zeros((N, K))
    hot = np.exp(float(smoothing))
    for r in range(N):
        l = lab[off[r]:off[r + 1]].astype(np.int64)
        if l.size == 0:
            pi[r] = 1.0 / K                      # never read: the recording has no window
            continue
        ids, cnt = np.unique(l, return_counts=True)
        if ids.size > K:
            ids = np.sort(ids[np.lexsort((ids, -cnt))[:K]])
        Kr = ids.size
        col = np.searchsorted(ids, l)
        kept = (col < Kr) & (ids[np.minimum(col, Kr - 1)] == l)
        g = np.full((l.size, Kr), 1.0 / (hot + Kr - 1))
        g[np.nonzero(kept)[0], col[kept]] = hot / (hot + Kr - 1)
        g[~kept] = 1.0 / Kr
        gamma[off[r]:off[r + 1], :Kr] = g
        pi[r, :Kr] = 1.0 / Kr
    return gamma, pi


def vbx_labels(gamma, offsets):
    """labels (S,) int32 = arg-max of each row of gamma (S, K), ties to the lower index, renumbered per recording to 1 .. K'_r in
    ascending column order, and counts (N,) int32 = K'_r (0 for a recording without windows); torch, on gamma's device."""
    off = np.asarray(offsets, dtype=np.int64)
    N, (S, K) = len(off) - 1, gamma.shape
    dev = gamma.device
    if S == 0:
        return torch.zeros((0,), dtype=torch.int32, device=dev), torch.zeros((N,), dtype=torch.int32, device=dev)
    top = gamma.max(1, keepdim=True).values
    arg = (gamma == top).to(torch.int32).argmax(1)               # the first column that reaches the row's maximum
    rec = torch.as_tensor(np.repeat(np.arange(N), np.diff(off)), device=dev)
    used = torch.zeros((N, K), dtype=torch.int32, device=dev)
    used[rec, arg] = 1
    rank = torch.cumsum(used, 1)
    return rank[rec, arg].to(torch.int32), used.sum(1).to(torch.int32)


class VBxResult:
    """VBx's result: gamma (S, K) fp64 window posteriors, pi (N, K), elbo (N, max_iters) NaN-padded, labels (S,) int32 (arg-max of
    gamma, ties to the lower index, renumbered per recording to 1 .. K'_r in ascending column order) and counts (N,) int32 = K'_r (0
    for a recording without windows), all on the GPU; iters (N,) and offsets (N + 1) host int64 (recording r owns windows
    offsets[r] .. offsets[r + 1])."""

    def __init__(self, gamma, pi, elbo, iters, offsets, labels, counts):
        self.gamma, self.pi, self.elbo, self.iters, self.offsets, self.labels, self.counts = gamma, pi, elbo, iters, offsets, labels, counts


class VBx:
    """Extension: VBx (Landini, Diez, Burget, "Bayesian HMM clustering of x-vector sequences") on the GPU, batched over recordings:
    the VB-HMM of VBResegmenter over the window x-vectors themselves, the speaker model being a PLDA with within-class covariance I
    and between-class covariance diag(phi) in the transformed space. phi (D,) > 0; transform (D, Din) and offset (D,) take the input
    vectors there (y = transform x + offset, D <= Din; None: the vectors are used as they are). The usual start is AHC's labels
    (`diarize(..., vbx=...)`). The defaults are the BUT recipe's as remembered (the recipe is not pinned here): max_speakers 10,
    max_iters 40, epsilon 1e-6, loop_prob 0.99, Fa 0.3, Fb 17.0, init_smoothing 5.0. The rules are those of include/ktf_hip.h
    (ktf_vbx_*) and INTEGRATION.md §2k."""

    def __init__(self, phi, transform=None, offset=None, max_speakers=10, max_iters=40, epsilon=1e-6, loop_prob=0.99, Fa=0.3, Fb=17.0,
                 init_smoothing=5.0):
        phi = np.ascontiguousarray(host(phi), dtype=np.float64)
        if phi.ndim != 1 or not 1 <= phi.size <= L.VBX_MAX_DIM:
            raise ValueError(f"phi must be a vector of 1 .. {L.VBX_MAX_DIM} values, got shape {phi.shape}")
        if not np.isfinite(phi).all() or (phi <= 0).any():
            raise ValueError("phi must be positive and finite")
        D = phi.size
        if transform is None:
            if offset is not None:
                raise ValueError("offset needs a transform")
            self._A = self._b = None
            Din = D
        else:
            A = np.asarray(host(transform), dtype=np.float64)
            if A.ndim != 2 or A.shape[0] != D or not D <= A.shape[1] <= L.PLDA_DENSE_MAX_DIM or not np.isfinite(A).all():
                raise ValueError(f"transform must be a finite ({D}, Din) matrix with {D} <= Din <= {L.PLDA_DENSE_MAX_DIM}, got shape {A.shape}")
            Din = A.shape[1]
            b = np.zeros(D) if offset is None else np.asarray(host(offset), dtype=np.float64)
            if b.shape != (D,) or not np.isfinite(b).all():
                raise ValueError(f"offset must be a finite ({D},) vector, got shape {b.shape}")
            self._A = np.zeros((Din, Din))       # ktf_plda_f64 takes a square matrix: rows past D are zero and dropped afterwards
            self._A[:D] = A
            self._b = np.concatenate([b, np.zeros(Din - D)])
        if not is_int(max_speakers) or not 1 <= int(max_speakers) <= L.VB_MAX_SPEAKERS:
            raise ValueError(f"max_speakers {max_speakers!r} outside 1 .. {L.VB_MAX_SPEAKERS}")
        if not is_int(max_iters) or int(max_iters) < 1:
            raise ValueError(f"max_iters {max_iters!r} < 1")
        if not is_real(loop_prob) or not 0.0 <= float(loop_prob) <= 1.0:
            raise ValueError(f"loop_prob {loop_prob!r} outside [0, 1]")
        if not (is_real(Fa) and is_real(Fb) and 0 < float(Fa) < np.inf and 0 < float(Fb) < np.inf):
            raise ValueError(f"Fa and Fb must be > 0 and finite, got {Fa!r}, {Fb!r}")
        if not is_real(epsilon) or np.isnan(float(epsilon)):
            raise ValueError(f"epsilon must be a number, got {epsilon!r}")
        if not is_real(init_smoothing) or not 0.0 <= float(init_smoothing) <= 700.0:
            raise ValueError(f"init_smoothing {init_smoothing!r} outside [0, 700]")
        self.phi, self.dim, self.inputDim = phi, D, Din
        self.maxSpeakers, self.maxIters, self.epsilon = int(max_speakers), int(max_iters), float(epsilon)
        self.loopProb, self.Fa, self.Fb, self.initSmoothing = float(loop_prob), float(Fa), float(Fb), float(init_smoothing)

    @classmethod
    def from_plda(cls, plda, lda_dim=None, **kw):
        """The speaker model of a layers.PLDA: its transformMat and offset as the plain affine transform (no length normalisation,
        whatever the layer's flags say) and its psi as phi. lda_dim keeps the first lda_dim rows, the largest between-class
        variances when psi descends as Kaldi writes it; a psi that does not descend is refused when lda_dim truncates."""
        A = np.asarray(plda.transformMat, dtype=np.float64)
        b = np.asarray(plda.offset, dtype=np.float64)
        psi = np.asarray(plda.psi, dtype=np.float64)
        dim = psi.size
        if lda_dim is None:
            lda_dim = dim
        if not is_int(lda_dim) or not 1 <= int(lda_dim) <= dim:
            raise ValueError(f"lda_dim {lda_dim!r} outside 1 .. {dim}")
        lda_dim = int(lda_dim)
        if lda_dim < dim and (np.diff(psi) > 0).any():
            raise ValueError("psi does not descend: the first lda_dim rows would not be the largest between-class variances")
        return cls(psi[:lda_dim], A[:lda_dim], b[:lda_dim], **kw)

    def _consts(self, device):
        f = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=device)  # noqa: E731
        return per_device(self, device, lambda: (f(self.phi), f(self._A), f(self._b)))

    def transform(self, x):
        """x (S, Din) fp32 / fp64 on a GPU -> y (S, D) fp64 = transform x + offset (ktf_plda_f64 without length normalisation)."""
        _, A, b = self._consts(x.device)
        y = x.to(torch.float64).contiguous()
        if A is None or y.shape[0] == 0:
            return y[:, :self.dim].contiguous()
        y = ops.plda(y, A, b, b, False, False, want_scores=False)[1]
        return y if self.dim == self.inputDim else y[:, :self.dim].contiguous()

    def _start(self, off, init_labels, gamma0, pi0, seed):
        """-> gamma0 (S, K), pi0 (N, K) host fp64, checked."""
        K, N, S = self.maxSpeakers, len(off) - 1, int(off[-1])
        if init_labels is not None and gamma0 is not None:
            raise ValueError("pass init_labels or gamma0, not both")
        if init_labels is not None:
            if pi0 is not None:
                raise ValueError("init_labels set pi0 themselves")
            return vbx_init(init_labels, off, K, self.initSmoothing)
        if gamma0 is not None:
            g = np.array(host(gamma0), dtype=np.float64)
            if g.shape != (S, K):
                raise ValueError(f"gamma0 must be ({S}, {K}), got {g.shape}")
            if not np.isfinite(g).all() or (g < 0).any() or (g > 1 + 1e-9).any():
                raise ValueError("gamma0 must hold probabilities")
        else:
            g = np.random.default_rng(seed).gamma(1.0, size=(S, K))
            g /= g.sum(1, keepdims=True)
        if pi0 is None:
            p = np.full((N, K), 1.0 / K)
        else:
            p = np.array(host(pi0), dtype=np.float64)
            if p.shape not in ((K,), (N, K)) or not np.isfinite(p).all() or (p < 0).any() or (np.abs(p.sum(-1) - 1) > 1e-6).any():
                raise ValueError(f"pi0 must be ({K},) or ({N}, {K}) probabilities that sum to 1")
            p = np.array(np.broadcast_to(p, (N, K)))
        return g, p

    def __call__(self, x, lengths, init_labels=None, gamma0=None, pi0=None, seed=0):
        """x (S, Din) fp32 / fp64 on a GPU, the windows of all recordings end to end in time order; lengths: the N window counts.
        Start: init_labels (S,) ints (vbx_init's rule with K = max_speakers), or gamma0 packed (S, K) with pi0 (K,) or (N, K)
        (default uniform), or neither: rows of np.random.default_rng(seed).gamma(1.0, (S, K)) normalised and a uniform pi0. Every
        recording runs until its ELBO gains less than epsilon (that iteration's gamma and pi are kept) or max_iters; one device ->
        host read per iteration. -> VBxResult."""
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or not x.is_cuda or x.dtype not in (torch.float32, torch.float64):
            raise ValueError("x must be a (S, Din) float32 or float64 tensor on a GPU")
        if x.shape[1] != self.inputDim:
            raise ValueError(f"x has {x.shape[1]} columns, the model takes {self.inputDim}")
        lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, (torch.Tensor, np.ndarray)) else lengths)]
        if not 1 <= len(lens) <= 65535 or min(lens) < 0 or sum(lens) != x.shape[0]:
            raise ValueError(f"lengths must be 1 .. 65535 non-negative counts that sum to {x.shape[0]}, got {lens}")
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        g0, p0 = self._start(off, init_labels, gamma0, pi0, seed)
        with L.on_device(x.device):
            return self._run(x, off, g0, p0)

    def _run(self, x, off, g0, p0):
        dev = x.device
        N, S = len(off) - 1, int(off[-1])
        phi = self._consts(dev)[0]
        gamma = torch.as_tensor(g0, device=dev)
        pi = torch.as_tensor(p0, device=dev)
        step = None
        if S:
            o32 = torch.as_tensor(off.astype(np.int32), device=dev)
            rho, G = ops.vbx_prepare(self.transform(x), phi)
            zero = torch.zeros((N,), dtype=torch.float64, device=dev)

            def step(gamma, pi):
                alpha, _, c, kl = ops.vbx_speaker_update(gamma, rho, phi, self.Fa / self.Fb, o32)
                lls = ops.vbx_loglike(rho, G, alpha, c, self.Fa, o32)
                gn, pn, tll = ops.vb_forward_backward(lls, o32, pi, self.loopProb)
                return gn, pn, ops.vb_bound(zero, tll, kl * self.Fb, 0.0)
        gamma, pi, elbo, iters = _vb_iterate(step, gamma, pi, off, self.maxIters, self.epsilon)
        labels, counts = vbx_labels(gamma, off)
        return VBxResult(gamma, pi, torch.as_tensor(elbo, device=dev), iters, off, labels, counts)
