"""Extension: speaker verification the way Kaldi's recipes (sitw, sre16 v2, voxceleb) score it:
ivector-mean over spk2utt on the raw x-vectors, ivector-subtract-global-mean / transform-vec / ivector-normalize-length
(XvectorExtractor.postprocess), then ivector-plda-scoring --num-utts over a trial list (PLDA.transform with the counts,
PLDA.score_trials), optionally followed by score normalisation against a cohort (S-norm / adaptive S-norm: PLDA.cohort_stats,
as_norm, score_normalized). Host parsers for spk2utt and trials files, and the two figures every recipe ends
with (eer, min_dcf)."""

import numpy as np
import torch

from . import _lib as L
from . import ops


def _csr(spk2utt):
    """spk2utt -> (offsets (S + 1), utts) as host int64 arrays, or as device tensors when it is a CSR pair of device tensors."""
    if isinstance(spk2utt, tuple) and len(spk2utt) == 2 and all(isinstance(a, (np.ndarray, torch.Tensor)) for a in spk2utt):
        off, utt = spk2utt
        on_dev = [isinstance(a, torch.Tensor) and a.is_cuda for a in (off, utt)]
        if all(on_dev):
            return off, utt
        if any(on_dev):
            raise ValueError("spk2utt: offsets and utterance indices must both be on the host or both on the device")
        off = np.asarray(off.numpy() if isinstance(off, torch.Tensor) else off)
        utt = np.asarray(utt.numpy() if isinstance(utt, torch.Tensor) else utt)
    else:
        lists = [np.asarray(u).reshape(-1) if np.ndim(u) else np.asarray([u]) for u in spk2utt]
        off = np.cumsum([0] + [len(u) for u in lists])
        utt = np.concatenate(lists) if lists else np.zeros((0,), np.int64)
    if off.ndim != 1 or utt.ndim != 1 or (off.size and off.dtype.kind not in "iu") or (utt.size and utt.dtype.kind not in "iu"):
        raise ValueError("spk2utt: offsets and utterance indices must be 1-D integer sequences")
    return off.astype(np.int64), utt.astype(np.int64)


def _checked_map(spk2utt, U, device, what, host_offsets=False):
    """spk2utt -> (offsets (S + 1), utts) as device int32 tensors and, with host_offsets, the offsets as a host int64 array (else
    None). Every speaker needs at least one utterance and every index must lie in [0, U): checked on the host, or for a device map
    with one reduction and one read (which also brings the offsets back when asked for), before anything is launched."""
    off, utt = _csr(spk2utt)
    S = off.shape[0] - 1
    if S < 0:
        raise ValueError("spk2utt: offsets need S + 1 >= 1 entries")
    if isinstance(off, torch.Tensor):
        for a in (off, utt):
            if a.device != device:
                raise ValueError(f"spk2utt is on {a.device}, {what} on {device}")
            if a.dim() != 1 or a.dtype.is_floating_point or a.dtype == torch.bool:
                raise ValueError("spk2utt: offsets and utterance indices must be 1-D integer tensors")
        n = utt.shape[0]
        off_h = None
        if S:
            bad = ((off[1:] <= off[:-1]).any() | (off[0] < 0) | (off[-1] > n) | ((utt < 0) | (utt >= U)).any()).reshape(1)
            if host_offsets:
                back = torch.cat([bad.to(torch.int64), off.to(torch.int64)]).cpu().numpy()       # the one device -> host read
                bad, off_h = bool(back[0]), back[1:]
            else:
                bad = bool(bad.item())                                                           # the one device -> host read
            if bad:
                raise ValueError(f"spk2utt: a speaker without utterances, or an index outside 0..{U - 1}")
        off_d, utt_d = off.to(torch.int32).contiguous(), utt.to(torch.int32).contiguous()
    else:
        if S and (np.any(off[1:] <= off[:-1]) or off[0] < 0 or off[-1] > utt.size):
            raise ValueError("spk2utt: every speaker needs at least one utterance")
        if utt.size and (utt.min() < 0 or utt.max() >= U):
            raise ValueError(f"spk2utt: an utterance index outside 0..{U - 1}")
        off_h = off
        off_d = torch.as_tensor(off.astype(np.int32)).to(device)
        utt_d = torch.as_tensor(utt.astype(np.int32) if utt.size else np.zeros((1,), np.int32)).to(device)
    return off_d, utt_d, (off_h if host_offsets else None)


def speaker_means(raw, spk2utt):
    """Kaldi ivector-mean: raw x-vectors (U, D) fp32 on the device (XvectorExtractor.embeddings) and the speaker map spk2utt --
    a list of row-index lists (speaker s owns rows spk2utt[s]) or a CSR pair (offsets (S + 1), utts) of host arrays or device
    int tensors -> (means (S, D) fp32, num_utts (S,) int32), both on raw's device. A mean is the fp64 sum of its rows in list
    order, divided by the count and rounded once to fp32 (ktf_spk_mean_f32). Every speaker needs at least one utterance and every
    index must lie in [0, U): checked on the host, or for a device map with one reduction and one read, before the launch."""
    L.require_gpu()
    if not isinstance(raw, torch.Tensor) or not raw.is_cuda or raw.dim() != 2:
        raise ValueError("raw must be a (U, D) device tensor")
    x = raw.to(torch.float32).contiguous()
    off_d, utt_d, _ = _checked_map(spk2utt, x.shape[0], x.device, "raw")
    S = off_d.shape[0] - 1
    if S == 0:
        return (torch.empty((0, x.shape[1]), dtype=torch.float32, device=x.device),
                torch.empty((0,), dtype=torch.int32, device=x.device))
    with L.launch_scope(x.device):
        return ops.spk_mean(x, off_d, utt_d, S)


def _devices(*objs):
    devs = set()
    for o in objs:
        if isinstance(o, torch.Tensor) and o.is_cuda:
            devs.add(o.device)
        elif isinstance(o, (list, tuple)):
            devs |= _devices(*o)
    return devs


def _stats(stats, what, device):
    """(mean, std) of as_norm as two 1-D float64 tensors of one length on `device`."""
    if not (isinstance(stats, (tuple, list)) and len(stats) == 2):
        raise ValueError(f"{what} must be a pair (mean, std)")
    out = []
    for a in stats:
        t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))
        if t.device != device:
            raise ValueError(f"{what} on {t.device}, the scores on {device}")
        if t.dim() != 1 or not t.dtype.is_floating_point:
            raise ValueError(f"{what} must hold 1-D floating-point tensors, got {t.dtype} {tuple(t.shape)}")
        out.append(t.to(torch.float64))
    if out[0].shape != out[1].shape:
        raise ValueError(f"{what}: {out[0].shape[0]} means, {out[1].shape[0]} standard deviations")
    return out


def _indices(a, what, device):
    """Trial indices as a 1-D int64 tensor on `device` (the checks of PLDA._trial_pairs; the range is checked by the caller)."""
    if isinstance(a, torch.Tensor):
        if a.device != device:
            raise ValueError(f"{what} on {a.device}, the scores on {device}")
        if a.dim() != 1 or a.dtype.is_floating_point or a.dtype == torch.bool or a.is_complex():
            raise ValueError(f"{what} must be a 1-D integer tensor, got {a.dtype} {tuple(a.shape)}")
        return a.to(torch.int64)
    a = np.asarray(a)
    if a.size == 0:
        a = a.reshape(0).astype(np.int64)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be a 1-D sequence of integers, got {a.dtype} {a.shape}")
    return torch.as_tensor(a.astype(np.int64)).to(device)


def as_norm(scores, trials_enroll, trials_test, enroll_stats=None, test_stats=None):
    """Symmetric score normalisation of trial scores with cohort statistics (PLDA.cohort_stats): for trial t of model
    e = trials_enroll[t] and test i = trials_test[t],
        0.5 * ((s_t - mu_e) / sigma_e + (s_t - mu_i) / sigma_i)
    with enroll_stats = (mu, sigma) per model (role "enroll") and test_stats = (mu, sigma) per test (role "test"). Only
    enroll_stats: Z-norm, (s - mu_e) / sigma_e; only test_stats: T-norm, (s - mu_i) / sigma_i (neither is halved); giving neither
    raises. scores (T,) in any float dtype -> (T,) float64, computed by torch indexing on the device the inputs are on (host
    tensors included). Indices are host sequences or integer tensors on that device, checked in range (for a device tensor with
    one reduction and one read). A sigma of 0 (an all-tied selection: a cohort of one vector, or equal scores) is not special-cased:
    the division gives IEEE inf, or nan where the score equals the mean."""
    if enroll_stats is None and test_stats is None:
        raise ValueError("as_norm needs enroll_stats (Z-norm), test_stats (T-norm) or both (S-norm)")
    s = scores if isinstance(scores, torch.Tensor) else torch.as_tensor(np.asarray(scores, dtype=np.float64))
    if s.dim() != 1 or not s.dtype.is_floating_point:
        raise ValueError(f"scores must be a 1-D floating-point tensor, got {s.dtype} {tuple(s.shape)}")
    s = s.to(torch.float64)
    je = _indices(trials_enroll, "trials_enroll", s.device)
    it = _indices(trials_test, "trials_test", s.device)
    if je.shape[0] != s.shape[0] or it.shape[0] != s.shape[0]:
        raise ValueError(f"{s.shape[0]} scores, {je.shape[0]} enrollment indices, {it.shape[0]} test indices")
    terms = []
    for stats, idx, what in ((enroll_stats, je, "enroll_stats"), (test_stats, it, "test_stats")):
        if stats is None:
            continue
        mu, sigma = _stats(stats, what, s.device)
        if idx.shape[0] and bool(((idx < 0) | (idx >= mu.shape[0])).any()):
            raise ValueError(f"a trial index is outside the {mu.shape[0]} entries of {what}")
        terms.append((s - mu[idx]) / sigma[idx])
    return terms[0] if len(terms) == 1 else 0.5 * (terms[0] + terms[1])


def score_normalized(plda, enroll_tr, test_tr, trials, cohort, top_n=None, enroll_num_examples=None, cohort_num_examples=None,
                     sides="both", workspace_limit=1 << 30):
    """Trial scores with S-norm (top_n None) or adaptive S-norm (the top_n best cohort scores per side) -> (normalised (T,)
    float64, raw (T,) in the PLDA's dtype: plda.score_trials' scores). enroll_tr / test_tr: TRANSFORMED models (with
    enroll_num_examples, as for score_trials) and tests; trials: a pair (model indices, test indices); cohort: (C, dim)
    post-processed cohort vectors as ext(...) or ext.postprocess(means) return them, NOT yet transformed by the PLDA: the enroll
    side scores them as tests (plain transform), the test side as classes of cohort_num_examples examples each (None: 1; transform
    with the counts). Statistics are computed only for the models and tests that occur in `trials` (PLDA.cohort_stats, at most
    workspace_limit bytes of scores at a time). sides: "both" (S-norm), "enroll" (Z-norm) or "test" (T-norm)."""
    if sides not in ("both", "enroll", "test"):
        raise ValueError(f"sides must be 'both', 'enroll' or 'test', got {sides!r}")
    if not (isinstance(trials, (list, tuple)) and len(trials) == 2):
        raise ValueError("trials must be a pair (model indices, test indices)")
    if not isinstance(cohort, torch.Tensor) or not cohort.is_cuda:
        raise ValueError("cohort must be a (C, dim) device tensor of post-processed vectors")
    coh = cohort.reshape(-1, cohort.shape[-1])
    if coh.shape[1] != plda.dim or coh.shape[0] < 1:
        raise ValueError(f"cohort must be (C >= 1, {plda.dim}), got {tuple(cohort.shape)}")
    t, e = plda._scoring_inputs(test_tr, enroll_tr)
    if coh.device != t.device:
        raise ValueError(f"the cohort on {coh.device}, the vectors on {t.device}")
    pairs = plda._trial_pairs(trials[0], trials[1], e.shape[0], t.shape[0], t.device).to(torch.int64)
    enroll_stats = test_stats = None
    je, it = pairs[:, 0], pairs[:, 1]
    if sides in ("both", "enroll"):
        models, je = torch.unique(pairs[:, 0], return_inverse=True)
        n = None
        if enroll_num_examples is not None:
            n = plda._counts(enroll_num_examples, e.shape[0], t.device, "enroll_num_examples")[models]
        enroll_stats = plda.cohort_stats(e[models], plda.transform(coh), top_n=top_n, role="enroll", num_examples=n,
                                         workspace_limit=workspace_limit)
    if sides in ("both", "test"):
        tests, it = torch.unique(pairs[:, 1], return_inverse=True)
        test_stats = plda.cohort_stats(t[tests], plda.transform(coh, num_examples=cohort_num_examples), top_n=top_n, role="test",
                                       num_examples=cohort_num_examples, workspace_limit=workspace_limit)
    raw = plda.score_trials(t, e, trials[0], trials[1], enroll_num_examples=enroll_num_examples)
    return as_norm(raw, je, it, enroll_stats=enroll_stats, test_stats=test_stats), raw


def score(ext, plda, enroll_wavs, spk2utt, test_wavs, trials, cohort=None, top_n=None, cohort_num_examples=None):
    """Kaldi's verification scoring chain, wav to trial scores. Enrollment: ext.embeddings(enroll_wavs) -> speaker_means(spk2utt)
    -> ext.postprocess -> plda.transform(num_examples=num_utts). Test: ext(test_wavs) -> plda.transform. Then
    plda.score_trials with the counts. trials: a pair (model indices into the speakers of spk2utt, test indices into the rows of
    test_wavs) -> (T,) scores in the PLDA's dtype. Inputs spread over several devices are refused before anything is launched.
    cohort (C, dim) post-processed cohort vectors: the scores are normalised against it (score_normalized with top_n and
    cohort_num_examples; S-norm on both sides) -> (T,) float64. Without a cohort nothing changes."""
    if not (isinstance(trials, (list, tuple)) and len(trials) == 2):
        raise ValueError("trials must be a pair (model indices, test indices)")
    devs = _devices(enroll_wavs, test_wavs, trials, cohort, spk2utt if isinstance(spk2utt, tuple) else ())
    if len(devs) > 1:
        raise ValueError(f"the inputs must all be on one GPU (or on the host), got {sorted(str(d) for d in devs)}")
    raw = ext.embeddings(enroll_wavs)
    means, num_utts = speaker_means(raw, spk2utt)
    enroll_tr = plda.transform(ext.postprocess(means), num_examples=num_utts)
    tv = ext(test_wavs)
    test_tr = plda.transform(tv.reshape(-1, tv.shape[-1]))
    if cohort is not None:
        return score_normalized(plda, enroll_tr, test_tr, trials, cohort, top_n=top_n, enroll_num_examples=num_utts,
                                cohort_num_examples=cohort_num_examples)[0]
    return plda.score_trials(test_tr, enroll_tr, trials[0], trials[1], enroll_num_examples=num_utts)


# ----------------------------------------------------------------------------- Kaldi text formats (host)
def read_spk2utt(path):
    """Kaldi spk2utt: one `speaker utt1 utt2 ...` per line -> a list of (speaker, [utterance ids]) in file order."""
    out = []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) < 2:
                raise ValueError(f"{path}:{n}: a speaker without utterances")
            out.append((parts[0], parts[1:]))
    return out


def read_trials(path):
    """Kaldi trials: one `model test [target|nontarget]` per line -> (models, tests, labels): two lists of ids and a bool array
    (True = target), or None when no line has a label (every line must then have none)."""
    models, tests, labels = [], [], []
    with open(path) as f:
        for n, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) not in (2, 3) or (len(parts) == 3 and parts[2] not in ("target", "nontarget")):
                raise ValueError(f"{path}:{n}: expected `model test [target|nontarget]`, got {line.strip()!r}")
            models.append(parts[0])
            tests.append(parts[1])
            labels.append(parts[2] == "target" if len(parts) == 3 else None)
    have = {lab is not None for lab in labels}
    if len(have) > 1:
        raise ValueError(f"{path}: some trials have a label and some do not")
    return models, tests, (np.asarray(labels, dtype=bool) if have == {True} else None)


# ----------------------------------------------------------------------------- evaluation (host NumPy)
def _scores_labels(scores, labels):
    s = np.asarray(scores.detach().cpu().numpy() if isinstance(scores, torch.Tensor) else scores, dtype=np.float64).reshape(-1)
    lab = np.asarray(labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else labels).reshape(-1).astype(bool)
    if s.shape != lab.shape:
        raise ValueError(f"{s.size} scores, {lab.size} labels")
    if lab.all() or not lab.any():
        raise ValueError("eer / min_dcf need at least one target and one non-target trial")
    return s, lab


def eer(scores, labels):
    """Equal error rate, restating Kaldi's compute-eer. No Kaldi source was at hand: the rule below, from the issue that asked for
    it, is the specification, with one correction. Target scores sorted ascending; for target position t (t targets would be
    missed at threshold target[t]) take n = floor(N_nt * t / N_t) and the non-target that has n non-targets above it, index
    N_nt - 1 - n of the non-target scores sorted ASCENDING (clamped at 0); the first t at which that non-target scores below
    target[t] -- at most n / N_nt false alarms against t / N_t misses -- gives EER = t / N_t (1 when there is none). The issue
    sorts the non-targets descending with the same index, which picks the n-th LOWEST non-target and gives 1.0 for lists whose
    error rates cross at 0.5 (targets 1, 3, non-targets 2, 4); DESIGN.md §7 keeps the example. Ties count as errors (the test is
    strict). A list without targets or without non-targets raises ValueError."""
    s, lab = _scores_labels(scores, labels)
    tgt = np.sort(s[lab])
    non = np.sort(s[~lab])
    nt, nn = tgt.size, non.size
    t = 0
    while t < nt:
        pos = max(nn - 1 - (nn * t) // nt, 0)
        if non[pos] < tgt[t]:
            break
        t += 1
    return t / nt


def min_dcf(scores, labels, p_target, c_miss=1.0, c_fa=1.0):
    """Minimum normalised detection cost, restating sid/compute_min_dcf.py: the trials sorted stably by score (tied scores keep
    their list order); at every position i the miss rate (targets at or below it / targets) and false-alarm rate (1 - non-targets
    at or below it / non-targets); min over i of c_miss * P_miss * p + c_fa * P_fa * (1 - p), divided by
    min(c_miss * p, c_fa * (1 - p)). A list without targets or without non-targets raises ValueError (the script divides by zero)."""
    s, lab = _scores_labels(scores, labels)
    if not 0.0 < float(p_target) < 1.0:
        raise ValueError(f"p_target must be in (0, 1), got {p_target}")
    order = np.argsort(s, kind="stable")
    y = lab[order].astype(np.float64)
    fnr = np.cumsum(y) / y.sum()
    fpr = 1.0 - np.cumsum(1.0 - y) / (y.size - y.sum())
    c_det = c_miss * fnr * p_target + c_fa * fpr * (1.0 - p_target)
    return float(c_det.min() / min(c_miss * p_target, c_fa * (1.0 - p_target)))
