"""fp64 NumPy restatement of Kaldi's verification scoring (what ktf.verification and the count-aware PLDA entry points compute):
ivector-mean over spk2utt, PLDA::TransformIvector(num_examples), PLDA::LogLikelihoodRatio(n), the recipe chain from raw
x-vectors to trial scores, compute-eer and sid/compute_min_dcf.py as the issue that asked for them specifies them (compute-eer with
the non-targets in ascending order: see verification.eer)."""

import numpy as np


def ivector_mean(raw, spk2utt):
    """(S, D) fp32 means: fp64 sums in list order, divided by the count, rounded once; and the counts (S,) int32."""
    raw = np.asarray(raw, np.float32)
    means = np.empty((len(spk2utt), raw.shape[1]), np.float32)
    for s, utts in enumerate(spk2utt):
        acc = np.zeros(raw.shape[1], np.float64)
        for u in utts:
            acc += raw[u].astype(np.float64)
        means[s] = (acc / len(utts)).astype(np.float32)
    return means, np.asarray([len(u) for u in spk2utt], np.int32)


def transform(x, mean, T, psi, n=1.0, normalize_length=True, simple_length_norm=False):
    """TransformIvector(num_examples = n) of rows x (B, dim): y = T (x - mean), scaled by sqrt(dim / sum y^2 / (psi + 1/n))."""
    x = np.asarray(x, np.float64)
    T, mean, psi = np.asarray(T, np.float64), np.asarray(mean, np.float64), np.asarray(psi, np.float64)
    y = (x - mean) @ T.T
    if not normalize_length:
        return y
    dim = y.shape[1]
    n = np.broadcast_to(np.asarray(n, np.float64), (y.shape[0],))[:, None]
    if simple_length_norm:
        return y * np.sqrt(dim) / np.linalg.norm(y, axis=1, keepdims=True)
    return y * np.sqrt(dim / np.sum(y * y / (psi + 1.0 / n), axis=1, keepdims=True))


def llr(test_tr, enroll_tr, psi, n=1.0):
    """LogLikelihoodRatio(enroll_j, n_j, test_i) -> (N, M): the class-conditional Gaussian of a class of n_j examples against the
    no-class Gaussian N(0, 1 + psi), per dimension."""
    y = np.asarray(test_tr, np.float64)[:, None, :]
    e = np.asarray(enroll_tr, np.float64)[None, :, :]
    psi = np.asarray(psi, np.float64)
    n = np.broadcast_to(np.asarray(n, np.float64), (e.shape[1],))[None, :, None]
    mean = n * psi / (n * psi + 1.0) * e
    var = 1.0 + psi / (n * psi + 1.0)
    given = -0.5 * np.sum(np.log(var) + (y - mean) ** 2 / var, axis=2)
    without = -0.5 * np.sum(np.log(1.0 + psi) + y[:, 0, :] ** 2 / (1.0 + psi), axis=1)
    return given - without[:, None]


def post(raw, global_mean, lda):
    """ivector-subtract-global-mean, transform-vec (lda (out, in + 1), last column the offset), ivector-normalize-length."""
    lda = np.asarray(lda, np.float64)
    z = (np.asarray(raw, np.float64) - np.asarray(global_mean, np.float64)) @ lda[:, :-1].T + lda[:, -1]
    return z * np.sqrt(z.shape[1]) / np.linalg.norm(z, axis=1, keepdims=True)


def chain(raw_enroll, spk2utt, test_xvectors, global_mean, lda, plda_mean, plda_T, psi, trials_model, trials_test):
    """The recipe from raw enrollment x-vectors and final test x-vectors to trial scores."""
    means, n = ivector_mean(raw_enroll, spk2utt)
    enroll = transform(post(means, global_mean, lda), plda_mean, plda_T, psi, n)
    test = transform(test_xvectors, plda_mean, plda_T, psi, 1.0)
    s = llr(test, enroll, psi, n)
    return s[np.asarray(trials_test), np.asarray(trials_model)]


def eer(scores, labels):
    tgt = sorted(float(s) for s, l in zip(scores, labels) if l)
    non = sorted(float(s) for s, l in zip(scores, labels) if not l)       # ascending: index nn - 1 - n has n non-targets above it
    nt, nn = len(tgt), len(non)
    t = 0
    for t in range(nt + 1):
        if t == nt:
            break
        pos = nn - 1 - int(nn * t / nt)
        pos = max(pos, 0)
        if non[pos] < tgt[t]:
            break
    return t / nt


def min_dcf(scores, labels, p_target, c_miss=1.0, c_fa=1.0):
    idx = sorted(range(len(scores)), key=lambda i: scores[i])          # Python's sort is stable
    lab = [1 if labels[i] else 0 for i in idx]
    fn, fp, fnrs, fprs = 0, 0, [], []
    for v in lab:
        fn += v
        fp += 1 - v
        fnrs.append(fn)
        fprs.append(fp)
    ntar = sum(lab)
    nnon = len(lab) - ntar
    best = min(c_miss * (a / ntar) * p_target + c_fa * (1 - b / nnon) * (1 - p_target) for a, b in zip(fnrs, fprs))
    return best / min(c_miss * p_target, c_fa * (1 - p_target))
