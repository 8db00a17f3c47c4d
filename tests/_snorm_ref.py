"""NumPy restatement of score normalisation against a cohort (what ktf_topn_stats_*, PLDA.cohort_stats and verification.as_norm
compute): per row the top_n largest scores by a full descending sort, their fp64 mean and centred population standard deviation;
and S-norm / Z-norm / T-norm of a trial list written out trial by trial."""

import numpy as np


def topn_stats(x, top_n=None):
    """x (R, C) -> (mean (R,), std (R,)) fp64 of the top_n largest entries of each row (None or >= C: the whole row). A sort keeps
    as many copies of the top_n-th largest value as fit, so the selected multiset does not depend on how ties are ordered."""
    x = np.asarray(x, np.float64)
    R, C = x.shape
    n = C if top_n is None else min(int(top_n), C)
    mean, std = np.empty(R), np.empty(R)
    for r in range(R):
        sel = np.sort(x[r])[::-1][:n]
        mean[r] = sel.sum() / n
        std[r] = np.sqrt(((sel - mean[r]) ** 2).sum() / n)
    return mean, std


def as_norm(scores, trials_enroll, trials_test, enroll_stats=None, test_stats=None):
    """The normalised score of every trial, in a loop: both sides 0.5 ((s - mu_e) / sd_e + (s - mu_t) / sd_t); one side alone is
    Z-norm (enroll) or T-norm (test), not halved."""
    out = np.empty(len(scores))
    for t, s in enumerate(np.asarray(scores, np.float64)):
        terms = []
        if enroll_stats is not None:
            e = int(trials_enroll[t])
            terms.append((s - enroll_stats[0][e]) / enroll_stats[1][e])
        if test_stats is not None:
            i = int(trials_test[t])
            terms.append((s - test_stats[0][i]) / test_stats[1][i])
        out[t] = terms[0] if len(terms) == 1 else 0.5 * (terms[0] + terms[1])
    return out
