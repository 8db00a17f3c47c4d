"""fp64 NumPy restatement of Kaldi's back-end estimators as INTEGRATION.md §2g specifies them: ivector-compute-lda,
ivector-compute-plda (PldaStats / PldaEstimator, literally: one D x D inverse per distinct count, classes taken in order of their
count, the output through a Cholesky inverse) and est-pca --read-vectors=true. np.linalg.eigh, eigenvector signs as in
kaldi_tflite_amd.training (largest-magnitude component positive, the lowest index on a tie). The oracle of the GPU tests."""

import numpy as np


def eigh_desc(A):
    w, V = np.linalg.eigh(0.5 * (A + A.T))
    w, V = w[::-1].copy(), V[:, ::-1]
    k = np.argmax(np.abs(V), axis=0)
    return w, V * np.where(V[k, np.arange(V.shape[1])] < 0, -1.0, 1.0)


def _lists(spk2utt):
    return [np.asarray(u, dtype=np.int64).reshape(-1) for u in spk2utt]


def lda_scatter(x, spk2utt):
    """(m, Sigma_tot, Sigma_w) of ivector-compute-lda: m over all rows, the two covariances over the listed rows."""
    x = np.asarray(x, np.float64)
    m = x.sum(0) / x.shape[0]
    xp = x - m
    lists = _lists(spk2utt)
    T = np.zeros((x.shape[1],) * 2)
    B = np.zeros_like(T)
    for u in lists:
        T += xp[u].T @ xp[u]
        mu = xp[u].mean(0)
        B += len(u) * np.outer(mu, mu)
    Nl = sum(len(u) for u in lists)
    return m, T / Nl, (T - B) / Nl


def compute_lda(x, spk2utt, dim, total_covariance_factor=0.0, covariance_floor=1e-6):
    m, tot, within = lda_scatter(x, spk2utt)
    f = total_covariance_factor
    s, U = eigh_desc(f * tot + (1 - f) * within)
    s = np.maximum(s, covariance_floor * s[0])
    P = np.diag(s ** -0.5) @ U.T
    _, V = eigh_desc(P @ tot @ P.T)
    A = V[:, :dim].T @ P
    return np.concatenate([A, -(A @ m)[:, None]], axis=1)


def plda_stats(x, spk2utt):
    """(class means (S, D), counts (S,), mean of the class means, O = sum_s (sum_u x x^T - n mu mu^T))."""
    x = np.asarray(x, np.float64)
    lists = _lists(spk2utt)
    mus = np.stack([x[u].mean(0) for u in lists])
    n = np.array([len(u) for u in lists], np.float64)
    O = np.zeros((x.shape[1],) * 2)
    for u, mu in zip(lists, mus):
        O += x[u].T @ x[u] - len(u) * np.outer(mu, mu)
    return mus, n, mus.mean(0), O


def em_step(stats, phi_w, phi_b):
    """One PldaEstimator iteration, Kaldi's form: classes grouped by count, M_n = (Phi_b^-1 + n Phi_w^-1)^-1 per distinct n."""
    mus, n, mbar, O = stats
    S, D = mus.shape
    Wi, Bi = np.linalg.inv(phi_w), np.linalg.inv(phi_b)
    Sb, Sw = np.zeros((D, D)), O.copy()
    for c in np.unique(n):                                  # ascending count
        sel = n == c
        M = np.linalg.inv(Bi + c * Wi)
        m = mus[sel] - mbar
        w = (c * m @ Wi) @ M                                # rows w_s = M (n Phi_w^-1 m_s) (M, Wi symmetric)
        d = m - w
        k = int(sel.sum())
        Sb += k * M + w.T @ w
        Sw += c * (k * M + d.T @ d)
    return Sw / n.sum(), Sb / S


def compute_plda(x, spk2utt, num_em_iters=10, history=None):
    """-> (mean, transform, psi), Kaldi's PLDA; history: a list that receives (Phi_w, Phi_b) after every iteration."""
    stats = plda_stats(x, spk2utt)
    D = stats[0].shape[1]
    phi_w, phi_b = np.eye(D), np.eye(D)
    for _ in range(num_em_iters):
        phi_w, phi_b = em_step(stats, phi_w, phi_b)
        if history is not None:
            history.append((phi_w, phi_b))
    return plda_output(stats[2], phi_w, phi_b)


def plda_output(mean, phi_w, phi_b):
    Lc = np.linalg.cholesky(phi_w)
    Linv = np.linalg.inv(Lc)
    lam, V = eigh_desc(Linv @ phi_b @ Linv.T)
    return mean, V.T @ Linv, np.maximum(lam, 0.0)


def plda_log_likelihood(x, spk2utt, mean, phi_w, phi_b):
    """Marginal log-likelihood of the listed rows under x = mean + y_s + e, y_s ~ N(0, Phi_b), e ~ N(0, Phi_w), per class jointly."""
    x = np.asarray(x, np.float64)
    Lc = np.linalg.cholesky(phi_w)
    Linv = np.linalg.inv(Lc)
    lam, V = eigh_desc(Linv @ phi_b @ Linv.T)
    P = V.T @ Linv
    logdet_p = -np.log(np.diag(Lc)).sum()
    total = 0.0
    for u in _lists(spk2utt):
        z = (x[u] - mean) @ P.T
        k = len(u)
        sz = z.sum(0)
        q = (z * z).sum(0) - lam * sz * sz / (1 + k * lam)
        total += -0.5 * (k * len(lam) * np.log(2 * np.pi) + np.log1p(k * lam).sum() + q.sum()) + k * logdet_p
    return total


def est_pca(x, dim=-1, normalize_mean=False, normalize_variance=False):
    x = np.asarray(x, np.float64)
    N, D = x.shape
    m = x.sum(0) / N
    s, P = eigh_desc(x.T @ x / N - np.outer(m, m))
    t = P.T
    if normalize_variance:
        t = t / np.sqrt(np.maximum(s, 1e-15))[:, None]
    if normalize_mean:
        t = np.concatenate([t, -(t @ m)[:, None]], axis=1)
    return t[:(D if dim <= 0 else dim)]


def sample_plda(rng, D, S, lo, hi, phi_w, phi_b, mean):
    """Rows of the PLDA generative model: speaker s has n_s ~ U{lo..hi} rows mean + y_s + e. -> (x (N, D), spk2utt lists)."""
    n = rng.integers(lo, hi + 1, S)
    cb, cw = np.linalg.cholesky(phi_b), np.linalg.cholesky(phi_w)
    y = rng.standard_normal((S, D)) @ cb.T
    x = mean + np.repeat(y, n, axis=0) + rng.standard_normal((int(n.sum()), D)) @ cw.T
    off = np.concatenate([[0], np.cumsum(n)])
    return x, [list(range(off[s], off[s + 1])) for s in range(S)]
