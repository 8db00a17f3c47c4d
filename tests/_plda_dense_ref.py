"""fp64 NumPy restatement of Kaldi's `ivector-plda-scoring-dense` for one recording (conversation-dependent PCA, the PLDA
model projected into that subspace, every pair scored), with this project's edge rules ("Dense PLDA
scoring"). The test suites compare PLDA.score_dense against it; tests/golden/plda_dense.npz pins it to Kaldi."""

import numpy as np

RANK_FLOOR = {np.float64: 1e-10, np.float32: 1e-6}      # ktf_hip.h KTF_PLDA_DENSE_RANK_FLOOR_F64 / _F32


def kaldi_pca_dim(lam, target, off_by_one=True):
    """EstPca's loop (ivector-plda-scoring-dense.cc): d ends one past the count of eigenvalues whose energy exceeds the
    target. `off_by_one=False` is the loop without that quirk (it does not reproduce Kaldi's table)."""
    tot, e, d = float(np.sum(lam)), 0.0, 1
    while d - 1 < len(lam) and e / tot <= target:
        e += lam[d - 1]
        d += 1
    return d if off_by_one else d - 1


def pca(x, target, floor=1e-10, off_by_one=True):
    """-> (M (d, D) with the retained eigenvectors of the centred covariance as rows, d); d == 0: no PCA (rank 0)."""
    n, D = x.shape
    xc = x - x.mean(0)
    if n <= D:                                          # the n x n Gram problem, eigenvectors lifted to dimension D
        lam, v = np.linalg.eigh(xc @ xc.T / n)
        lam, v = lam[::-1], v[:, ::-1]
    else:
        lam, v = np.linalg.eigh(xc.T @ xc / n)
        lam, v = lam[::-1], v[:, ::-1]
    # numerical rank: eigenvalues above floor * lam[0]; none when lam[0] itself is below floor * the mean squared row norm
    # (tr(Sigma) + |m|^2): rows equal up to rounding
    big = lam[0] > floor * (np.sum(lam) + np.dot(x.mean(0), x.mean(0)))
    rank = int(np.sum(lam > floor * lam[0])) if big else 0
    if rank == 0:                                       # n = 1 or all rows equal: no PCA
        return None, 0
    d = min(kaldi_pca_dim(lam, target, off_by_one), rank)
    if n <= D:
        M = (xc.T @ v[:, :d] / np.sqrt(n * lam[:d])).T
    else:
        M = v[:, :d].T
    return M, d


def project_plda(M, mean, T, psi):
    """Plda::ApplyTransform(M) -> (T', offset', psi') of the model in the subspace."""
    Ti = np.linalg.inv(T)
    W, B = Ti @ Ti.T, Ti @ np.diag(psi) @ Ti.T
    mu, Wp, Bp = M @ mean, M @ W @ M.T, M @ B @ M.T
    Ci = np.linalg.inv(np.linalg.cholesky(Wp))
    s, U = np.linalg.eigh(Ci @ Bp @ Ci.T)
    s, U = np.maximum(s[::-1], 0.0), U[:, ::-1]
    Tp = U.T @ Ci
    return Tp, -Tp @ mu, s


def transform_score(y, T, offset, psi, normalize_length=True, simple_length_norm=False):
    """PLDA.call on rows y: transform (num_examples = 1), length norm in the model's dimension, LLR of every pair."""
    z = y @ T.T + offset
    dim = z.shape[1]
    if normalize_length:
        tot = np.sum(z * z, 1) if simple_length_norm else np.sum(z * z / (psi + 1.0), 1)
        z = z * np.sqrt(dim / tot)[:, None]
    k = psi / (psi + 1.0)
    v1, v2 = 1.0 + k, 1.0 + psi
    given = np.sum(np.log(v1)) + np.sum((z[:, None, :] - k * z[None, :, :]) ** 2 / v1, -1)
    without = np.sum(np.log(v2)) + np.sum(z * z / v2, -1)
    return -0.5 * given + 0.5 * without[:, None]


def score_dense(x, mean, T, psi, target=0.1, floor=1e-10, off_by_one=True, **norm):
    """One recording's rows x (n, D) -> (scores (n, n), d). target None (or rank 0): the model as it is."""
    x, mean, T, psi = (np.asarray(a, np.float64) for a in (x, mean, T, psi))
    M, d = (None, 0) if target is None else pca(x, target, floor, off_by_one)
    if d == 0:
        return transform_score(x, T, -T @ mean, psi, **norm), 0
    Tp, off, s = project_plda(M, mean, T, psi)
    return transform_score(x @ M.T, Tp, off, s, **norm), d
