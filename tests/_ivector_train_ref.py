"""fp64 NumPy oracle of i-vector extractor training (ivector-extractor-acc-stats / -sum-accs / -est / -init, no ivector-dependent
weights), written from the formulas with dense matrices: np.linalg.inv(Q) per utterance and explicit loops over utterances and
Gaussians. Built on _ivector_ref's posteriors, stats and derived. `marginal_objf` computes the log marginal likelihood per frame
independently of the accumulated scalars, from slogdet and solve."""

import numpy as np

import _ivector_ref as R


def eigh_desc(A):
    """As training.eigh_desc: descending, every eigenvector's largest-magnitude component positive."""
    w, V = np.linalg.eigh(0.5 * (A + A.T))
    w, V = w[::-1].copy(), V[:, ::-1].copy()
    for k in range(V.shape[1]):
        if V[np.argmax(np.abs(V[:, k])), k] < 0:
            V[:, k] = -V[:, k]
    return w, V


def utt_terms(x, gauss, post, M, sigma_inv, prior_offset, posterior_scale=1.0):
    """One utterance: gamma, F, lin (offset included), Q (dense), C = Q^-1, w = C lin, W = C + w w^T, the fp32 weights p'."""
    I, D, S = M.shape
    gamma, F = R.stats(x, gauss, post, I, posterior_scale=posterior_scale)
    lin = np.zeros(S)
    Q = np.eye(S)
    for i in range(I):
        lin += M[i].T @ sigma_inv[i] @ F[i]
        Q += gamma[i] * (M[i].T @ sigma_inv[i] @ M[i])
    lin[0] += prior_offset
    C = np.linalg.inv(Q)
    w = C @ lin
    return gamma, F, lin, Q, C, w, C + np.outer(w, w)


def accumulate(utts, M, sigma_inv, prior_offset, posterior_scale=1.0):
    """utts: a list of (x (T, D) fp32, gauss (T, n) int32, post (T, n)) -> the totals as a dict (R and the scatter dense)."""
    I, D, S = M.shape
    a = dict(gamma=np.zeros(I), Y=np.zeros((I, D, S)), R=np.zeros((I, S, S)), Ssec=np.zeros((I, D, D)), ivector_sum=np.zeros(S),
             ivector_scatter=np.zeros((S, S)), num_ivectors=0.0)
    for x, g, p in utts:
        if x.shape[0] == 0:
            continue
        gamma, F, lin, Q, C, w, W = utt_terms(x, g, p, M, sigma_inv, prior_offset, posterior_scale)
        a["gamma"] += gamma
        for i in range(I):
            a["Y"][i] += np.outer(F[i], w)
            a["R"][i] += gamma[i] * W
        a["ivector_sum"] += w
        a["ivector_scatter"] += W
        a["num_ivectors"] += 1
        pw = R.count_scale(p, posterior_scale=posterior_scale).astype(np.float64)
        xd = np.asarray(x, np.float64)
        for t in range(x.shape[0]):
            for s in range(g.shape[1]):
                if 0 <= g[t, s] < I:
                    a["Ssec"][g[t, s]] += pw[t, s] * np.outer(xd[t], xd[t])
    return a


def pack(A):
    """(..., S, S) symmetric -> (..., P) lower triangles row by row."""
    r, c = np.tril_indices(A.shape[-1])
    return A[..., r, c]


def marginal_objf(utts, M, sigma_inv, prior_offset, posterior_scale=1.0):
    """sum_u log int prod_t prod_i N(x_t; M_i w, Sigma_i)^p'_ti N(w; offset e0, I) dw / sum gamma: per utterance the Gaussian
    integral in closed form, log N-terms at w = 0 plus b^T Q^-1 b / 2 - log det Q / 2 - offset^2 / 2."""
    I, D, S = M.shape
    total, frames = 0.0, 0.0
    logdet = [np.linalg.slogdet(sigma_inv[i])[1] for i in range(I)]
    MtS = [M[i].T @ sigma_inv[i] for i in range(I)]
    MtSM = [MtS[i] @ M[i] for i in range(I)]
    for x, g, p in utts:
        if x.shape[0] == 0:
            continue
        pw = R.count_scale(p, posterior_scale=posterior_scale).astype(np.float64)
        xd = np.asarray(x, np.float64)
        Q = np.eye(S)
        b = np.zeros(S)
        b[0] = prior_offset
        const = 0.0
        for t in range(x.shape[0]):
            for s in range(g.shape[1]):
                i = g[t, s]
                if 0 <= i < I:
                    c = pw[t, s]
                    const += c * (0.5 * logdet[i] - 0.5 * D * np.log(2 * np.pi) - 0.5 * xd[t] @ sigma_inv[i] @ xd[t])
                    b += c * (MtS[i] @ xd[t])
                    Q += c * MtSM[i]
                    frames += c
        total += const + 0.5 * b @ np.linalg.solve(Q, b) - 0.5 * np.linalg.slogdet(Q)[1] - 0.5 * prior_offset ** 2
    return total / frames


def floored_inverse(Rm):
    """SolveQuadraticMatrixProblem's inverse with diagonal_precondition: (inverse, number of floored eigenvalues)."""
    d = np.diag(Rm).copy()
    d[~(d > 0)] = 1.0
    sc = 1.0 / np.sqrt(d)
    lam, P = np.linalg.eigh(Rm * np.outer(sc, sc))
    floor = max(1e-40, lam.max() / 1e4)
    nfl = int((lam < floor).sum())
    lam = np.maximum(lam, floor)
    return (P / lam) @ P.T * np.outer(sc, sc), nfl


def apply_floor(cov, floor):
    """SpMatrix::ApplyFloor(floor): floor = L L^T, the eigenvalues of L^-1 cov L^-T raised to at least 1, mapped back."""
    Lf = np.linalg.cholesky(floor)
    Li = np.linalg.inv(Lf)
    T = Li @ cov @ Li.T
    lam, P = np.linalg.eigh(0.5 * (T + T.T))
    return Lf @ (P * np.maximum(lam, 1.0)) @ P.T @ Lf.T


def prior_transform(m, cov, G=None):
    """V with V cov V^T = I and V m = |.| e0; with G (the weighted quadratic term) the rotation of rows 1... that makes
    (V^-T G V^-1)[1:, 1:] diagonal."""
    S = m.shape[0]
    s, P = np.linalg.eigh(0.5 * (cov + cov.T))
    T = np.diag(s ** -0.5) @ P.T
    x = T @ m
    x = x / np.linalg.norm(x)
    a = x - np.eye(S)[0]
    H = np.eye(S) if np.linalg.norm(a) == 0 else np.eye(S) - 2.0 * np.outer(a, a) / (a @ a)
    V = H @ T
    if G is not None:
        Vi = np.linalg.inv(V)
        _, E = eigh_desc((Vi.T @ G @ Vi)[1:, 1:])
        V = np.concatenate([V[:1], E.T @ V[1:]])
    return V


def update(M, sigma_inv, a, variance_floor_factor=0.1, gaussian_min_count=100.0, diagonalize=True, details=None, update_variances=True):
    """IvectorExtractorStats::Update from the totals of `accumulate` -> (M, sigma_inv, prior_offset). details: a dict that receives
    the intermediate quantities the tests look at."""
    I, D, S = M.shape
    M, sigma_inv = M.copy(), sigma_inv.copy()
    upd = [i for i in range(I) if a["gamma"][i] >= gaussian_min_count]
    floored = {}
    for i in upd:
        rinv, floored[i] = floored_inverse(a["R"][i])
        M[i] = M[i] + (a["Y"][i] - M[i] @ a["R"][i]) @ rinv
    if upd and update_variances:
        raw = {i: a["Ssec"][i] + M[i] @ a["R"][i] @ M[i].T - a["Y"][i] @ M[i].T - M[i] @ a["Y"][i].T for i in upd}
        floor = variance_floor_factor * sum(raw[i] for i in upd) / sum(a["gamma"][i] for i in upd)
        for i in upd:
            sigma_inv[i] = np.linalg.inv(apply_floor(0.5 * (raw[i] + raw[i].T) / a["gamma"][i], floor))
    n = a["num_ivectors"]
    m = a["ivector_sum"] / n
    cov = a["ivector_scatter"] / n - np.outer(m, m)
    G = None
    if diagonalize:
        G = sum(a["gamma"][i] * (M[i].T @ sigma_inv[i] @ M[i]) for i in range(I)) / a["gamma"].sum()
    V = prior_transform(m, cov, G)
    Vi = np.linalg.inv(V)
    if details is not None:
        details.update(V=V, m=m, cov=cov, floored=floored, M_before_prior=M.copy(), updated=upd)
    return np.stack([M[i] @ Vi for i in range(I)]), sigma_inv, float((V @ m)[0])


def init(means, inv_covars, S, seed=0):
    """ivector-extractor-init: (M, sigma_inv, prior_offset 100)."""
    I, D = means.shape
    M = np.random.default_rng(seed).standard_normal((I, D, S))
    M[:, :, 0] = means / 100.0
    return M, np.array(inv_covars, dtype=np.float64), 100.0


def sample(rng, M, sigma, prior_offset, n_utts, frames):
    """Data from the model itself with hard alignments: w ~ N(offset e0, I), Gaussian i uniform per frame, x ~ N(M_i w, Sigma_i).
    -> a list of (x fp32 (T, D), gauss (T, 1) int32, post (T, 1) = 1)."""
    I, D, S = M.shape
    chol = [np.linalg.cholesky(sigma[i]) for i in range(I)]
    utts = []
    for _ in range(n_utts):
        w = rng.standard_normal(S)
        w[0] += prior_offset
        g = rng.integers(0, I, frames)
        x = np.stack([M[i] @ w + chol[i] @ rng.standard_normal(D) for i in g]).astype(np.float32)
        utts.append((x, g.astype(np.int32)[:, None], np.ones((frames, 1))))
    return utts
