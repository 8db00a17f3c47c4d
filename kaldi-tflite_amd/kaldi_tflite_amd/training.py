"""Extension: PLDA back-end training, the estimators Kaldi's speaker recipes run on freshly extracted embeddings (INTEGRATION.md
§2g): `ivector-compute-lda` (compute_lda), `ivector-compute-plda` (compute_plda) and `est-pca --read-vectors=true` (est_pca).
The global mean (`ivector-mean` without spk2utt) is verification.speaker_means(x, [range(N)]).

Inputs follow ktf.verification: x (N, D) fp32 on the device (1 <= D <= 1024) and spk2utt as speaker_means takes it. Statistics whose
cost grows with N or S run on the GPU (csrc/plda_train.hip, fp64); the D x D factorisations run in fp64 NumPy on the host. Outputs
are host NumPy arrays (compute_plda: a ktf.layers.PLDA), ready for the ktf.io writers, XvectorExtractor.from_parts and PLDA.

Eigenvector signs: Kaldi's are arbitrary. Here every eigenvector's largest-magnitude component is positive (on a tie the lowest index
decides). A row's sign leaves PLDA scores and LDA'd, length-normalised scores unchanged."""

import numpy as np
import torch

from . import _lib as L
from . import ops
from .verification import _checked_map


# ----------------------------------------------------------------------------- host linear algebra (fp64)
def eigh_desc(A):
    """Symmetric eigendecomposition A = V diag(w) V^T, w descending; each column of V has its largest-magnitude component positive."""
    w, V = np.linalg.eigh(0.5 * (A + A.T))
    w, V = w[::-1].copy(), V[:, ::-1]
    k = np.argmax(np.abs(V), axis=0)
    return w, np.ascontiguousarray(V * np.where(V[k, np.arange(V.shape[1])] < 0, -1.0, 1.0))


def plda_diagonalize(phi_w, phi_b):
    """Phi_w = L L^T, L^-1 Phi_b L^-T = V diag(lam) V^T -> (P = V^T L^-1, Q = L V, lam): P Phi_w P^T = I, P Phi_b P^T = diag(lam)."""
    Lc = np.linalg.cholesky(0.5 * (phi_w + phi_w.T))
    Linv = np.linalg.inv(Lc)
    lam, V = eigh_desc(Linv @ phi_b @ Linv.T)
    return V.T @ Linv, Lc @ V, lam


# ----------------------------------------------------------------------------- inputs
def _rows(x):
    L.require_gpu()
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("x must be an (N, D) fp32 device tensor")
    N, D = x.shape
    if N < 1 or not 1 <= D <= L.TRAIN_MAX_DIM:
        raise ValueError(f"x: need N >= 1 rows and 1 <= D <= {L.TRAIN_MAX_DIM}, got {tuple(x.shape)}")
    return x.contiguous()


def _inputs(x, spk2utt, who):
    """-> (x, device offsets / utts int32, host counts, the listed rows (device int32)). ValueError before any launch."""
    x = _rows(x)
    off_d, utt_d, off_h = _checked_map(spk2utt, x.shape[0], x.device, "x", host_offsets=True)
    counts = np.diff(off_h).astype(np.int64)
    S, Nl = counts.size, int(counts.sum())
    if S < 1:
        raise ValueError("spk2utt: no speakers")
    if Nl <= S:
        raise ValueError(f"{who} needs more utterances than speakers ({Nl} <= {S}): no within-class data")
    return x, off_d, utt_d, counts, utt_d[int(off_h[0]):int(off_h[-1])]


def _host(*ts):
    return [t.cpu().numpy() for t in ts]


# ----------------------------------------------------------------------------- the estimators
def compute_lda(x, spk2utt, dim, total_covariance_factor=0.0, covariance_floor=1e-6):
    """Kaldi ivector-compute-lda --dim=dim: (dim, D + 1) fp32 [A | -A m], the transform.mat that XvectorExtractor.from_parts takes.
    m = the mean of ALL N rows; over the listed rows T = sum x' x'^T and B = sum_s n_s mu'_s mu'_s^T (x' = x - m), Sigma_tot = T / N_l,
    Sigma_w = (T - B) / N_l; C = f Sigma_tot + (1 - f) Sigma_w = U diag(s) U^T, s floored at covariance_floor * s_0,
    P = diag(s^-1/2) U^T; P Sigma_tot P^T = V diag(t) V^T; A = V[:, :dim]^T P. Needs 1 <= dim <= D and N_l > S."""
    x, off_d, utt_d, counts, listed = _inputs(x, spk2utt, "ivector-compute-lda")
    N, D = x.shape
    Nl = int(counts.sum())
    if not 1 <= int(dim) <= D:
        raise ValueError(f"dim must be in 1..{D}, got {dim}")
    f = float(total_covariance_factor)
    if not 0.0 <= f <= 1.0:
        raise ValueError(f"total_covariance_factor must be in [0, 1], got {f}")
    with L.launch_scope(x.device):
        ws = ops.train_workspace(max(N, Nl), D, x.device)
        m = ops.train_mean(x, ws)
        mu, _ = ops.train_class_means(x, off_d, utt_d, counts.size)
        n = torch.as_tensor(counts.astype(np.float64)).to(x.device)
        T = ops.train_gram(x, ws, idx=listed, center=m)
        B = ops.train_gram(mu, ws, center=m, weights=n)
        m, T, B = _host(m, T, B)
    tot = T / Nl
    within = (T - B) / Nl
    s, U = eigh_desc(f * tot + (1.0 - f) * within)
    if not s[0] > 0:
        raise ValueError("ivector-compute-lda: the covariance is zero")
    s = np.maximum(s, float(covariance_floor) * s[0])
    P = (U / np.sqrt(s)).T
    _, V = eigh_desc(P @ tot @ P.T)
    A = V[:, :int(dim)].T @ P
    return np.concatenate([A, -(A @ m)[:, None]], axis=1).astype(np.float32)


def compute_plda(x, spk2utt, num_em_iters=10):
    """Kaldi ivector-compute-plda (PldaStats, PldaEstimator; every class has weight 1) -> ktf.layers.PLDA with its defaults, whose
    .mean, .transformMat and .psi are the trained fp64 arrays. mean = the mean of the class means; O = the within-class scatter;
    from Phi_w = Phi_b = I, num_em_iters EM steps in the simultaneous diagonalisation of (Phi_w, Phi_b): one Cholesky and one
    eigendecomposition per step whatever the counts, M_n = Q diag(lam / (1 + n lam)) Q^T. Output: Phi_w = L L^T,
    L^-1 Phi_b L^-T = V diag(lam) V^T, transform = V^T L^-1, psi = max(lam, 0). Needs S >= 2 and N_l > S."""
    from .layers import PLDA
    x, off_d, utt_d, counts, listed = _inputs(x, spk2utt, "ivector-compute-plda")
    N, D = x.shape
    S, Nl = counts.size, int(counts.sum())
    if S < 2:
        raise ValueError("ivector-compute-plda needs at least two speakers")
    if int(num_em_iters) < 0:
        raise ValueError(f"num_em_iters must be >= 0, got {num_em_iters}")
    nh = counts.astype(np.float64)
    phi_w, phi_b = np.eye(D), np.eye(D)
    with L.launch_scope(x.device):
        ws = ops.train_workspace(Nl, D, x.device)
        mu, cnt = ops.train_class_means(x, off_d, utt_d, S)
        n = torch.as_tensor(nh).to(x.device)
        mbar = ops.train_mean(mu, ws)
        O, mbar_h = _host(ops.train_gram(x, ws, idx=listed, center=mbar) - ops.train_gram(mu, ws, center=mbar, weights=n), mbar)
        for _ in range(int(num_em_iters)):
            P, Q, lam = plda_diagonalize(phi_w, phi_b)
            a, b = ops.plda_em_project(mu, mbar, torch.as_tensor(P).to(x.device), torch.as_tensor(lam).to(x.device), cnt)
            SA, SB = _host(ops.train_gram(a, ws), ops.train_gram(b, ws, weights=n))
            nl = nh[:, None] * lam[None, :]
            SA[np.diag_indices(D)] += (lam[None, :] / (1.0 + nl)).sum(0)
            SB[np.diag_indices(D)] += (nl / (1.0 + nl)).sum(0)
            phi_b = Q @ SA @ Q.T / S
            phi_w = (O + Q @ SB @ Q.T) / Nl
    P, _, lam = plda_diagonalize(phi_w, phi_b)
    return PLDA(D, mbar_h, P, np.maximum(lam, 0.0))


def est_pca(x, dim=-1, normalize_mean=False, normalize_variance=False):
    """Kaldi est-pca --read-vectors=true: (dim, D) fp32, or (dim, D + 1) with normalize_mean. m = the mean of all rows,
    Cov = sum x x^T / N - m m^T = P diag(s) P^T; the transform is P^T, its row i scaled by 1 / sqrt(max(s_i, 1e-15)) with
    normalize_variance; normalize_mean appends the column -transform m; the first dim rows are kept (dim <= 0: all D)."""
    x = _rows(x)
    N, D = x.shape
    dim = D if int(dim) <= 0 else int(dim)
    if dim > D:
        raise ValueError(f"dim must be <= {D}, got {dim}")
    with L.launch_scope(x.device):
        ws = ops.train_workspace(N, D, x.device)
        m = ops.train_mean(x, ws)
        m, G = _host(m, ops.train_gram(x, ws, center=m))
    s, P = eigh_desc(G / N)
    t = P.T
    if normalize_variance:
        t = t / np.sqrt(np.maximum(s, 1e-15))[:, None]
    if normalize_mean:
        t = np.concatenate([t, -(t @ m)[:, None]], axis=1)
    return np.ascontiguousarray(t[:dim]).astype(np.float32)
