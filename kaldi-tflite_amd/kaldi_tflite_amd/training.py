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


# ----------------------------------------------------------------------------- i-vector extractor training
class IvectorStats:
    """Kaldi's IvectorExtractorStats (ivector-extractor-acc-stats, no ivector-dependent weights) as fp64 device accumulators, filled
    by IvectorExtractor.accumulate / accumulate_from_posteriors and read by ivector_extractor_est. `extractor`: the model the
    statistics are taken with (a path to final.ie, an io.KaldiIvecExtractorReader or io.IvecExtractorModel). The accumulators are
    allocated on the device of the first batch: gamma (I), Y (I * D, S), R (I, S(S+1)/2) packed lower triangles, ivector_sum (S),
    ivector_scatter (packed), totals (2) and, with update_variances, Ssec (I, D, D)."""

    def __init__(self, extractor, update_variances=True):
        from . import io as kio
        ie = extractor if isinstance(extractor, kio.KaldiIvecExtractorReader) else kio.KaldiIvecExtractorReader(extractor, binary=True)
        if ie.w is not None and ie.w.size:
            raise NotImplementedError("ivector-dependent weights (a non-empty <w>) are not supported")
        self.shape = (int(ie.numGauss), int(ie.featDim), int(ie.ivecDim))
        self.updateVariances = bool(update_variances)
        self._sigmaInv = np.asarray(ie.sigmaInv, dtype=np.float64)
        self._names = ("gamma", "Y", "R", "ivector_sum", "ivector_scatter", "totals") + (("Ssec",) if self.updateVariances else ())
        self.device = None

    def _alloc(self, device):
        if self.device is not None:
            if torch.device(device) != self.device:
                raise ValueError(f"IvectorStats lives on {self.device}, the batch on {device}")
            return
        I, D, S = self.shape
        P = S * (S + 1) // 2
        sizes = dict(gamma=(I,), Y=(I * D, S), R=(I, P), ivector_sum=(S,), ivector_scatter=(P,), totals=(2,), Ssec=(I, D, D))
        self.device = torch.device(device)
        for k in self._names:
            setattr(self, k, torch.zeros(sizes[k], dtype=torch.float64, device=self.device))

    def merge(self, other):
        """ivector-extractor-sum-accs: add another object's statistics (taken with the same model) to this one."""
        if other.shape != self.shape or other.updateVariances != self.updateVariances:
            raise ValueError(f"cannot merge statistics of shape {other.shape} into {self.shape}")
        if other.device is None:
            return self
        self._alloc(other.device)
        for k in self._names:
            getattr(self, k).add_(getattr(other, k))
        return self

    def host(self):
        """NumPy copies: gamma (I), Y (I, D, S), R (I, P) packed, Ssec (I, D, D) or None, ivector_sum (S), ivector_scatter (S, S)
        symmetric, num_ivectors, objf_sum (the sum of the utterances' scalars of ktf_ivector_acc_stats)."""
        I, D, S = self.shape
        P = S * (S + 1) // 2
        if self.device is None:
            z = np.zeros
            return dict(gamma=z(I), Y=z((I, D, S)), R=z((I, P)), Ssec=z((I, D, D)) if self.updateVariances else None, ivector_sum=z(S),
                        ivector_scatter=z((S, S)), num_ivectors=0.0, objf_sum=0.0)
        h = {k: getattr(self, k).cpu().numpy() for k in self._names}
        sc = np.zeros((S, S))
        r, c = np.tril_indices(S)
        sc[r, c] = h["ivector_scatter"]
        sc[c, r] = h["ivector_scatter"]
        return dict(gamma=h["gamma"], Y=h["Y"].reshape(I, D, S), R=h["R"], Ssec=h.get("Ssec"), ivector_sum=h["ivector_sum"],
                    ivector_scatter=sc, num_ivectors=float(h["totals"][0]), objf_sum=float(h["totals"][1]))

    def objf(self):
        """The exact log marginal likelihood per frame of the accumulated data under the model the statistics were taken with, at
        fixed alignments: [sum_u (lin_u^T w_u / 2 - log det Q_u / 2 - offset^2 / 2) + sum_i (gamma_i log det SigmaInv_i / 2 -
        tr(SigmaInv_i Ssec_i) / 2) - D log(2 pi) sum gamma / 2] / sum gamma. This is NOT the auxiliary function Kaldi logs: it is the
        quantity EM provably does not decrease. Needs update_variances=True (the second-order statistics)."""
        if not self.updateVariances:
            raise ValueError("objf needs the second-order statistics (update_variances=True)")
        h = self.host()
        tot = h["gamma"].sum()
        if not tot > 0:
            raise ValueError("objf: no statistics accumulated")
        D = self.shape[1]
        logdet = np.linalg.slogdet(self._sigmaInv)[1]
        tr = np.einsum("ide,ide->i", self._sigmaInv, h["Ssec"])
        return float((h["objf_sum"] + 0.5 * (h["gamma"] * logdet).sum() - 0.5 * tr.sum() - 0.5 * D * np.log(2 * np.pi) * tot) / tot)


def _unpack_sym(p, S):
    """(n, P) packed lower triangles -> (n, S, S) symmetric."""
    r, c = np.tril_indices(S)
    out = np.zeros((p.shape[0], S, S))
    out[:, r, c] = p
    out[:, c, r] = p
    return out


def ivector_extractor_est(extractor, stats, variance_floor_factor=0.1, gaussian_min_count=100.0, diagonalize=True):
    """Kaldi ivector-extractor-est (IvectorExtractorStats::Update, no weight update) -> io.IvecExtractorModel.
    Projections: for gamma_i >= gaussian_min_count, M_i += (Y_i - M_i R_i) R~_i^-1 with the diagonally preconditioned, eigenvalue-
    floored inverse (floor max(1e-40, lam_max / 1e4)) of SolveQuadraticMatrixProblem. Variances: raw_i = Ssec_i + M_i R_i M_i^T -
    Y_i M_i^T - M_i Y_i^T, floored (SpMatrix::ApplyFloor) at variance_floor_factor * sum raw / sum gamma. Prior: the whitening of
    the i-vector distribution, a Householder reflection onto e0 and, with diagonalize, the rotation that makes the weighted
    quadratic term diagonal on dimensions 1...; prior_offset = (V m)[0], M_i <- M_i V^-1.
    The per-Gaussian S x S and D x D factorisations run in fp64 NumPy on the host (np.linalg on stacks of 64 Gaussians); the
    returned model's `estInfo` = {"backend": "numpy-host", "seconds": wall time}."""
    import time
    from . import io as kio
    t_start = time.perf_counter()
    ie = extractor if isinstance(extractor, kio.KaldiIvecExtractorReader) else kio.KaldiIvecExtractorReader(extractor, binary=True)
    I, D, S = int(ie.numGauss), int(ie.featDim), int(ie.ivecDim)
    if stats.shape != (I, D, S):
        raise ValueError(f"statistics of shape {stats.shape} do not match the extractor {(I, D, S)}")
    h = stats.host()
    n = h["num_ivectors"]
    if not n >= 1:
        raise ValueError("ivector-extractor-est: no utterances accumulated")
    gamma, Y, Rp = h["gamma"], h["Y"], h["R"]
    M = np.array(ie.M, dtype=np.float64)
    sig_inv = np.array(ie.sigmaInv, dtype=np.float64)
    upd = np.nonzero(gamma >= float(gaussian_min_count))[0]
    raw = np.zeros((I, D, D))
    for lo in range(0, upd.size, 64):
        ix = upd[lo:lo + 64]
        R = _unpack_sym(Rp[ix], S)
        d = np.diagonal(R, axis1=1, axis2=2).copy()
        d[~(d > 0)] = 1.0                                   # an unseen direction: no preconditioning there
        sc = 1.0 / np.sqrt(d)
        lam, Pv = np.linalg.eigh(R * sc[:, :, None] * sc[:, None, :])
        floor = np.maximum(1e-40, lam.max(1) / 1e4)
        lam = np.maximum(lam, floor[:, None])
        rinv = np.matmul(Pv / lam[:, None, :], np.swapaxes(Pv, 1, 2)) * sc[:, :, None] * sc[:, None, :]
        M[ix] += np.matmul(Y[ix] - np.matmul(M[ix], R), rinv)
        if stats.updateVariances:
            YMt = np.matmul(Y[ix], np.swapaxes(M[ix], 1, 2))
            raw[ix] = h["Ssec"][ix] + np.matmul(np.matmul(M[ix], R), np.swapaxes(M[ix], 1, 2)) - YMt - np.swapaxes(YMt, 1, 2)
    if stats.updateVariances and upd.size:
        raw = 0.5 * (raw + np.swapaxes(raw, 1, 2))
        floor = float(variance_floor_factor) * raw[upd].sum(0) / gamma[upd].sum()
        try:
            Lf = np.linalg.cholesky(floor)
        except np.linalg.LinAlgError:
            raise ValueError("ivector-extractor-est: the variance floor is not positive definite") from None
        Li = np.linalg.inv(Lf)
        for lo in range(0, upd.size, 64):
            ix = upd[lo:lo + 64]
            T = np.matmul(np.matmul(Li, raw[ix] / gamma[ix, None, None]), Li.T)
            lam, Pv = np.linalg.eigh(0.5 * (T + np.swapaxes(T, 1, 2)))
            LP = np.matmul(Lf, Pv)
            cov = np.matmul(LP * np.maximum(lam, 1.0)[:, None, :], np.swapaxes(LP, 1, 2))
            inv = np.linalg.inv(cov)
            sig_inv[ix] = 0.5 * (inv + np.swapaxes(inv, 1, 2))
    # prior
    m = h["ivector_sum"] / n
    cov = h["ivector_scatter"] / n - np.outer(m, m)
    s, Pm = np.linalg.eigh(0.5 * (cov + cov.T))
    if not s[0] > 0:
        raise ValueError("ivector-extractor-est: the i-vector covariance is singular (too few utterances)")
    T = (Pm / np.sqrt(s)).T
    x = T @ m
    x /= np.linalg.norm(x)
    a = x.copy()
    a[0] -= 1.0
    na = np.linalg.norm(a)
    V = T if na == 0 else T - 2.0 * np.outer(a / na, (a / na) @ T)
    if diagonalize:
        G = np.zeros((S, S))
        for lo in range(0, I, 64):
            sl = slice(lo, lo + 64)
            G += np.einsum("i,ids,ide,iet->st", gamma[sl], M[sl], sig_inv[sl], M[sl], optimize=True)
        G /= gamma.sum()
        Vi = np.linalg.inv(V)
        _, E = eigh_desc((Vi.T @ G @ Vi)[1:, 1:])
        V = np.concatenate([V[:1], E.T @ V[1:]])
    Vi = np.linalg.inv(V)
    out = kio.IvecExtractorModel(np.matmul(M, Vi), sig_inv, float((V @ m)[0]), wVec=ie.wVec)
    out.estInfo = {"backend": "numpy-host", "seconds": time.perf_counter() - t_start}
    return out


def ivector_extractor_init(full_ubm, ivector_dim, seed=0):
    """Kaldi ivector-extractor-init --ivector-dim=ivector_dim (no ivector-dependent weights) from a full UBM (a path to final.ubm or
    an io.KaldiFullGmmReader) -> io.IvecExtractorModel: prior_offset 100, SigmaInv_i = the UBM's inverse covariances,
    M_i[:, 0] = mean_i / 100, the other columns standard normal from np.random.default_rng(seed), w empty, w_vec = log weights."""
    from . import io as kio
    full = full_ubm if isinstance(full_ubm, kio.KaldiFullGmmReader) else kio.KaldiFullGmmReader(full_ubm, binary=True)
    I, D, S = full.numGauss, full.featDim, int(ivector_dim)
    if not 1 <= S <= L.IVECTOR_MAX_DIM:
        raise ValueError(f"ivector_dim {ivector_dim} outside 1 .. {L.IVECTOR_MAX_DIM}")
    ic = full.inv_covars.astype(np.float64)
    mean = np.linalg.solve(ic, full.means_invcovars.astype(np.float64)[:, :, None])[:, :, 0]
    M = np.random.default_rng(seed).standard_normal((I, D, S))
    M[:, :, 0] = mean / 100.0
    with np.errstate(divide="ignore"):
        wvec = np.log(full.weights.astype(np.float64))
    return kio.IvecExtractorModel(M, ic, 100.0, wVec=wvec)


def train_ivector_extractor(layer_kwargs, full_ubm, batches, num_iters, ivector_dim=None, extractor=None, seed=0, **est_kwargs):
    """sid/train_ivector_extractor.sh as a loop: from `extractor` (default: ivector_extractor_init(full_ubm, ivector_dim, seed)),
    num_iters times: an IvectorExtractor(model, full_ubm=full_ubm, **layer_kwargs), one IvectorStats, layer.accumulate(stats, *b) for
    every b of `batches` (a list of argument tuples (feats[, lengths[, mask]]), walked once per iteration), then
    ivector_extractor_est(model, stats, **est_kwargs). -> (the final model, [objf of iteration 0, 1, ...]), each objf measured under
    the model the iteration started from."""
    from . import io as kio
    from .layers import IvectorExtractor
    full = full_ubm if isinstance(full_ubm, kio.KaldiFullGmmReader) else kio.KaldiFullGmmReader(full_ubm, binary=True)
    if extractor is None:
        if ivector_dim is None:
            raise ValueError("train_ivector_extractor needs ivector_dim or an initial extractor")
        extractor = ivector_extractor_init(full, ivector_dim, seed)
    model, objfs = extractor, []
    for _ in range(int(num_iters)):
        layer = IvectorExtractor(model, full_ubm=full, **dict(layer_kwargs))
        stats = IvectorStats(model)
        for b in batches:
            layer.accumulate(stats, *(b if isinstance(b, (tuple, list)) else (b,)))
        objfs.append(stats.objf())
        model = ivector_extractor_est(model, stats, **est_kwargs)
    return model, objfs
