"""Extension: PLDA back-end training, the estimators Kaldi's speaker recipes run on freshly extracted embeddings (INTEGRATION.md
§2g): `ivector-compute-lda` (compute_lda), `ivector-compute-plda` (compute_plda) and `est-pca --read-vectors=true` (est_pca).
The global mean (`ivector-mean` without spk2utt) is verification.speaker_means(x, [range(N)]).

Inputs follow ktf.verification: x (N, D) fp32 on the device (1 <= D <= 1024) and spk2utt as speaker_means takes it. Statistics whose
cost grows with N or S run on the GPU (csrc/plda_train.hip, fp64); the D x D factorisations run in fp64 NumPy on the host. Outputs
are host NumPy arrays (compute_plda: a ktf.layers.PLDA), ready for the ktf.io writers, XvectorExtractor.from_parts and PLDA.

Eigenvector signs: Kaldi's are arbitrary. Here every eigenvector's largest-magnitude component is positive (on a tie the lowest index
decides). A row's sign leaves PLDA scores and LDA'd, length-normalised scores unchanged.

Further down: i-vector extractor training and UBM training, Kaldi's sid/train_diag_ubm.sh and
sid/train_full_ubm.sh: E-steps and fp64 EM statistics on the GPU (csrc/gmm_train.hip), updates on the host."""

import numpy as np
import torch

from . import _lib as L
from . import ops
from ._host import chunks, max_under, per_device
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


# ----------------------------------------------------------------------------- UBM training
def _diag_gmm(g):
    from . import io as kio
    return g if isinstance(g, kio.KaldiDiagGmmReader) else kio.KaldiDiagGmmReader(g, binary=True)


def _full_gmm(g):
    from . import io as kio
    return g if isinstance(g, kio.KaldiFullGmmReader) else kio.KaldiFullGmmReader(g, binary=True)


def _check_gmm_shape(I, D):
    if not (1 <= I <= L.IVECTOR_MAX_GAUSS and 1 <= D <= L.IVECTOR_MAX_FEAT_DIM):
        raise ValueError(f"GMM shape (I={I}, D={D}) outside I <= {L.IVECTOR_MAX_GAUSS}, D <= {L.IVECTOR_MAX_FEAT_DIM}")


def _gmm_frames(feats, D, lengths, mask):
    """feats (B, T, D), or (F, D) = one utterance -> the selected frames (F, D) end to end, as IvectorExtractor.posteriors lays them."""
    from .layers import select_frames
    L.require_gpu()
    if isinstance(feats, torch.Tensor) and feats.dim() == 2:
        feats = feats[None]
    return select_frames(feats, D, lengths, mask)[0]


def _device_consts(gmm, device, make):
    """The model's device arrays, uploaded once per model object and device (a device given as a string is normalised first)."""
    return per_device(gmm, torch.device(device),
                      lambda: tuple(torch.as_tensor(np.ascontiguousarray(a), device=device) for a in make()))


def _diag_consts(d, device):
    """W (2D, I) = [means_invvars^T; -inv_vars^T / 2] and gconst as ktf_ivector_post_f32 takes them, means_invvars, inv_vars."""
    f = np.float32
    return _device_consts(d, device, lambda: (np.concatenate([d.means_invvars.astype(f).T, (f(-0.5) * d.inv_vars.astype(f)).T]),
                                              d.gconsts.astype(f), d.means_invvars.astype(f), d.inv_vars.astype(f)))


def _full_consts(g, device):
    f = np.float32
    return _device_consts(g, device, lambda: (g.means_invcovars.astype(f), g.inv_covars.astype(f), g.gconsts.astype(f)))


def _max_frames(nbytes, limit, n):
    """The most frames F (F * n < 2^31, at least one) for which nbytes(F) <= limit."""
    return max_under(nbytes, limit, ((1 << 31) - 1) // max(int(n), 1))


def select_gaussians(dubm, feats, n, lengths=None, mask=None):
    """gmm-gselect --n=n: the n Gaussians of the diagonal GMM `dubm` (a path to final.dubm, an io.KaldiDiagGmmReader or
    io.DiagGmmModel) with the largest log-likelihood per frame (ties: the lower index; ktf_ivector_post_f32 with min_post = 0) ->
    gselect (F, n) int32 on the device, -1 beyond min(n, I). Frames are laid end to end as IvectorExtractor.posteriors lays them."""
    d = _diag_gmm(dubm)
    _check_gmm_shape(d.numGauss, d.featDim)
    if not 1 <= int(n) <= L.IVECTOR_MAX_GSELECT:
        raise ValueError(f"n {n} outside 1 .. {L.IVECTOR_MAX_GSELECT}")
    x = _gmm_frames(feats, d.featDim, lengths, mask)
    W, gc, _, _ = _diag_consts(d, x.device)
    with L.launch_scope(x.device):
        return ops.ivector_post(x, W, gc, int(n), 0.0)[0]


class _GmmStats:
    """fp64 device accumulators of a GMM's EM statistics (allocated on the device of the first batch): occ (I), mean_acc (I, D) and
    the second-order term; loglike_sum = the sum of the frames' log-likelihoods under the model the statistics are taken with,
    frames = the frames counted (those with a non-empty Gaussian list)."""
    full = False

    def __init__(self, gmm):
        g = (_full_gmm if self.full else _diag_gmm)(gmm)
        _check_gmm_shape(g.numGauss, g.featDim)
        self.shape = (int(g.numGauss), int(g.featDim))
        self.device = None
        self.loglike_sum, self.frames = 0.0, 0

    def _second(self):
        return self.cov_acc if self.full else self.var_acc

    def _alloc(self, device):
        if self.device is not None:
            if torch.device(device) != self.device:
                raise ValueError(f"the statistics live on {self.device}, the batch on {device}")
            return
        I, D = self.shape
        self.device = torch.device(device)
        z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=self.device)  # noqa: E731
        self.occ, self.mean_acc = z(I), z(I, D)
        if self.full:
            self.cov_acc = z(I, D, D)
        else:
            self.var_acc = z(I, D)

    def merge(self, other):
        """gmm-global-sum-accs / fgmm-global-sum-accs: add another object's statistics (taken with the same model) to this one."""
        if type(other) is not type(self) or other.shape != self.shape:
            raise ValueError(f"cannot merge statistics of shape {getattr(other, 'shape', None)} into {self.shape}")
        if other.device is not None:
            self._alloc(other.device)
            self.occ.add_(other.occ)
            self.mean_acc.add_(other.mean_acc)
            self._second().add_(other._second())
        self.loglike_sum += other.loglike_sum
        self.frames += other.frames
        return self

    def host(self):
        """(occ (I), mean_acc (I, D), the second-order accumulator) as NumPy fp64 copies."""
        I, D = self.shape
        if self.device is None:
            return np.zeros(I), np.zeros((I, D)), np.zeros((I, D, D) if self.full else (I, D))
        return self.occ.cpu().numpy(), self.mean_acc.cpu().numpy(), self._second().cpu().numpy()

    def objf(self):
        """The mean frame log-likelihood of the accumulated data under the model the statistics were taken with."""
        if self.frames < 1:
            raise ValueError("objf: no frames accumulated")
        return self.loglike_sum / self.frames


class DiagGmmStats(_GmmStats):
    """Kaldi's AccumDiagGmm (gmm-global-acc-stats): occ (I), mean_acc (I, D), var_acc (I, D) = sum p x^2."""
    full = False


class FullGmmStats(_GmmStats):
    """Kaldi's AccumFullGmm (fgmm-global-acc-stats): occ (I), mean_acc (I, D), cov_acc (I, D, D) = sum p x x^T."""
    full = True


def _check_acc(stats, g, x, gselect, kind):
    if not isinstance(stats, kind) or stats.shape != (g.numGauss, g.featDim):
        raise ValueError(f"statistics of shape {getattr(stats, 'shape', None)} do not match the model {(g.numGauss, g.featDim)}")
    if gselect is None:
        return None
    if not isinstance(gselect, torch.Tensor) or gselect.dim() != 2 or gselect.shape[0] != x.shape[0] or \
            not 1 <= gselect.shape[1] <= L.IVECTOR_MAX_GSELECT:
        raise ValueError(f"gselect must be ({x.shape[0]}, n) with 1 <= n <= {L.IVECTOR_MAX_GSELECT}, got "
                         f"{tuple(getattr(gselect, 'shape', ()))}")
    return gselect.to(device=x.device, dtype=torch.int32).contiguous()


def acc_diag_gmm(stats, gmm, feats, gselect=None, lengths=None, mask=None, workspace_limit=1 << 30):
    """gmm-global-acc-stats on one batch, added to `stats` (DiagGmmStats) in place. With gselect (F, n) int32 (select_gaussians; an
    index outside [0, I) is skipped) the posteriors are taken over each frame's list (ktf_gmm_post_preselect_f32) and the
    statistics over the pairs (ktf_gmm_acc_f64). With gselect=None every Gaussian takes part (the E-step of
    gmm-global-init-from-feats): ktf_gmm_post_dense_f32, then ktf_atb_f64 into (I, 2D + 1). The frames run in chunks whose workspace
    stays under workspace_limit bytes, added in order. -> the number of chunks."""
    d = _diag_gmm(gmm)
    _check_gmm_shape(d.numGauss, d.featDim)
    I, D = d.numGauss, d.featDim
    x = _gmm_frames(feats, D, lengths, mask)
    gsel = _check_acc(stats, d, x, gselect, DiagGmmStats)
    F = x.shape[0]
    if F == 0:
        return 0
    stats._alloc(x.device)
    W, gc, mi, iv = _diag_consts(d, x.device)
    with L.launch_scope(x.device):
        if gsel is None:
            per = I * 4 + I * 8 + (2 * D + 1) * 8                     # workspace, P and Xaug per frame
            step = int(max(1, min(F, int(workspace_limit) // per)))
            tmp = torch.zeros((I, 2 * D + 1), dtype=torch.float64, device=x.device)
            ll_sum = 0.0
            pieces = chunks(F, step)
            for lo, hi in pieces:
                P, Xaug, ll = ops.gmm_post_dense(x[lo:hi], W, gc)
                ops.atb_f64(P, Xaug, tmp)
                ll_sum += float(ll.double().sum())
            stats.occ.add_(tmp[:, 0])
            stats.mean_acc.add_(tmp[:, 1:D + 1])
            stats.var_acc.add_(tmp[:, D + 1:])
            stats.loglike_sum += ll_sum
            stats.frames += F
        else:
            n = gsel.shape[1]
            step = min(F, _max_frames(lambda f: ops.gmm_acc_workspace_bytes(f, I, D, n, False), int(workspace_limit), n))
            valid = torch.zeros((1,), dtype=torch.int32, device=x.device)
            ll_sum = 0.0
            pieces = chunks(F, step)
            for lo, hi in pieces:
                xs, gs = x[lo:hi], gsel[lo:hi]
                post, ll = ops.gmm_post_preselect(xs, gs, mi, iv, gc, valid)
                ops.gmm_acc(xs, gs, post, stats.occ, stats.mean_acc, stats.var_acc)
                ll_sum += float(ll.double().sum())
            stats.loglike_sum += ll_sum
            stats.frames += int(valid.item())
    return len(pieces)


def acc_full_gmm(stats, gmm, feats, gselect, lengths=None, mask=None, workspace_limit=1 << 30):
    """fgmm-global-acc-stats --gselect on one batch, added to `stats` (FullGmmStats) in place: the posteriors of each frame's list
    under the full GMM with their log-likelihood (ktf_fgmm_post_ll_f32, no pruning), then ktf_gmm_acc_f64's full form. Chunked as
    acc_diag_gmm. -> the number of chunks."""
    g = _full_gmm(gmm)
    _check_gmm_shape(g.numGauss, g.featDim)
    I, D = g.numGauss, g.featDim
    x = _gmm_frames(feats, D, lengths, mask)
    if gselect is None:
        raise ValueError("acc_full_gmm needs gselect (select_gaussians)")
    gsel = _check_acc(stats, g, x, gselect, FullGmmStats)
    F = x.shape[0]
    if F == 0:
        return 0
    stats._alloc(x.device)
    mic, ic, gc = _full_consts(g, x.device)
    n = gsel.shape[1]
    step = min(F, _max_frames(lambda f: ops.fgmm_workspace_bytes(f, I, D, n) + ops.gmm_acc_workspace_bytes(f, I, D, n, True),
                              int(workspace_limit), n))
    pieces = chunks(F, step)
    ll_sum, frames = 0.0, 0
    with L.launch_scope(x.device):
        for lo, hi in pieces:
            xs = x[lo:hi]
            gauss, post, ll = ops.fgmm_post_ll(xs, gsel[lo:hi], mic, ic, gc, 0.0)
            ops.gmm_acc(xs, gauss, post, stats.occ, stats.mean_acc, stats.cov_acc)
            ll_sum += float(ll.double().sum())
            frames += int((gauss[:, 0] >= 0).sum())
    stats.loglike_sum += ll_sum
    stats.frames += frames
    return len(pieces)


def _diag_params(d):
    """(means, variances) in fp64 from the stored fp32 fields."""
    var = 1.0 / d.inv_vars.astype(np.float64)
    return d.means_invvars.astype(np.float64) * var, var


def _diag_model(weights, mean, var):
    from . import io as kio
    return kio.DiagGmmModel(weights, mean / var, 1.0 / var)


def _est_gate(occ, min_gaussian_weight, min_gaussian_occupancy):
    tot = occ.sum()
    if not tot > 0:
        raise ValueError("no statistics accumulated")
    prob = occ / tot
    return prob, (occ > float(min_gaussian_occupancy)) & (prob > float(min_gaussian_weight))


def diag_gmm_est(gmm, stats, min_gaussian_weight=1e-5, min_gaussian_occupancy=10.0, min_variance=0.001, remove_low_count_gaussians=True):
    """gmm-global-est (MleDiagGmmUpdate, all of weights, means and variances) -> io.DiagGmmModel. prob_i = occ_i / sum occ; a Gaussian
    with occ_i > min_gaussian_occupancy and prob_i > min_gaussian_weight gets mean = mean_acc / occ, var = max(var_acc / occ -
    mean^2, min_variance), weight prob_i; any other is removed or, with remove_low_count_gaussians=False, keeps its mean and
    variance and takes weight prob_i. Weights are renormalised. ValueError if every Gaussian would be removed. The model's
    `estInfo`: {"removed", "floored" (variance elements floored), "kept" (the indices of the Gaussians kept)}."""
    d = _diag_gmm(gmm)
    if not isinstance(stats, DiagGmmStats) or stats.shape != (d.numGauss, d.featDim):
        raise ValueError(f"statistics of shape {getattr(stats, 'shape', None)} do not match the model {(d.numGauss, d.featDim)}")
    occ, macc, vacc = stats.host()
    prob, ok = _est_gate(occ, min_gaussian_weight, min_gaussian_occupancy)
    mean, var = _diag_params(d)
    o = occ[ok][:, None]
    m = macc[ok] / o
    v = vacc[ok] / o - m * m
    floored = int((v < float(min_variance)).sum())
    mean[ok], var[ok] = m, np.maximum(v, float(min_variance))
    keep = ok if remove_low_count_gaussians else np.ones_like(ok)
    if not keep.any():
        raise ValueError("gmm-global-est: every Gaussian would be removed (too few frames)")
    w = prob[keep]
    out = _diag_model(w / w.sum(), mean[keep], var[keep])
    out.estInfo = {"removed": int((~keep).sum()), "floored": floored, "kept": np.nonzero(keep)[0]}
    return out


def full_gmm_est(gmm, stats, min_gaussian_weight=1e-5, min_gaussian_occupancy=100.0, variance_floor=0.001, max_condition=1e5,
                 remove_low_count_gaussians=True):
    """fgmm-global-est (MleFullGmmUpdate) -> io.FullGmmModel. The gate of diag_gmm_est; cov = cov_acc / occ - mean mean^T,
    symmetrised, = V diag(lam) V^T with lam floored at max(variance_floor, lam_max / max_condition); inv_covars = V diag(1 / lam)
    V^T, means_invcovars = inv_covars mean. `estInfo`: {"removed", "floored" (Gaussians with a floored eigenvalue), "kept"}."""
    from . import io as kio
    g = _full_gmm(gmm)
    if not isinstance(stats, FullGmmStats) or stats.shape != (g.numGauss, g.featDim):
        raise ValueError(f"statistics of shape {getattr(stats, 'shape', None)} do not match the model {(g.numGauss, g.featDim)}")
    occ, macc, cacc = stats.host()
    prob, ok = _est_gate(occ, min_gaussian_weight, min_gaussian_occupancy)
    ic = g.inv_covars.astype(np.float64)
    mic = g.means_invcovars.astype(np.float64)
    floored = 0
    if ok.any():
        o = occ[ok]
        m = macc[ok] / o[:, None]
        cov = cacc[ok] / o[:, None, None] - m[:, :, None] * m[:, None, :]
        lam, V = np.linalg.eigh(0.5 * (cov + np.swapaxes(cov, 1, 2)))
        floor = np.maximum(float(variance_floor), lam.max(1) / float(max_condition))
        floored = int((lam < floor[:, None]).any(1).sum())
        lam = np.maximum(lam, floor[:, None])
        inv = np.matmul(V / lam[:, None, :], np.swapaxes(V, 1, 2))
        ic[ok] = 0.5 * (inv + np.swapaxes(inv, 1, 2))
        mic[ok] = np.einsum("ide,ie->id", ic[ok], m)
    keep = ok if remove_low_count_gaussians else np.ones_like(ok)
    if not keep.any():
        raise ValueError("fgmm-global-est: every Gaussian would be removed (too few frames)")
    w = prob[keep]
    out = kio.FullGmmModel(w / w.sum(), mic[keep], ic[keep])
    out.estInfo = {"removed": int((~keep).sum()), "floored": floored, "kept": np.nonzero(keep)[0]}
    return out


def split_largest(weights, mean, var, target, normals):
    """Kaldi's DiagGmm::Split on fp64 arrays: until there are `target` Gaussians, the one of largest weight (ties: the lower index)
    halves its weight and is copied; the copy's mean is + 0.1 sqrt(var) * r, the original's - 0.1 sqrt(var) * r, r = next(normals)
    (D standard normal values). -> (weights, mean, var)."""
    w, m, v = list(weights), list(mean), list(var)
    while len(w) < target:
        i = int(np.argmax(w))
        r = np.asarray(next(normals), dtype=np.float64)
        w[i] *= 0.5
        step = 0.1 * np.sqrt(v[i]) * r
        w.append(w[i])
        m.append(m[i] + step)
        v.append(v[i].copy())
        m[i] = m[i] - step
    return np.asarray(w), np.asarray(m), np.asarray(v)


def init_diag_ubm(feats, num_gauss, num_gauss_init=None, num_iters=20, num_frames=500000, lengths=None, mask=None, seed=0,
                  workspace_limit=1 << 30, **est):
    """gmm-global-init-from-feats --num-gauss --num-gauss-init --num-iters --num-frames -> (io.DiagGmmModel, [objf of iteration 0,
    1, ...]). Every random draw comes from rng = np.random.default_rng(seed) on the host, in this order: (1) if there are more than
    num_frames frames, rng.choice(F, num_frames, replace=False), sorted ascending; (2) rng.choice(F', num_gauss_init, replace=False),
    the frames that become the initial means; (3) one rng.standard_normal(D) per split, in split order. The initial model has the
    global variance (floored at 1e-10) and uniform weights. Then num_iters dense EM iterations (acc_diag_gmm without gselect,
    diag_gmm_est(**est)); after each the model is split (split_largest) up to cur = min(num_gauss, cur + (num_gauss -
    num_gauss_init) // max(1, num_iters // 2)), cur starting at num_gauss_init. num_gauss_init defaults to num_gauss // 2 (at least 1).
    Kaldi's own generator is not reproduced."""
    num_gauss, num_iters = int(num_gauss), int(num_iters)
    ngi = max(1, num_gauss // 2) if num_gauss_init is None else int(num_gauss_init)
    if not 1 <= ngi <= num_gauss <= L.IVECTOR_MAX_GAUSS or num_iters < 1 or int(num_frames) < 1:
        raise ValueError(f"need 1 <= num_gauss_init ({ngi}) <= num_gauss ({num_gauss}) <= {L.IVECTOR_MAX_GAUSS}, num_iters >= 1 and "
                         "num_frames >= 1")
    D = feats.shape[-1] if isinstance(feats, torch.Tensor) else 0
    if not 1 <= D <= L.IVECTOR_MAX_FEAT_DIM:
        raise ValueError(f"feature dim {D} outside 1 .. {L.IVECTOR_MAX_FEAT_DIM}")
    x = _gmm_frames(feats, D, lengths, mask)
    rng = np.random.default_rng(seed)
    if x.shape[0] > int(num_frames):
        idx = np.sort(rng.choice(x.shape[0], int(num_frames), replace=False))
        x = x[torch.as_tensor(idx, device=x.device)].contiguous()
    F = x.shape[0]
    if F < ngi:
        raise ValueError(f"{F} frames cannot seed {ngi} Gaussians")
    first = rng.choice(F, ngi, replace=False)
    xd = x.double()
    gmean = xd.mean(0)
    gvar = ((xd * xd).mean(0) - gmean * gmean).clamp_min(1e-10).cpu().numpy()
    mean = x[torch.as_tensor(first, device=x.device)].double().cpu().numpy()
    model = _diag_model(np.full(ngi, 1.0 / ngi), mean, np.tile(gvar, (ngi, 1)))
    normals = (rng.standard_normal(D) for _ in iter(int, 1))            # one draw per split, as long as splits are asked for
    inc = (num_gauss - ngi) // max(1, num_iters // 2)
    cur, objfs = ngi, []
    for _ in range(num_iters):
        stats = DiagGmmStats(model)
        acc_diag_gmm(stats, model, x, workspace_limit=workspace_limit)
        objfs.append(stats.objf())
        model = diag_gmm_est(model, stats, **est)
        cur = min(num_gauss, cur + inc)
        if cur > model.numGauss:
            m, v = _diag_params(model)
            model = _diag_model(*split_largest(model.weights.astype(np.float64), m, v, cur, normals))
    return model, objfs


def diag_to_full(dubm):
    """gmm-global-to-fgmm: the same weights and means, inv_covars = diag(inv_vars) -> io.FullGmmModel."""
    from . import io as kio
    d = _diag_gmm(dubm)
    I, D = d.numGauss, d.featDim
    ic = np.zeros((I, D, D), np.float32)
    ic[:, np.arange(D), np.arange(D)] = d.inv_vars.astype(np.float32)
    return kio.FullGmmModel(d.weights, d.means_invvars, ic)


def _remap_gselect(gsel, kept, I):
    """The cached lists after a removal: old index -> new index, a removed Gaussian -> -1."""
    table = np.full(I + 1, -1, np.int32)                     # entry I serves the indices outside [0, I)
    table[kept] = np.arange(len(kept), dtype=np.int32)
    t = torch.as_tensor(table, device=gsel.device)
    g = gsel.long()
    return t[torch.where((g >= 0) & (g < I), g, torch.full_like(g, I))]


def _train_ubm(model, sel_model, batches, gselect_n, num_iters, gselect, stats_cls, acc, est, est_kwargs):
    batches = [tuple(b) if isinstance(b, (tuple, list)) else (b,) for b in batches]
    if gselect is None:
        gselect = [select_gaussians(sel_model, b[0], gselect_n, *b[1:]) for b in batches]
    elif len(gselect) != len(batches):
        raise ValueError(f"gselect must hold one (F, n) tensor per batch ({len(batches)}), got {len(gselect)}")
    gselect = list(gselect)
    remove_last = bool(est_kwargs.pop("remove_low_count_gaussians", True))
    objfs = []
    for it in range(int(num_iters)):
        stats = stats_cls(model)
        for b, gs in zip(batches, gselect):
            acc(stats, model, b[0], gs, *b[1:])
        objfs.append(stats.objf())
        I = model.numGauss
        model = est(model, stats, remove_low_count_gaussians=remove_last and it == int(num_iters) - 1, **est_kwargs)
        if model.estInfo["removed"]:
            gselect = [_remap_gselect(gs.to(torch.int32), model.estInfo["kept"], I) for gs in gselect]
    return model, objfs


def train_diag_ubm(dubm, batches, gselect_n=30, num_iters=4, gselect=None, **est):
    """sid/train_diag_ubm.sh after the initialisation: gmm-gselect once from the incoming model, then num_iters times
    gmm-global-acc-stats --gselect over `batches` (a list of argument tuples (feats[, lengths[, mask]])) and gmm-global-est(**est),
    low-count Gaussians removed on the last iteration only (the cached lists are remapped, removed entries become -1). `gselect`:
    one (F, n) tensor per batch in place of the computed lists. -> (io.DiagGmmModel, [objf of each iteration])."""
    d = _diag_gmm(dubm)
    return _train_ubm(d, d, batches, gselect_n, num_iters, gselect, DiagGmmStats, acc_diag_gmm, diag_gmm_est, dict(est))


def train_full_ubm(fubm, batches, gselect_n=20, num_iters=4, gselect=None, **est):
    """sid/train_full_ubm.sh: gmm-gselect once from fubm.toDiag() (fgmm-global-to-gmm), then num_iters times fgmm-global-acc-stats
    --gselect and fgmm-global-est(**est), low-count Gaussians removed on the last iteration only. `fubm`: a path to final.ubm, an
    io.KaldiFullGmmReader or io.FullGmmModel (diag_to_full). -> (io.FullGmmModel, [objf of each iteration])."""
    g = _full_gmm(fubm)
    return _train_ubm(g, None if gselect is not None else g.toDiag(), batches, gselect_n, num_iters, gselect, FullGmmStats, acc_full_gmm,
                      full_gmm_est, dict(est))
