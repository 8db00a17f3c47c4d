"""fp64 NumPy restatement of i-vector extraction (gmm-global-get-post | scale-post | ivector-extract, sid/extract_ivectors.sh) and
writers of Kaldi-binary <DiagGMM> / <IvectorExtractor> files for random models.

Two independent forms of the extraction: `extract_packed` follows Kaldi's data flow (packed U, gamma . U, Cholesky of the packed
quadratic term); `extract_dense` solves (I + sum_i gamma_i M_i^T SigmaInv_i M_i) w = sum_i M_i^T SigmaInv_i F_i + offset e0 with
np.linalg.solve from the model's M and SigmaInv alone."""

import struct

import numpy as np


# ------------------------------------------------------------------ writers (Kaldi binary: "\0B", tokens, typed containers)
def _tok(t):
    return t.encode() + b" "


def _int(v):
    return b"\x04" + struct.pack("<i", int(v))


def _dbl(v):
    return b"\x08" + struct.pack("<d", float(v))


def _vec(a, dt):
    a = np.ascontiguousarray(a, dtype=dt)
    return (b"FV " if dt == np.float32 else b"DV ") + _int(a.shape[0]) + a.tobytes()


def _mat(a, dt):
    a = np.ascontiguousarray(a, dtype=dt).reshape(a.shape[0] if a.ndim == 2 else 0, -1 if a.size else 0)
    rows, cols = a.shape
    return (b"FM " if dt == np.float32 else b"DM ") + _int(rows) + _int(cols) + a.tobytes()


def _packed(a, dt):
    n = a.shape[0]
    r, c = np.tril_indices(n)
    return (b"FP " if dt == np.float32 else b"DP ") + _int(n) + np.ascontiguousarray(a[r, c], dtype=dt).tobytes()


def write_diag_gmm(path, weights, means_invvars, inv_vars, gconsts=None):
    """<DiagGMM> <GCONSTS> FV <WEIGHTS> FV <MEANS_INVVARS> FM <INV_VARS> FM </DiagGMM> (fp32). gconsts: what is stored (zeros by
    default: the reader recomputes them)."""
    I = len(weights)
    g = np.zeros(I, np.float32) if gconsts is None else gconsts
    with open(path, "wb") as f:
        f.write(b"\x00B" + _tok("<DiagGMM>") + _tok("<GCONSTS>") + _vec(g, np.float32) + _tok("<WEIGHTS>") + _vec(weights, np.float32)
                + _tok("<MEANS_INVVARS>") + _mat(means_invvars, np.float32) + _tok("<INV_VARS>") + _mat(inv_vars, np.float32)
                + _tok("</DiagGMM>"))


def write_ivector_extractor(path, M, sigma_inv, prior_offset, w_vec=None, w=None):
    """<IvectorExtractor> <w> DM <w_vec> DV <M> I (DM)* <SigmaInv> (DP)* <IvectorOffset> double </IvectorExtractor> (fp64)."""
    I, D, S = M.shape
    w = np.zeros((0, 0)) if w is None else w
    w_vec = np.full(I, 1.0 / I) if w_vec is None else w_vec
    with open(path, "wb") as f:
        f.write(b"\x00B" + _tok("<IvectorExtractor>") + _tok("<w>") + _mat(w, np.float64) + _tok("<w_vec>") + _vec(w_vec, np.float64)
                + _tok("<M>") + _int(I))
        for i in range(I):
            f.write(_mat(M[i], np.float64))
        f.write(_tok("<SigmaInv>"))
        for i in range(I):
            f.write(_packed(sigma_inv[i], np.float64))
        f.write(_tok("<IvectorOffset>") + _dbl(prior_offset) + _tok("</IvectorExtractor>"))


def random_models(rng, I, D, S, prior_offset=100.0, full_sigma=True):
    """A random UBM (weights, means_invvars, inv_vars) and extractor (M (I, D, S), SPD SigmaInv (I, D, D)) of comparable scale."""
    w = rng.uniform(0.5, 1.5, I)
    w = (w / w.sum()).astype(np.float32)
    iv = rng.uniform(0.5, 2.0, (I, D)).astype(np.float32)
    mean = rng.standard_normal((I, D))
    mi = (mean * iv).astype(np.float32)
    M = rng.standard_normal((I, D, S)) * 0.3
    M[:, :, 0] = mean / prior_offset                   # w = prior_offset e0 reproduces the UBM means
    if full_sigma:
        A = rng.standard_normal((I, D, D)) * 0.2
        sig = np.einsum("idk,iek->ide", A, A) + np.eye(D)[None] * rng.uniform(0.5, 2.0, (I, 1, 1))
    else:
        sig = np.eye(D)[None] * rng.uniform(0.5, 2.0, (I, 1, D))
    return (w, mi, iv), (M, sig)


# ------------------------------------------------------------------ (a) posteriors
def loglikes(x, gmm):
    """fp64 log-likelihoods (F, I) of the diagonal UBM: gconst + x . mi - x^2 . iv / 2."""
    gconst, mi, iv = gmm
    x = np.asarray(x, np.float64)
    return np.asarray(gconst, np.float64)[None] + x @ np.asarray(mi, np.float64).T - 0.5 * (x * x) @ np.asarray(iv, np.float64).T


def select(ll, n, min_post):
    """The selection contract on one frame's log-likelihoods: the n largest (ties: lower index), exp(l - max) normalised over the
    kept set, the smallest dropped while below min_post of the running sum (at least one kept), renormalised. -> (idx, post)."""
    I = ll.shape[0]
    n = min(n, I)
    order = np.lexsort((np.arange(I), -ll))[:n]
    e = np.exp(ll[order] - ll[order[0]])
    keep, s = n, e.sum()
    while keep > 1 and e[keep - 1] < min_post * s:
        s -= e[keep - 1]
        keep -= 1
    return order[:keep].astype(np.int32), e[:keep] / s


def posteriors(x, gmm, n, min_post):
    """(gauss (F, n) int32, post (F, n)) with unused slots (-1, 0), as ktf_ivector_post_f32 lays them out."""
    ll = loglikes(x, gmm)
    F = ll.shape[0]
    g = np.full((F, n), -1, np.int32)
    p = np.zeros((F, n))
    for t in range(F):
        idx, pt = select(ll[t], n, min_post)
        g[t, :len(idx)] = idx
        p[t, :len(idx)] = pt
    return g, p


def margins(x, gmm, n, min_post):
    """Per frame: the distance of the n-th and (n+1)-th log-likelihoods and of every normalised posterior from the cut-offs (the
    smaller the more a rounding difference could change the selection)."""
    ll = loglikes(x, gmm)
    out = np.zeros(ll.shape[0])
    I = ll.shape[1]
    for t in range(ll.shape[0]):
        s = np.sort(ll[t])[::-1]
        m = s[n - 1] - s[n] if n < I else np.inf
        idx, p = select(ll[t], n, min_post)
        e = np.exp(s[:min(n, I)] - s[0])
        if min_post > 0:
            m = min(m, np.min(np.abs(e / e.sum() - min_post)), np.min(np.abs(p - min_post)))
        out[t] = m
    return out


# ------------------------------------------------------------------ (b) - (d)
def count_scale(post, posterior_scale=1.0, acoustic_weight=1.0, max_count=0.0):
    """scale-post, then ivector-extract's acoustic_weight x max_count scale, in Kaldi's precisions -> the fp32 weights."""
    p = (np.asarray(post, np.float32) * np.float32(posterior_scale)).astype(np.float32)
    this_t = float(np.float32(acoustic_weight)) * float(np.sum(p, dtype=np.float64))
    mcs = float(np.float32(max_count)) / this_t if (max_count > 0 and this_t > float(np.float32(max_count))) else 1.0
    scale = np.float32(float(np.float32(acoustic_weight)) * mcs)
    return (p * scale).astype(np.float32)


def stats(x, gauss, post, I, **scales):
    """gamma (I) and F (I, D) in fp64 from one utterance's frames and slots."""
    w = count_scale(post, **scales).astype(np.float64)
    x = np.asarray(x, np.float64)
    gamma = np.zeros(I)
    F = np.zeros((I, x.shape[1]))
    for t in range(x.shape[0]):
        for s in range(gauss.shape[1]):
            g = gauss[t, s]
            if 0 <= g < I:
                gamma[g] += w[t, s]
                F[g] += w[t, s] * x[t]
    return gamma, F


def derived(M, sigma_inv):
    """sigmaInvM (I, D, S) and packed U (I, S(S+1)/2), as the reader derives them."""
    sim = np.matmul(sigma_inv, M)
    S = M.shape[2]
    r, c = np.tril_indices(S)
    return sim, np.matmul(np.swapaxes(M, 1, 2), sim)[:, r, c]


def extract_packed(gamma, F, sim, U, prior_offset):
    """GetIvectorDistMean + GetIvectorDistPrior + the solve, ivector(0) -= prior_offset (Kaldi's data flow)."""
    S = sim.shape[2]
    if not gamma.any() and not F.any():
        return np.zeros(S)
    lin = np.einsum("ids,id->s", sim, F)
    lin[0] += prior_offset
    q = gamma @ U
    Q = np.zeros((S, S))
    r, c = np.tril_indices(S)
    Q[r, c] = q
    Q[c, r] = q
    Q += np.eye(S)
    L = np.linalg.cholesky(Q)
    w = np.linalg.solve(L.T, np.linalg.solve(L, lin))
    w[0] -= prior_offset
    return w


def extract_dense(gamma, F, M, sigma_inv, prior_offset):
    """(I + sum_i gamma_i M_i^T SigmaInv_i M_i) w = sum_i M_i^T SigmaInv_i F_i + offset e0 by np.linalg.solve."""
    S = M.shape[2]
    if not gamma.any() and not F.any():
        return np.zeros(S)
    A = np.eye(S) + np.einsum("i,ids,ide,iet->st", gamma, M, sigma_inv, M)
    b = np.einsum("ids,ide,ie->s", M, sigma_inv, F)
    b[0] += prior_offset
    w = np.linalg.solve(A, b)
    w[0] -= prior_offset
    return w
