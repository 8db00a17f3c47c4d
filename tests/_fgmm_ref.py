"""fp64 NumPy restatement of the full-covariance posterior stage of Kaldi's sid/extract_ivectors.sh (gmm-gselect |
fgmm-global-gselect-to-post), of fgmm-global-to-gmm and of add-deltas (fp32, in the stated order), a writer of Kaldi-binary
<FullGMM> files and a generator of random SPD full UBMs with frames drawn from the mixture. The diagonal parts and the binary
writers come from _ivector_ref."""

import numpy as np

import _ivector_ref as R


# ------------------------------------------------------------------ models and files
def write_full_gmm(path, weights, means_invcovars, inv_covars, gconsts=None, with_gconsts=True):
    """<FullGMM> [<GCONSTS> FV] <WEIGHTS> FV <MEANS_INVCOVARS> FM <INV_COVARS> (FP) x I </FullGMM> (fp32); gconsts: what is stored
    (zeros by default: the reader recomputes them)."""
    I = len(weights)
    g = np.zeros(I, np.float32) if gconsts is None else gconsts
    with open(path, "wb") as f:
        f.write(b"\x00B" + R._tok("<FullGMM>"))
        if with_gconsts:
            f.write(R._tok("<GCONSTS>") + R._vec(g, np.float32))
        f.write(R._tok("<WEIGHTS>") + R._vec(weights, np.float32) + R._tok("<MEANS_INVCOVARS>") + R._mat(means_invcovars, np.float32)
                + R._tok("<INV_COVARS>"))
        for i in range(I):
            f.write(R._packed(inv_covars[i], np.float32))
        f.write(R._tok("</FullGMM>"))


def random_full_ubm(rng, I, D):
    """Weights, means ~ N(0, 1), covariances A A^T * 0.04 + c I with c in [0.5, 2] -> ((weights, means_invcovars, inv_covars) as a
    FullGmm stores them, fp32, inv_covars symmetric bit for bit), (means, covars) fp64 for drawing frames."""
    w = rng.uniform(0.5, 1.5, I)
    w = (w / w.sum()).astype(np.float32)
    mean = rng.standard_normal((I, D))
    A = rng.standard_normal((I, D, D))
    cov = np.einsum("idk,iek->ide", A, A) * 0.04 + np.eye(D)[None] * rng.uniform(0.5, 2.0, (I, 1, 1))
    ic = np.linalg.inv(cov)
    ic = (0.5 * (ic + np.swapaxes(ic, 1, 2))).astype(np.float32)
    r, c = np.tril_indices(D)
    ic[:, c, r] = ic[:, r, c]
    mic = np.einsum("ide,ie->id", ic.astype(np.float64), mean).astype(np.float32)
    return (w, mic, ic), (mean, cov)


def draw_frames(rng, mean, cov, F, comp=None):
    """F frames from the mixture (a uniformly random component each, or the components `comp`), fp32."""
    c = rng.integers(0, mean.shape[0], F) if comp is None else np.asarray(comp)
    Lc = np.linalg.cholesky(cov)
    z = rng.standard_normal((F, mean.shape[1]))
    return (mean[c] + np.einsum("fde,fe->fd", Lc[c], z)).astype(np.float32)


def gconsts(weights, means_invcovars, inv_covars):
    """FullGmm::ComputeGconsts in fp64: log w - D/2 log 2 pi - (log det Sigma + mu^T Sigma^-1 mu) / 2."""
    ic = np.asarray(inv_covars, np.float64)
    mic = np.asarray(means_invcovars, np.float64)
    D = mic.shape[1]
    mu = np.linalg.solve(ic, mic[..., None])[..., 0]
    logdet = -np.linalg.slogdet(ic)[1]
    return np.log(np.asarray(weights, np.float64)) - 0.5 * D * np.log(2 * np.pi) - 0.5 * (logdet + np.sum(mu * mic, axis=1))


def to_diag(weights, means_invcovars, inv_covars):
    """fgmm-global-to-gmm in fp64 -> (weights, means_invvars, inv_vars)."""
    cov = np.linalg.inv(np.asarray(inv_covars, np.float64))
    iv = 1.0 / np.einsum("idd->id", cov)
    mu = np.einsum("ide,ie->id", cov, np.asarray(means_invcovars, np.float64))
    return np.asarray(weights, np.float64), mu * iv, iv


# ------------------------------------------------------------------ posteriors
def gselect(x, diag, n):
    """gmm-gselect --n on the diagonal UBM diag = (gconst, means_invvars, inv_vars): (F, n) int32, the min(n, I) best by diagonal
    log-likelihood (ties: the lower index), padded with -1."""
    ll = R.loglikes(x, diag)
    F, I = ll.shape
    out = np.full((F, n), -1, np.int32)
    for t in range(F):
        out[t, :min(n, I)] = np.lexsort((np.arange(I), -ll[t]))[:n]
    return out


def loglikes_on(x, full, sel):
    """fp64 l = gconst + means_invcovars . x - x^T inv_covars x / 2 of the Gaussians listed per frame in sel (F, n); entries outside
    [0, I) give -inf. full = (gconst, means_invcovars, inv_covars)."""
    gc, mic, ic = (np.asarray(a, np.float64) for a in full)
    x = np.asarray(x, np.float64)
    I = gc.shape[0]
    ok = (sel >= 0) & (sel < I)
    g = np.where(ok, sel, 0)
    lin = np.einsum("fnd,fd->fn", mic[g], x)
    quad = np.zeros(sel.shape)
    for t0 in range(0, x.shape[0], 32):                      # (32, n, D, D) gathered matrices at a time
        xs = x[t0:t0 + 32]
        quad[t0:t0 + 32] = np.einsum("fne,fe->fn", np.einsum("fd,fnde->fne", xs, ic[g[t0:t0 + 32]]), xs)
    return np.where(ok, gc[g] + lin - 0.5 * quad, -np.inf)


def prune(idx, ll, min_post):
    """One frame: softmax over the listed Gaussians (idx < 0 = not listed), every p < min_post set to 0 and the rest divided by
    their sum, the arg-max (ties: the lower index) getting 1 if that sum is 0; the Gaussians with p != 0 sorted by posterior,
    descending (ties: the lower index) -> (gauss, post, the posteriors before pruning in list order)."""
    idx = np.asarray(idx)
    ok = idx >= 0
    if not ok.any():
        return np.zeros(0, np.int32), np.zeros(0), np.zeros(0)
    l = np.where(ok, ll, -np.inf)
    top = np.lexsort((idx, -l))[0]
    e = np.where(ok, np.exp(l - l[top]), 0.0)
    pre = e / e.sum()
    p = pre.copy()
    if min_post != 0:
        p[p < min_post] = 0.0
        s = p.sum()
        if s == 0:
            p[top] = 1.0
        else:
            p = p / s
    keep = np.nonzero(ok & (p != 0))[0]
    order = keep[np.lexsort((idx[keep], -p[keep]))]
    return idx[order].astype(np.int32), p[order], pre[ok]


def posteriors(x, full, sel, min_post):
    """(gauss (F, n) int32, post (F, n) fp64) with unused slots (-1, 0), and per frame the smallest distance of a posterior
    before pruning from min_post (inf when min_post is 0)."""
    ll = loglikes_on(x, full, sel)
    F, n = sel.shape
    g = np.full((F, n), -1, np.int32)
    p = np.zeros((F, n))
    dist = np.full(F, np.inf)
    for t in range(F):
        gt, pt, pre = prune(np.where(np.isfinite(ll[t]), sel[t], -1), ll[t], min_post)
        g[t, :len(gt)] = gt
        p[t, :len(gt)] = pt
        if min_post != 0 and len(pre):
            dist[t] = np.abs(pre - min_post).min()
    return g, p, dist


def well_posed(x, diag, full, n, min_post):
    """(sel, mask): a frame is well posed when (a) the diagonal log-likelihoods ranked n and n + 1 differ by >= 1e-3 (no condition
    when every Gaussian is listed) and (b) every posterior before pruning is >= 2e-4 away from min_post."""
    ll = R.loglikes(x, diag)
    I = ll.shape[1]
    sel = gselect(x, diag, n)
    ok = np.ones(ll.shape[0], bool)
    if n < I:
        s = -np.sort(-ll, axis=1)
        ok &= (s[:, n - 1] - s[:, n]) >= 1e-3
    _, _, dist = posteriors(x, full, sel, min_post)
    ok &= dist >= 2e-4
    return sel, ok


def diag_of(full_w_mic_ic):
    """The diagonal UBM (gconst, means_invvars, inv_vars) in fp32 as KaldiFullGmmReader.toDiag() makes it, from the oracle."""
    from kaldi_tflite_amd.io import KaldiDiagGmmReader
    w, mi, iv = to_diag(*full_w_mic_ic)
    d = KaldiDiagGmmReader.__new__(KaldiDiagGmmReader)
    d.weights, d.means_invvars, d.inv_vars = w.astype(np.float32), mi.astype(np.float32), iv.astype(np.float32)
    d.numGauss, d.featDim = mi.shape
    d.gconsts = d.computeGconsts()
    return d


# the configurations of the GPU test: (I, D, n, min_post); 600 frames drawn from the mixture, seed = the row's index
CONFIGS = [(2047, 24, 20, 0.025), (2047, 24, 8, 0.025), (2047, 24, 5, 0.0), (2048, 60, 20, 0.025), (256, 60, 50, 0.0),
           (37, 60, 20, 0.025), (12, 24, 20, 0.025)]
FRAMES = 600


def config_case(k):
    """Model, frames, lists and the well-posed mask of configuration k."""
    I, D, n, min_post = CONFIGS[k]
    rng = np.random.default_rng(1000 + k)
    stored, (mean, cov) = random_full_ubm(rng, I, D)
    x = draw_frames(rng, mean, cov, FRAMES)
    diag = diag_of(stored)
    full = (gconsts(*stored).astype(np.float32), stored[1], stored[2])
    sel, ok = well_posed(x, (diag.gconsts, diag.means_invvars, diag.inv_vars), full, n, min_post)
    return stored, diag, full, x, sel, ok


POPULAR = (40, 24, 4, 0.025)        # (I, D, n, min_post) of the skewed case: 3000 frames, all drawn from component 3
POPULAR_FRAMES = 3000


def popular_case():
    """Means four times as far apart, every frame drawn from component 3: its bucket holds every frame, most others nothing."""
    I, D, n, min_post = POPULAR
    rng = np.random.default_rng(24)
    stored, (mean, cov) = random_full_ubm(rng, I, D)
    mean = mean * 4.0
    stored = (stored[0], np.einsum("ide,ie->id", stored[2].astype(np.float64), mean).astype(np.float32), stored[2])
    x = draw_frames(rng, mean, cov, POPULAR_FRAMES, comp=np.full(POPULAR_FRAMES, 3))
    diag = diag_of(stored)
    full = (gconsts(*stored).astype(np.float32), stored[1], stored[2])
    sel, ok = well_posed(x, (diag.gconsts, diag.means_invvars, diag.inv_vars), full, n, min_post)
    return stored, diag, full, x, sel, ok


WHOLE = (64, 20, 20, 0.025)         # (I, D, n, min_post) of the whole-call case
WHOLE_LENS = [120, 1, 0, 64]


def whole_call_case():
    """The whole-call case: a pool of 600 frames drawn from the mixture, its well-posed frames handed out to the utterances in
    order -> (stored, (mean, cov), diag, full, pool, ok)."""
    I, D, n, min_post = WHOLE
    rng = np.random.default_rng(22)
    stored, (mean, cov) = random_full_ubm(rng, I, D)
    pool = draw_frames(rng, mean, cov, FRAMES)
    diag = diag_of(stored)
    full = (gconsts(*stored).astype(np.float32), stored[1], stored[2])
    _, ok = well_posed(pool, (diag.gconsts, diag.means_invvars, diag.inv_vars), full, n, min_post)
    return stored, diag, full, pool, ok


# ------------------------------------------------------------------ add-deltas
def delta_coeffs(order, window):
    """DeltaFeatures' scales, fp32: a list of order + 1 filters, filter i of length 2 i window + 1."""
    f = np.float32
    s = [np.ones(1, f)]
    for i in range(1, order + 1):
        prev = s[-1]
        cur = np.zeros(len(prev) + 2 * window, f)
        norm = f(0)
        for j in range(-window, window + 1):
            norm = f(norm + f(j * j))
            for k in range(len(prev)):
                cur[j + window + k] = f(cur[j + window + k] + f(f(j) * prev[k]))
        s.append((cur / norm).astype(f))
    return s


def add_deltas(x, lengths, order, window):
    """x (B, T, D) fp32 -> (B, T, D (order + 1)) fp32: block i of frame t = sum_j s_i[j] x[clamp(t + j, 0, len - 1)], j ascending,
    zero coefficients skipped, every step acc = fl(acc + fl(s * x)); rows at and beyond lengths[b] zero."""
    f = np.float32
    x = np.asarray(x, f)
    B, T, D = x.shape
    s = delta_coeffs(order, window)
    out = np.zeros((B, T, D * (order + 1)), f)
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        if n == 0:
            continue
        t = np.arange(n)
        for i in range(order + 1):
            acc = np.zeros((n, D), f)
            half = i * window
            for j in range(-half, half + 1):
                c = s[i][j + half]
                if c == 0:
                    continue
                acc = (acc + (c * x[b, np.clip(t + j, 0, n - 1)]).astype(f)).astype(f)
            out[b, :n, i * D:(i + 1) * D] = acc
    return out
