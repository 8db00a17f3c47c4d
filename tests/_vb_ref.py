"""Plain fp64 NumPy oracle of the VB-HMM resegmentation: dense posteriors, explicit loops, a log-domain
forward-backward with logaddexp and np.linalg.inv. Every stage is a function of its own; `run` takes supplied (gauss, post, loglike)."""

import itertools

import numpy as np


def random_model(rng, I, D, R, spread=2.0):
    """-> (weights, means_invvars, inv_vars) fp32 as a DiagGMM stores them, and M (I, D, R) fp64."""
    mean = rng.standard_normal((I, D)) * spread
    var = rng.uniform(0.5, 1.5, (I, D))
    w = rng.dirichlet(np.full(I, 5.0))
    return (w.astype(np.float32), (mean / var).astype(np.float32), (1.0 / var).astype(np.float32)), rng.standard_normal((I, D, R)) * 0.3


def consts(mi, iv, M):
    """m (I, D), iE (I, D), B (I D, R), UU (I, R, R) from the fp32 UBM arrays and M."""
    iE = iv.astype(np.float64)
    m = mi.astype(np.float64) / iE
    I, D, R = M.shape
    return m, iE, (iE[:, :, None] * M).reshape(I * D, R), np.einsum("cdr,cd,cds->crs", M, iE, M)


def loglikes(x, gconst, mi, iv, dtype=np.float64):
    x = x.astype(dtype)
    return gconst.astype(dtype)[None, :] + x @ mi.astype(dtype).T - dtype(0.5) * ((x * x) @ iv.astype(dtype).T)


def posteriors(x, gconst, mi, iv, n, ll_scale=1.0, stat_scale=1.0, thr=0.0, dtype=np.float64):
    """-> gauss (F, n), post (F, n), G (F), dense p (F, I), frames with more than n candidates."""
    l = loglikes(x, gconst, mi, iv, dtype) * dtype(ll_scale)
    mx = l.max(1, keepdims=True)
    G = (mx + np.log(np.exp(l - mx).sum(1, keepdims=True, dtype=dtype))).astype(dtype)
    p = (np.exp(l - G) * dtype(stat_scale)).astype(dtype)
    F, I = p.shape
    gauss = np.full((F, n), -1, np.int32)
    post = np.zeros((F, n), dtype)
    over = 0
    for t in range(F):
        cand = [c for c in np.lexsort((np.arange(I), -p[t])) if p[t, c] >= thr]
        over += len(cand) > n
        for k, c in enumerate(cand[:n]):
            gauss[t, k], post[t, k] = c, p[t, c]
    return gauss, post, G[:, 0], p, over


def blocks(T, d):
    return (T + d - 1) // d


def speaker_stats(x, gauss, post, q, d, m):
    """One recording: q (T', K) -> N (K, I), F (K, I, D)."""
    K, (I, D) = q.shape[1], m.shape
    N, Fs = np.zeros((K, I)), np.zeros((K, I, D))
    for t in range(x.shape[0]):
        for c, p in zip(gauss[t], post[t]):
            if 0 <= c < I:
                w = q[t // d] * float(p)
                N[:, c] += w
                Fs[:, c] += w[:, None] * (x[t].astype(np.float64) - m[c])[None, :]
    return N, Fs


def tril_pack(A):
    return A[np.tril_indices(A.shape[0])]


def speaker_update(N, Fs, B, UU):
    """-> a (K, R), W (K, R, R), kl (K), h (K, I, D), g (K, I)."""
    K, I = N.shape
    R = B.shape[1]
    D = B.shape[0] // I
    a, W, kl = np.zeros((K, R)), np.zeros((K, R, R)), np.zeros(K)
    for s in range(K):
        lin = B.T @ Fs[s].reshape(-1)
        Q = np.eye(R) + np.einsum("c,crs->rs", N[s], UU)
        C = np.linalg.inv(Q)
        a[s] = C @ lin
        W[s] = C + np.outer(a[s], a[s])
        kl[s] = 0.5 * (R - np.trace(W[s])) - np.log(np.diag(np.linalg.cholesky(Q))).sum()
    h = (a @ B.T).reshape(K, I, D)
    g = 0.5 * np.einsum("crs,ksr->kc", UU, W)
    return a, W, kl, h, g


def block_loglike(x, gauss, post, d, m, h, g):
    K, I = g.shape
    T = x.shape[0]
    lls = np.zeros((blocks(T, d), K))
    for t in range(T):
        for c, p in zip(gauss[t], post[t]):
            if 0 <= c < I:
                lls[t // d] += float(p) * (h[:, c] @ (x[t].astype(np.float64) - m[c]) - g[:, c])
    return lls


def _lse(v, axis=None):
    mx = np.max(v, axis=axis, keepdims=True)
    mx = np.where(np.isfinite(mx), mx, 0.0)
    return np.squeeze(mx, axis) + np.log(np.sum(np.exp(v - mx), axis=axis)) if axis is not None else float(mx + np.log(np.sum(np.exp(v - mx))))


def forward_backward(lls, sp, lp):
    """Log-domain forward-backward -> q (T', K), tll, sp_new (K)."""
    T, K = lls.shape
    with np.errstate(divide="ignore"):
        lt = np.log(lp * np.eye(K) + (1.0 - lp) * sp[None, :])
        lnl = np.log((1.0 - lp) * sp)
        la = np.zeros((T, K))
        lb = np.zeros((T, K))
        la[0] = np.log(sp) + lls[0]
        for b in range(1, T):
            for j in range(K):
                la[b, j] = lls[b, j] + np.logaddexp.reduce(la[b - 1] + lt[:, j])
        for b in range(T - 2, -1, -1):
            for i in range(K):
                lb[b, i] = np.logaddexp.reduce(lt[i] + lls[b + 1] + lb[b + 1])
        tll = float(np.logaddexp.reduce(la[T - 1]))
        q = np.exp(la + lb - tll)
        acc = q[0].copy()
        for b in range(1, T):
            acc += np.exp(np.logaddexp.reduce(la[b - 1]) + lnl + lls[b] + lb[b] - tll)
    return q, tll, acc / acc.sum()


def brute_force(lls, sp, lp):
    """Path enumeration (tiny T', K): q, tll and sp_new. A step i -> j is one of two exclusive events, the loop (lp, i = j only) or
    the re-entry (1 - lp) sp_j; every (path, choice per step) is enumerated with its probability, and sp_new gathers the posterior
    mass of block 0's state and of the states entered through a re-entry."""
    T, K = lls.shape
    tot, q, ent = 0.0, np.zeros((T, K)), np.zeros(K)
    for path in itertools.product(range(K), repeat=T):
        for loops in itertools.product((False, True), repeat=T - 1):
            pr = sp[path[0]] * np.exp(lls[0, path[0]])
            for b in range(1, T):
                step = (lp if path[b - 1] == path[b] else 0.0) if loops[b - 1] else (1.0 - lp) * sp[path[b]]
                pr *= step * np.exp(lls[b, path[b]])
            tot += pr
            ent[path[0]] += pr
            for b in range(T):
                q[b, path[b]] += pr
                if b and not loops[b - 1]:
                    ent[path[b]] += pr
    return q / tot, float(np.log(tot)), ent / ent.sum()


def init_q(labels, T, d, K):
    q = np.full((blocks(T, d), K), 1.0 / K)
    for b in range(q.shape[0]):
        l = int(labels[b * d])
        if 0 <= l < K:
            q[b] = 0.0
            q[b, l] = 1.0
    return q


def run(x, gauss, post, loglike, m, B, UU, q, sp, d=1, max_iters=10, epsilon=1e-6, loop_prob=0.9, stat_scale=1.0):
    """One recording's loop on supplied posteriors -> q, sp, bound (list)."""
    bound = []
    base = stat_scale * float(np.sum(loglike.astype(np.float64)))
    for it in range(max_iters):
        N, Fs = speaker_stats(x, gauss, post, q, d, m)
        _, _, kl, h, g = speaker_update(N, Fs, B, UU)
        lls = block_loglike(x, gauss, post, d, m, h, g)
        q, tll, sp = forward_backward(lls, sp, loop_prob)
        bound.append(base + tll + kl.sum())
        if it > 0 and bound[-1] - bound[-2] < epsilon:
            break
    return q, sp, bound


def planted(seed, I, D, R, K, T, seg=50, scale=3.0):
    """A recording whose speakers are offsets M_c y_s of a random mixture: -> ubm arrays, M, x (T, D) fp32, truth (T,)."""
    rng = np.random.default_rng(seed)
    (w, mi, iv), M = random_model(rng, I, D, R)
    mean, var = mi.astype(np.float64) / iv, 1.0 / iv.astype(np.float64)
    y = rng.standard_normal((K, R)) * scale
    truth = np.repeat(rng.integers(0, K, (T + seg - 1) // seg), seg)[:T]
    c = rng.choice(I, T, p=w.astype(np.float64) / w.astype(np.float64).sum())
    x = mean[c] + np.einsum("tdr,tr->td", M[c], y[truth]) + rng.standard_normal((T, D)) * np.sqrt(var[c])
    return (w, mi, iv), M, x.astype(np.float32), truth


def gconsts(w, mi, iv):
    w, mi, iv = (a.astype(np.float64) for a in (w, mi, iv))
    D = mi.shape[1]
    return (np.log(w) - 0.5 * D * np.log(2 * np.pi) + 0.5 * np.log(iv).sum(1) - 0.5 * (mi * mi / iv).sum(1)).astype(np.float32)
