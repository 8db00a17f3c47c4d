"""Plain fp64 NumPy oracle of VBx: the VB-HMM over window x-vectors in the PLDA-transformed space, one recording
at a time, the HMM being _vb_ref.forward_backward. Every stage is a function of its own; `run` is the loop."""

import numpy as np

import _vb_ref as V


def prepare(X, phi):
    """-> rho (T, D), G (T)."""
    D = X.shape[1]
    return X * np.sqrt(phi)[None, :], -0.5 * ((X * X).sum(1) + D * np.log(2 * np.pi))


def speaker_update(gamma, rho, phi, fafb):
    """-> alpha (K, D), invL (K, D), c (K), kl (K)."""
    Nk = gamma.sum(0)
    invL = 1.0 / (1.0 + fafb * Nk[:, None] * phi[None, :])
    alpha = fafb * invL * (gamma.T @ rho)
    c = 0.5 * ((invL + alpha ** 2) * phi[None, :]).sum(1)
    kl = 0.5 * (np.log(invL) - invL - alpha ** 2 + 1.0).sum(1)
    return alpha, invL, c, kl


def loglike(rho, G, alpha, c, Fa):
    return Fa * (rho @ alpha.T - c[None, :] + G[:, None])


def run(X, phi, gamma, pi, loop_prob=0.99, Fa=0.3, Fb=17.0, max_iters=40, epsilon=1e-6):
    """One recording -> gamma (T, K), pi (K), elbo (list)."""
    rho, G = prepare(X, phi)
    elbo = []
    for ii in range(max_iters):
        alpha, _, c, kl = speaker_update(gamma, rho, phi, Fa / Fb)
        gamma, tll, pi = V.forward_backward(loglike(rho, G, alpha, c, Fa), pi, loop_prob)
        elbo.append(tll + Fb * sum(float(v) for v in kl))       # in speaker order: a padded speaker adds an exact 0
        if ii > 0 and elbo[-1] - elbo[-2] < epsilon:
            break
    return gamma, pi, elbo


def init(labels, K, smoothing=5.0):
    """gamma0 = softmax(smoothing * onehot) over the K_r distinct labels (ascending) in the first K_r of K columns, pi0 = 1 / K_r
    there; both 0 on the other columns. Needs K_r <= K."""
    ids = np.unique(labels)
    Kr = ids.size
    assert Kr <= K
    z = np.zeros((len(labels), Kr))
    z[np.arange(len(labels)), np.searchsorted(ids, labels)] = smoothing
    e = np.exp(z)
    gamma, pi = np.zeros((len(labels), K)), np.zeros(K)
    gamma[:, :Kr] = e / e.sum(1, keepdims=True)
    pi[:Kr] = 1.0 / Kr
    return gamma, pi


def labels_of(gamma):
    """arg-max (ties to the lower index) renumbered to 1 .. K' in ascending column order -> labels, K'."""
    arg = gamma.argmax(1)
    cols = np.unique(arg)
    return np.searchsorted(cols, arg) + 1, cols.size


def planted(seed, D, K, T, seg):
    """phi (D,) sorted descending in [0.05, 8], speaker means ~ N(0, phi), unit within-class noise, segments of `seg` windows of one
    speaker -> phi, X (T, D), truth (T,)."""
    rng = np.random.default_rng(seed)
    phi = np.sort(rng.uniform(0.05, 8.0, D))[::-1].copy()
    means = rng.standard_normal((K, D)) * np.sqrt(phi)[None, :]
    truth = np.repeat(rng.integers(0, K, (T + seg - 1) // seg), seg)[:T]
    return phi, means[truth] + rng.standard_normal((T, D)), truth


def noisy_start(truth, K0, share, seed):
    """The true labels modulo K0 with `share` of them replaced at random."""
    rng = np.random.default_rng(seed)
    lab = truth % K0
    bad = rng.random(truth.size) < share
    lab[bad] = rng.integers(0, K0, int(bad.sum()))
    return lab
