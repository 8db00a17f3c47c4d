"""fp64 NumPy oracle of include/ktf_norm.h: ReLU + batch normalisation, forward and backward, as plain loops over the valid rows
(b, t < len_b), one row of D features at a time. Next to every result it returns the magnitudes the tests' bounds are made of."""

import numpy as np


def _lens(lens, B, T):
    if lens is None:
        return [T] * B
    return [min(max(int(n), 0), T) for n in lens]


def _act(row, relu):
    # max(z, 0) with -0.0 -> +0.0, as the kernels take it
    return np.where(row > 0, row, 0.0) if relu else row


def forward(z, lens, relu, training, gamma, moving_mean, moving_var, momentum, eps):
    """z (B, T, D) (any columns beyond D already cut off), gamma / moving_* (D,). Returns a dict: y (B, T, D) fp64 unrounded, mean,
    invstd, n, moving_mean / moving_var after the call (fp64, unrounded: the fp32 library rounds them once), y_mag = (|a| + |mean|)
    * |gamma * invstd| per element (zero on invalid rows)."""
    z = np.asarray(z, dtype=np.float64)
    gamma = np.asarray(gamma, dtype=np.float64)
    mm, mv = np.asarray(moving_mean, dtype=np.float64).copy(), np.asarray(moving_var, dtype=np.float64).copy()
    B, T, D = z.shape
    lens = _lens(lens, B, T)
    n = sum(lens)
    y, mag = np.zeros((B, T, D)), np.zeros((B, T, D))
    if n == 0:
        return dict(y=y, mean=np.zeros(D), invstd=np.zeros(D), n=0, moving_mean=mm, moving_var=mv, y_mag=mag)
    if training:
        S1, S2 = np.zeros(D), np.zeros(D)
        for b in range(B):
            for t in range(lens[b]):
                a = _act(z[b, t], relu)
                S1 += a
                S2 += a * a
        mean = S1 / n
        var = np.maximum(S2 / n - mean * mean, 0.0)
        mm = mm * momentum + mean * (1.0 - momentum)
        mv = mv * momentum + var * (1.0 - momentum)
    else:
        mean, var = mm.copy(), mv.copy()
    invstd = 1.0 / np.sqrt(var + eps)
    for b in range(B):
        for t in range(lens[b]):
            a = _act(z[b, t], relu)
            y[b, t] = ((a - mean) * gamma) * invstd
            mag[b, t] = (np.abs(a) + np.abs(mean)) * np.abs(gamma * invstd)
    return dict(y=y, mean=mean, invstd=invstd, n=n, moving_mean=mm, moving_var=mv, y_mag=mag)


def backward(gy, z, lens, relu, training, gamma, mean, invstd):
    """gy, z (B, T, D); mean / invstd as forward() returned them. Returns a dict: dz (B, T, D) and dgamma (D,) fp64 unrounded, s1, s2,
    n, dz_mag = |gamma * invstd| * (|gy| + |s1 / n| + |ahat * s2 / n|) per element where dz is not forced to zero (training; |gamma *
    invstd * gy| in evaluation), dgamma_abs = sum |gy * ahat|."""
    gy, z = np.asarray(gy, dtype=np.float64), np.asarray(z, dtype=np.float64)
    gamma = np.asarray(gamma, dtype=np.float64)
    B, T, D = z.shape
    lens = _lens(lens, B, T)
    n = sum(lens)
    s1, s2, sabs = np.zeros(D), np.zeros(D), np.zeros(D)
    for b in range(B):
        for t in range(lens[b]):
            ahat = (_act(z[b, t], relu) - mean) * invstd
            s1 += gy[b, t]
            s2 += gy[b, t] * ahat
            sabs += np.abs(gy[b, t] * ahat)
    dz, mag = np.zeros((B, T, D)), np.zeros((B, T, D))
    k = gamma * invstd
    for b in range(B):
        for t in range(lens[b]):
            ahat = (_act(z[b, t], relu) - mean) * invstd
            if training:
                row = k * ((gy[b, t] - s1 / n) - ahat * (s2 / n))
                m = np.abs(k) * (np.abs(gy[b, t]) + np.abs(s1 / n) + np.abs(ahat * (s2 / n)))
            else:
                row = k * gy[b, t]
                m = np.abs(row)
            on = z[b, t] > 0 if relu else np.ones(D, bool)
            dz[b, t] = np.where(on, row, 0.0)
            mag[b, t] = np.where(on, m, 0.0)
    return dict(dz=dz, dgamma=s2.copy(), s1=s1, s2=s2, n=n, dz_mag=mag, dgamma_abs=sabs)
