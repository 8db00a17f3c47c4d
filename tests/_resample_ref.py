"""Sample-rate conversion in fp64 NumPy: rules 1 to 4 of include/ktf_resample.h as loops (the oracle of test_resample_cpu.py and
test_gpu_resample.py). Every operation is IEEE fp64 in the order the header writes it."""

import math

import numpy as np


def default_cutoff(fi, fo):
    return 0.99 * 0.5 * min(fi, fo)


def plan(fi, fo, cutoff=None, zeros=6):
    """-> (iu, ou, first [ou ints], taps [ou ints], w [ou fp64 arrays of taps[i] weights])."""
    cutoff = default_cutoff(fi, fo) if cutoff is None else float(cutoff)
    g = math.gcd(fi, fo)
    iu, ou = fi // g, fo // g
    ww = zeros / (2.0 * cutoff)
    two_pi_cutoff = 2.0 * math.pi * cutoff
    first, taps, w = [], [], []
    for i in range(ou):
        t = i / fo
        lo = math.ceil((t - ww) * fi)
        hi = math.floor((t + ww) * fi)
        row = np.zeros(hi - lo + 1, np.float64)
        for j in range(hi - lo + 1):
            d = (lo + j) / fi - t
            win = 0.5 * (1.0 + math.cos(two_pi_cutoff / zeros * d)) if abs(d) < ww else 0.0
            f = math.sin(two_pi_cutoff * d) / (math.pi * d) if d != 0.0 else 2.0 * cutoff
            row[j] = f * win / fi
        first.append(lo)
        taps.append(hi - lo + 1)
        w.append(row)
    return iu, ou, first, taps, w


def num_out(n, fi, fo):
    if n == 0:
        return 0
    tick = fi * fo // math.gcd(fi, fo)
    span = n * (tick // fi)
    last = span // (tick // fo)
    if last * (tick // fo) == span:
        last -= 1
    return last + 1


def resample64(x, first, taps, w32, iu, ou, m):
    """Rule 4 on the fp32 samples x with fp32 weights w32[i][j] -> (the fp64 sums y (m,), sum_j |w x| per output (m,)): each
    product exact in fp64 (24 x 24 bits), added in ascending j. The loop runs over j for all outputs at once; an output whose
    phase has fewer taps, or whose sample lies outside [0, n), adds an exact 0."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n = x.size
    s = np.arange(m)
    u, i = s // ou, s % ou
    k0 = np.asarray(first, np.int64)[i] + u * iu
    nt = np.asarray(taps, np.int64)
    wide = int(nt.max()) if m else 0
    table = np.zeros((ou, wide), np.float64)
    for p in range(ou):
        table[p, :min(nt[p], wide)] = np.asarray(w32[p], np.float32)[:min(nt[p], wide)].astype(np.float64)
    y, mag = np.zeros(m, np.float64), np.zeros(m, np.float64)
    for j in range(wide):
        k = k0 + j
        ok = (k >= 0) & (k < n) & (j < nt[i])
        prod = np.where(ok, table[i, j] * x[np.clip(k, 0, max(n - 1, 0))] if n else 0.0, 0.0)
        y = y + prod
        mag = mag + np.abs(prod)
    return y, mag


def to_int16(v):
    return np.clip(np.rint(np.asarray(v, np.float64)), -32768, 32767).astype(np.int16)
