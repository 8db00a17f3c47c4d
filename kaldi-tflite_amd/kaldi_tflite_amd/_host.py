"""Host-side helpers the back-end modules share: argument checks, host copies, per-device constants and chunking under a
workspace limit. No kernel is launched from here."""

import numbers

import numpy as np
import torch


def host(a, dtype=None):
    """A tensor (on any device) or an array-like -> a NumPy array."""
    return np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=dtype)


def is_real(v):
    return isinstance(v, numbers.Real) and not isinstance(v, (bool, np.bool_))


def is_int(v):
    return isinstance(v, (numbers.Integral, np.integer)) and not isinstance(v, (bool, np.bool_))


def per_device(obj, device, make):
    """One device-resident constant set per (object, device), made by make() on first use: an object used on a second GPU must not
    hand kernels pointers into the first one's memory."""
    cache = obj.__dict__.setdefault("_dev_cache", {})
    key = str(device)
    if key not in cache:
        cache[key] = make()
    return cache[key]


def max_under(nbytes, limit, hi):
    """The largest count in [1, hi] for which nbytes(count) <= limit (nbytes ascending); 1 when none is."""
    lo = 1
    if nbytes(hi) <= limit:
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if nbytes(mid) <= limit:
            lo = mid
        else:
            hi = mid
    return lo


def chunks(total, step):
    """[(lo, hi)] covering range(total) in pieces of at most `step`."""
    return [(lo, min(total, lo + step)) for lo in range(0, total, step)]
