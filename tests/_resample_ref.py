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


# ----------------------------------------------------------------------------- what csrc/resample.hip's launcher and kernel choose
# Internal constants of the kernel, mirrored here because the library does not export them (test_augment_paths_cpu.py checks
# the cases of test_gpu_resample_paths.py against them: a changed constant moves the edge, and that module then fails).
RS_THREADS = 256                   # resample.hip:24, threads of a workgroup (the steps of the table's copy loop)
RS_R, RS_J = 4, 4                  # resample.hip:25-26, outputs of one phase per task; taps read ahead per step of the tap loop
RS_LDS_FLOATS = 16384              # resample.hip:28, floats of LDS a workgroup may use
MAX_TAPS, MAX_TABLE_FLOATS, MAX_SPAN = 256, 1 << 16, 12288     # include/ktf_resample.h:43-45


def tile_unit_reach(ou, tile):
    """resample.hip:61: the most units a tile's outputs reach past its first one."""
    return (tile - 1 + ou - 1) // ou


def is_ordered(first, taps, iu):
    """resample.hip:333-342, ktf_rs_resample's `ordered`: first[] and first[] + taps[] ascend with the phase and wrap by at most
    iu. Only then is a tile's span taken from its own first and last phase; otherwise from the lowest first and the highest end."""
    first, end = np.asarray(first, np.int64), np.asarray(first, np.int64) + np.asarray(taps, np.int64)
    if (np.diff(first) < 0).any() or (np.diff(end) < 0).any():
        return False
    return not (first[-1] > first[0] + iu or end[-1] > end[0] + iu)


def lds_budget(first, taps, iu, ou, tile):
    """resample.hip:346 and :368-371 -> dict(span, span_floats, table, floats, wlds): the input span the host allows for a tile, the
    floats it takes with its zero tail, the table's floats in LDS (rows of max_taps | 1), what the launch asks for with the table,
    and whether the table goes to LDS (WLDS) or stays in global memory."""
    first, taps = np.asarray(first, np.int64), np.asarray(taps, np.int64)
    widest = int(taps.max())
    span = tile_unit_reach(ou, tile) * iu + int((first + taps).max() - first.min())
    span_floats = span + widest + 2
    table = ou * (widest | 1)
    floats = span_floats + tile + table
    return dict(span=span, span_floats=span_floats, table=table, floats=floats, wlds=floats <= RS_LDS_FLOATS,
                refused=widest > MAX_TAPS or ou * widest > MAX_TABLE_FLOATS or span > MAX_SPAN)


def tiles_of(m, first, taps, iu, ou, tile):
    """The tiles of a row of m outputs as rs_kernel sees them (resample.hip:158-174) -> [dict(s0, s_end, u_first, u_last, lo, hi,
    parities)]: `parities` is the set of (first[i] - lo) & 1 over the phases (resample.hip:214) -- with an even iu an odd one
    sends that task's first tap through rs_tap before the pair loop."""
    first, taps = np.asarray(first, np.int64), np.asarray(taps, np.int64)
    ordered = is_ordered(first, taps, iu)
    out = []
    for s0 in range(0, m, tile):
        s_end = min(s0 + tile, m) - 1
        u_first, u_last = s0 // ou, s_end // ou
        if ordered:
            i0, i1 = s0 - u_first * ou, s_end - u_last * ou
            lo, hi = first[i0] + u_first * iu, first[i1] + taps[i1] + u_last * iu
            if u_last > u_first:
                lo = min(lo, first[0] + (u_first + 1) * iu)
                hi = max(hi, first[ou - 1] + taps[ou - 1] + (u_last - 1) * iu)
        else:
            lo, hi = first.min() + u_first * iu, (first + taps).max() + u_last * iu
        out.append(dict(s0=s0, s_end=s_end, u_first=u_first, u_last=u_last, lo=int(lo), hi=int(hi),
                        parities={int(v) for v in (first - lo) & 1}))
    return out


def rows_for(iu, ou, tile, short=5):
    """The row lengths of test_gpu_resample.py's batch for a plan of iu -> ou samples per unit: the fewest input samples that give
    at least 0, 1, 2, tile - 1, tile, tile + 1 and 2 tile + 17 outputs (rule 3: m = ceil(n ou / iu)), and one of `short` samples."""
    ns = []
    for m in (0, 1, 2, tile - 1, tile, tile + 1, 2 * tile + 17):
        n = 0 if m == 0 else max(1, (m - 1) * iu // ou)
        while m and -(-n * ou // iu) < m:
            n += 1
        ns.append(n)
    return ns + [short]


def table_copy_steps(max_taps, ou):
    """resample.hip:195-202, the WLDS copy loop: (di, dj) of one step of RS_THREADS table elements, and the steps thread 0 takes."""
    di = RS_THREADS // max_taps
    dj = RS_THREADS - di * max_taps
    return di, dj, -(-ou * max_taps // RS_THREADS)


# The plans of test_gpu_resample_paths.py: (fi, fo, zeros, cutoff or None for the default). Pure data; the CPU module proves what
# each reaches.
GLOBAL_TABLE_PLANS = [(44100, 16000, 16, None), (48000, 44100, 48, None), (8000, 11025, 16, None), (44100, 8000, 12, None)]
WIDE_OU_PLANS = [(16000, 44100, 6, None), (8000, 44100, 6, None), (7, 1031, 6, None)]
FEW_TAPS_PLANS = [(1, 2, 1, 0.5), (2, 3, 1, 1.0), (3, 2, 1, 1.0)]          # the cutoff at the Nyquist frequency: 2 to 4 taps
# 48000 -> 8000 with 21 zeros: 255 taps in its one phase (22 zeros: 267, refused). 3 -> 2 with 64 zeros and cutoff 0.7515:
# 3 ww = 127.745, so phase 0 has 2 floor(3 ww) + 1 = 255 taps and phase 1 floor(1.5 + 3 ww) - ceil(1.5 - 3 ww) + 1 = 256
MOST_TAPS_PLANS = [(48000, 8000, 21, None), (3, 2, 64, 0.7515)]


def one_tap_plan():
    """A hand-made plan of one tap per phase (max_taps = 1): 300 -> 301, phase i reads sample floor(300 i / 301) of its unit with
    its own weight. An even iu, more phases than threads. -> (iu, ou, first, taps, w (ou, 1))"""
    iu, ou = 300, 301
    i = np.arange(ou)
    first = (i * iu // ou).astype(np.int32)
    w = (0.5625 + (i % 7) / 8.0 - (i % 3 == 0)).astype(np.float32).reshape(ou, 1)      # 14 distinct weights, none 0
    return iu, ou, first, np.ones(ou, np.int32), w


def unordered_plan(first, taps, w, phase, by=3):
    """The plan with phase `phase` starting `by` samples earlier under `by` leading zero weights: the same sums (the added products
    are exact zeros), but first[] no longer ascends. -> (first, taps, w (ou, widest))"""
    first, taps = np.array(first, np.int32), np.array(taps, np.int32)
    first[phase] -= by
    taps[phase] += by
    out = np.zeros((first.size, int(taps.max())), np.float32)
    for i in range(first.size):
        k = by if i == phase else 0
        out[i, k:taps[i]] = np.asarray(w[i], np.float32)[:taps[i] - k]
    return first, taps, out
