"""NumPy restatement of Kaldi's `agglomerative-cluster` (AgglomerativeClusterer, single pass): the yardstick of
ktf.diarization.agglomerative_cluster (the reference ships no clustering code and no clustering golden).

ahc_kaldi is literal (a heap of (avg, lo_id, hi_id), an active set, pairs dropped when a merge is refused) and slow;
ahc_fast keeps a cached best partner per row, is fast enough for n = 5000 in seconds, and must give the same labels.
Both take one (n, n) block and return (labels 1 .. K (n,) int32, K). All arithmetic is in the block's dtype."""

import heapq
import math

import numpy as np


def params(n, dtype, threshold=None, num_speakers=None, max_spk_fraction=1.0):
    """(threshold, min_clusters, max_size) as Kaldi's binary sets them in its two modes."""
    dt = np.dtype(dtype).type
    if num_speakers is None:
        thr, minc = dt(0.0 if threshold is None else threshold), 1
    else:
        thr, minc = dt(np.finfo(dt).max), int(num_speakers)
    max_size = int(math.ceil(np.float32(n) * np.float32(max_spk_fraction)))
    return thr, minc, max_size


def costs(scores, read_costs=False):
    s = np.asarray(scores)
    assert s.ndim == 2 and s.shape[0] == s.shape[1] and s.dtype in (np.float32, np.float64), (s.shape, s.dtype)
    return s.copy() if read_costs else -s


def _labels(ids_of_rows, final_ids):
    rank = {c: r + 1 for r, c in enumerate(sorted(final_ids))}
    return np.array([rank[c] for c in ids_of_rows], np.int32), len(final_ids)


def ahc_kaldi(scores, threshold=None, num_speakers=None, max_spk_fraction=1.0, read_costs=False):
    C = costs(scores, read_costs)
    dt = C.dtype.type
    n = C.shape[0]
    thr, minc, max_size = params(n, dt, threshold, num_speakers, max_spk_fraction)
    cost = {}                                  # (lo_id, hi_id) -> Sigma
    size = {i + 1: 1 for i in range(n)}
    members = {i + 1: [i] for i in range(n)}
    active = set(size)
    heap = []
    for i in range(n):
        for j in range(i + 1, n):
            c = dt(C[i, j])
            cost[(i + 1, j + 1)] = c
            if c <= thr:
                heap.append((float(c), i + 1, j + 1))
    heapq.heapify(heap)
    next_id = n + 1
    while len(active) > minc and heap:
        avg, a, b = heapq.heappop(heap)
        if a not in active or b not in active:
            continue
        if size[a] + size[b] > max_size:
            continue                           # dropped for good: sizes only grow
        new = next_id
        next_id += 1
        active.discard(a)
        active.discard(b)
        size[new] = size[a] + size[b]
        members[new] = members.pop(a) + members.pop(b)
        for k in sorted(active):
            c = dt(cost[(min(k, a), max(k, a))] + cost[(min(k, b), max(k, b))])
            cost[(k, new)] = c
            avg_k = c / dt(size[k] * size[new])
            if avg_k <= thr:
                heapq.heappush(heap, (float(avg_k), k, new))
        active.add(new)
    of_row = np.empty(n, np.int64)
    for c in active:
        of_row[members[c]] = c
    return _labels(of_row, active)


def ahc_fast(scores, threshold=None, num_speakers=None, max_spk_fraction=1.0, read_costs=False):
    C = costs(scores, read_costs)
    dt = C.dtype.type
    n = C.shape[0]
    thr, minc, max_size = params(n, dt, threshold, num_speakers, max_spk_fraction)
    iu = np.triu_indices(n, 1)
    sig = np.zeros((n, n), C.dtype)
    sig[iu] = C[iu]
    sig.T[iu] = C[iu]
    size = np.ones(n, np.int64)
    ids = np.arange(1, n + 1, dtype=np.int64)
    alive = np.ones(n, bool)
    par = np.arange(n)
    best_v = np.full(n, np.inf, C.dtype)
    best_j = np.full(n, -1, np.int64)
    pos = np.arange(n)

    def rescan(rows):
        """Best eligible (avg, key) partner of each of `rows`, keys lo_id << 16 | hi_id."""
        rows = np.asarray(rows, np.int64)
        if rows.size == 0:
            return
        with np.errstate(invalid="ignore", divide="ignore"):
            avg = sig[rows] / (size[rows, None] * size[None, :]).astype(C.dtype)
        ok = (avg <= thr) & alive[None, :] & (pos[None, :] != rows[:, None]) & (size[rows, None] + size[None, :] <= max_size)
        key = np.minimum(ids[rows, None], ids[None, :]) * 65536 + np.maximum(ids[rows, None], ids[None, :])
        v = np.where(ok, avg, np.inf)
        vmin = v.min(axis=1)
        tie = ok & (v == vmin[:, None])
        j = np.where(tie, key, np.iinfo(np.int64).max).argmin(axis=1)
        has = ok.any(axis=1)
        best_v[rows] = np.where(has, vmin, np.inf)
        best_j[rows] = np.where(has, j, -1)

    for start in range(0, n, 256):
        rescan(np.arange(start, min(n, start + 256)))
    active, next_id = n, n + 1
    while active > minc:
        cand = np.nonzero(alive & (best_j >= 0))[0]
        if cand.size == 0:
            break
        v = best_v[cand]
        vmin = v.min()
        t = cand[v == vmin]
        key = np.minimum(ids[t], ids[best_j[t]]) * 65536 + np.maximum(ids[t], ids[best_j[t]])
        p = t[key.argmin()]
        q = best_j[p]
        a, b = (p, q) if ids[p] < ids[q] else (q, p)
        sz = size[a] + size[b]
        others = np.nonzero(alive)[0]
        others = others[(others != a) & (others != b)]
        c = sig[a, others] + sig[b, others]
        sig[a, others] = c
        sig[others, a] = c
        alive[b] = False
        size[a], size[b] = sz, 0
        ids[a] = next_id
        par[b] = a
        with np.errstate(invalid="ignore", divide="ignore"):
            avg = c / (size[others] * sz).astype(C.dtype)
        ok = (avg <= thr) & (size[others] + sz <= max_size)
        stale = (best_j[others] == a) | (best_j[others] == b)
        # rows that keep their best: the new pair (k, new) has key id_k << 16 | next_id, above any other key with the same lo id
        keep = others[~stale]
        kv, kok = avg[~stale], ok[~stale]
        cur_j = best_j[keep]
        cur_key = np.where(cur_j >= 0, np.minimum(ids[keep], ids[np.maximum(cur_j, 0)]) * 65536 +
                           np.maximum(ids[keep], ids[np.maximum(cur_j, 0)]), np.iinfo(np.int64).max)
        new_key = ids[keep] * 65536 + next_id
        better = kok & ((cur_j < 0) | (kv < best_v[keep]) | ((kv == best_v[keep]) & (new_key < cur_key)))
        best_v[keep[better]] = kv[better]
        best_j[keep[better]] = a
        # the new cluster's own best
        if ok.any():
            vv = np.where(ok, avg, np.inf)
            m = vv.min()
            tt = ok & (vv == m)
            kk = np.where(tt, ids[others] * 65536 + next_id, np.iinfo(np.int64).max)
            best_v[a], best_j[a] = m, others[kk.argmin()]
        else:
            best_v[a], best_j[a] = np.inf, -1
        best_j[b] = -1
        rescan(others[stale])
        active -= 1
        next_id += 1
    root = par.copy()
    while True:
        nxt = root[root]
        if np.array_equal(nxt, root):
            break
        root = nxt
    return _labels(ids[root], ids[alive])
