"""Times PLDA back-end training (ktf.training) on one GPU at a recipe's size: N x-vectors of dimension D from S speakers with ragged
counts (default sitw's train_combined_200k: 200 k x 512, 7 k speakers). Prints one JSON line: the wall time of compute_lda and of
compute_plda (10 EM iterations), the split of compute_plda between GPU kernels and host factorisations (one instrumented run that
synchronises around every GPU call), the Gram kernel's rate against the fp64 peak, and the host NumPy oracle (tests/_plda_train_ref.py)
on the same data as the baseline (its threads are the BLAS library's; OMP_NUM_THREADS sets them).

    python tools/plda_train_time.py [--N 200000] [--D 512] [--S 7000] [--reps 2] [--no-host]
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kaldi-tflite_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import _plda_train_ref as R                                     # noqa: E402
from kaldi_tflite_amd import _lib as L, ops, training           # noqa: E402

FP64_PEAK = 78.6e12            # MI355X published fp64 rate (vector FMA and MFMA alike), FLOP/s


def counts(rng, N, S):
    """Ragged speaker sizes summing to N: log-normal around N / S, at least 2 (Kaldi's recipes drop speakers with fewer)."""
    c = np.maximum(2, np.round(rng.lognormal(np.log(N / S) - 0.32, 0.8, S))).astype(np.int64)
    while c.sum() != N:
        d = N - c.sum()
        i = rng.integers(0, S, abs(d))
        np.add.at(c, i, np.sign(d))
        c = np.maximum(c, 2)
    return c


def synced(fn, acc, key):
    def run(*a, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*a, **k)
        torch.cuda.synchronize()
        acc[key] = acc.get(key, 0.0) + time.perf_counter() - t0
        return out
    return run


def timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200000)
    ap.add_argument("--D", type=int, default=512)
    ap.add_argument("--S", type=int, default=7000)
    ap.add_argument("--lda-dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    rng = np.random.default_rng(1)
    c = counts(rng, a.N, a.S)
    off = np.concatenate([[0], np.cumsum(c)])
    spk = (off, rng.permutation(a.N))                               # speakers' rows scattered over x, as in a real utt list
    g = torch.Generator(device=dev).manual_seed(2)
    y = torch.randn((a.S, a.D), generator=g, device=dev) * 2.0
    owner = torch.as_tensor(np.repeat(np.arange(a.S), c), device=dev)
    x = torch.empty((a.N, a.D), device=dev)
    x[torch.as_tensor(spk[1], device=dev)] = y[owner] + torch.randn((a.N, a.D), generator=g, device=dev)
    training.compute_lda(x[:4096], [np.arange(0, 2048), np.arange(2048, 4096)], 8)          # warm-up (code objects, allocator)
    t_lda, _ = timed(lambda: training.compute_lda(x, spk, a.lda_dim), a.reps)
    t_plda, plda = timed(lambda: training.compute_plda(x, spk), a.reps)

    # one instrumented compute_plda: every GPU call synchronised, every host factorisation timed
    acc = {}
    saved = {k: getattr(ops, k) for k in ("train_gram", "train_mean", "train_class_means", "plda_em_project")}
    saved_h = {k: getattr(training, k) for k in ("plda_diagonalize",)}
    for k, f in saved.items():
        setattr(ops, k, synced(f, acc, "gpu_" + k))
    training.plda_diagonalize = synced(saved_h["plda_diagonalize"], acc, "host_diagonalize")
    try:
        t_inst, _ = timed(lambda: training.compute_plda(x, spk), 1)
    finally:
        for k, f in saved.items():
            setattr(ops, k, f)
        training.plda_diagonalize = saved_h["plda_diagonalize"]

    # the Gram kernel over all N rows (ktf_train_gram_f32: the D x D scatter of compute_lda / compute_plda)
    ws = ops.train_workspace(a.N, a.D, dev)
    t_gram, _ = timed(lambda: ops.train_gram(x, ws), max(a.reps, 3))
    flop = float(a.N) * a.D * (a.D + 1)                             # one multiply-add per (i <= j) element and row
    res = {
        "build_id": L.load().ktf_build_id().decode(), "device": torch.cuda.get_device_name(dev),
        "N": a.N, "D": a.D, "S": a.S, "lda_dim": a.lda_dim, "count_min": int(c.min()), "count_max": int(c.max()),
        "distinct_counts": int(np.unique(c).size),
        "compute_lda_s": round(t_lda, 4), "compute_plda_s": round(t_plda, 4),
        "plda_instrumented_s": round(t_inst, 4), **{k + "_s": round(v, 4) for k, v in sorted(acc.items())},
        "gram_N_ms": round(t_gram * 1e3, 3), "gram_tflops": round(flop / t_gram / 1e12, 2),
        "gram_fraction_of_fp64_peak": round(flop / t_gram / FP64_PEAK, 3),
        "psi_top": float(plda.psi[0]), "finite": bool(np.isfinite(plda.transformMat).all()),
    }
    if not a.no_host:
        xh = x.cpu().numpy().astype(np.float64)
        lists = np.split(spk[1], off[1:-1])
        t0 = time.perf_counter()
        R.compute_lda(xh, lists, a.lda_dim)
        res["host_oracle_lda_s"] = round(time.perf_counter() - t0, 2)
        t0 = time.perf_counter()
        R.compute_plda(xh, lists)
        res["host_oracle_plda_s"] = round(time.perf_counter() - t0, 2)
        res["host_threads"] = os.environ.get("OMP_NUM_THREADS")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
