"""Cohort statistics for score normalisation at a deployment shape: R = 8192 vectors against a cohort of
C = 10000, the top N = 400 per row, D = 128, fp64, both roles. `PLDA.cohort_stats` (scores formed chunk by chunk in a bounded
workspace, radix select per row) against what a user could write before it existed: `PLDA.score` into the full matrix, then
`torch.topk` and mean / population std. Both are timed on the same GPU in alternating regions after a warm-up of both, each region
`--reps` calls between two device events; the figures are the median / min / max over `--regions` regions, the ratio is the
baseline's median over the new path's, and `new_wins` says whether the new path's slowest region still beats the baseline's
fastest. Peak device memory above what is allocated before the call is reported for both. Before timing, the two are compared
(the selected values are the same multiset; the baseline sums in another order). The new path's two stages alone follow (the score
block of one chunk, the selection on it); one JSON line per role.

    python tools/bench_snorm.py [--R 8192] [--C 10000] [--N 400] [--D 128] [--dtype f64] [--limit-mb 1024 64] [--reps 40] [--regions 5]"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-tflite_amd"))
import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import ops  # noqa: E402


def region(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def stats(v):
    return [float(np.median(v)), float(min(v)), float(max(v))]


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=8192)
    ap.add_argument("--C", type=int, default=10000)
    ap.add_argument("--N", type=int, default=400)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64")
    ap.add_argument("--limit-mb", type=int, nargs="+", default=[1024, 64])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    R, Cn, N, D = a.R, a.C, a.N, a.D
    dtype = torch.float64 if a.dtype == "f64" else torch.float32
    rng = np.random.default_rng(1)
    T = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
    plda = ktf.layers.PLDA(D, rng.standard_normal(D) * 0.1, T, np.sort(rng.uniform(0.05, 30.0, D))[::-1].copy(), dtype=dtype)
    g = torch.Generator(device=dev).manual_seed(2)
    centroids = torch.randn((Cn // 8 + 1, D), dtype=torch.float64, device=dev, generator=g) * 2.0

    def vectors(n):
        pick = torch.randint(0, centroids.shape[0], (n,), device=dev, generator=g)
        return centroids[pick] + torch.randn((n, D), dtype=torch.float64, device=dev, generator=g)

    n_rows = torch.randint(1, 51, (R,), device=dev, generator=g).to(dtype)
    n_coh = torch.randint(1, 51, (Cn,), device=dev, generator=g).to(dtype)
    for role in ("test", "enroll"):
        if role == "test":
            rows, coh, n = plda.transform(vectors(R)), plda.transform(vectors(Cn), num_examples=n_coh), n_coh
        else:
            rows, coh, n = plda.transform(vectors(R), num_examples=n_rows), plda.transform(vectors(Cn)), n_rows

        def baseline():
            if role == "test":
                top = torch.topk(plda.score(rows, coh, enroll_num_examples=n), N, dim=1).values.to(torch.float64)
                return top.mean(1), top.std(1, unbiased=False)
            top = torch.topk(plda.score(coh, rows, enroll_num_examples=n), N, dim=0).values.to(torch.float64)
            return top.mean(0), top.std(0, unbiased=False)

        res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), role=role, R=R, C=Cn, N=N, D=D, dtype=a.dtype, reps=a.reps,
                   regions=a.regions, full_matrix_mb=R * Cn * rows.element_size() / 2 ** 20)
        want = baseline()
        for mb in a.limit_mb:
            def new():
                return plda.cohort_stats(rows, coh, top_n=N, role=role, num_examples=n, workspace_limit=mb << 20)

            got = new()                                             # (the warm-up of both, too)
            tag = f"limit_{mb}mb"
            res[tag] = cur = dict(rows_per_chunk_at_most=max(1, (mb << 20) // (Cn * rows.element_size())))
            cur["mean_diff"] = float((got[0] - want[0]).abs().max())
            cur["std_diff"] = float((got[1] - want[1]).abs().max())
            cur["new_peak_mb"], cur["baseline_peak_mb"] = peak_mb(new), peak_mb(baseline)
            tn, tb = [], []
            for _ in range(a.regions):                              # alternating: both see the same neighbours on the machine
                tn.append(region(new, a.reps))
                tb.append(region(baseline, a.reps))
            cur["new_ms"], cur["baseline_ms"] = stats(tn), stats(tb)
            cur["baseline_over_new"] = cur["baseline_ms"][0] / cur["new_ms"][0]
            cur["new_wins"] = max(tn) < min(tb)
        # the stages of one chunk of at most 1024 rows: its score block, and the selection on a block of that size
        rc = min(R, 1024)
        blk = plda.score(rows[:rc], coh, enroll_num_examples=n) if role == "test" else plda.score(coh, rows[:rc], enroll_num_examples=n[:rc]).t().contiguous()
        stage = dict(score=(lambda: plda.score(rows[:rc], coh, enroll_num_examples=n)) if role == "test" else
                     (lambda: plda.score(coh, rows[:rc], enroll_num_examples=n[:rc])), select=lambda: ops.topn_stats(blk, N),
                     select_all=lambda: ops.topn_stats(blk, None),
                     topk=lambda: torch.topk(blk, N, dim=1))
        for k, fn in stage.items():
            fn()
            torch.cuda.synchronize()
            res[f"{k}_{rc}_rows_ms"] = stats([region(fn, a.reps) for _ in range(a.regions)])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
