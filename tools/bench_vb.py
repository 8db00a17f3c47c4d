"""Stage times of the VB-HMM resegmentation on synthetic data: ms per iteration by stage, for one recording and
a batch, at the sizes Kaldi's callhome recipe runs (T = 60 000 frames, D = 60, I = 2048, R = 128 / 400, K = 10, downsample 1 / 25).
Each figure is the median of `--regions` regions of `--reps` calls after a warm-up, timed with device events; the build id of the
library is printed with them. The forward-backward is timed in both forms: the chunked scan the package runs, and the serial form
(ktf_vb_forward_backward_serial: one wave per recording walks every block; nothing else calls it). `fb_spread` is the largest
(max - min) / median over the regions of the two, and `fb_chunked_wins` says whether the chunked scan's slowest region still beats
the serial form's fastest one: the scan is worth keeping only where it does at T' = 60 000 (downsample 1).

    python tools/bench_vb.py [--N 1 16] [--R 128 400] [--downsample 1 25] [--T 60000] [--I 2048] [--D 60] [--K 10] [--n 32]"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-tflite_amd"))
from kaldi_tflite_amd import ops  # noqa: E402


def timed(fn, reps, regions, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--R", type=int, nargs="+", default=[128, 400])
    ap.add_argument("--downsample", type=int, nargs="+", default=[1, 25])
    ap.add_argument("--T", type=int, default=60000)
    ap.add_argument("--I", type=int, default=2048)
    ap.add_argument("--D", type=int, default=60)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(1)
    I, D, K, n = a.I, a.D, a.K, a.n
    for R in a.R:
        P = R * (R + 1) // 2
        Bm = torch.randn((I * D, R), dtype=torch.float64, device=dev, generator=g) * 0.05
        U = torch.rand((I, P), dtype=torch.float64, device=dev, generator=g) * 1e-3
        means = torch.randn((I, D), dtype=torch.float64, device=dev, generator=g)
        for N in a.N:
            F = N * a.T
            x = torch.randn((F, D), device=dev, generator=g)
            gauss = torch.randint(0, I, (F, n), device=dev, generator=g, dtype=torch.int32)
            post = torch.rand((F, n), device=dev, generator=g) * 0.02
            off = torch.arange(N + 1, dtype=torch.int32, device=dev) * a.T
            start, pairs = ops.vb_bucket(gauss, I)
            for ds in a.downsample:
                Tb = (a.T + ds - 1) // ds
                boff = torch.arange(N + 1, dtype=torch.int32, device=dev) * Tb
                q = torch.softmax(torch.randn((N * Tb, K), dtype=torch.float64, device=dev, generator=g), 1)
                sp = torch.full((N, K), 1.0 / K, dtype=torch.float64, device=dev)
                st = ops.vb_speaker_stats(x, off, boff, ds, post, start, pairs, means, q)
                up = ops.vb_speaker_update(*st, Bm, U)
                lls = ops.vb_block_loglike(x, off, boff, ds, N * Tb, gauss, post, means, up[3], up[4], K)
                res = dict(build=ops.build_id(), N=N, T=a.T, D=D, I=I, R=R, K=K, n=n, downsample=ds, reps=a.reps, regions=a.regions)
                res["stats_ms"] = timed(lambda: ops.vb_speaker_stats(x, off, boff, ds, post, start, pairs, means, q), a.reps, a.regions)
                res["update_ms"] = timed(lambda: ops.vb_speaker_update(*st, Bm, U), a.reps, a.regions)
                res["block_loglike_ms"] = timed(lambda: ops.vb_block_loglike(x, off, boff, ds, N * Tb, gauss, post, means, up[3], up[4], K),
                                                a.reps, a.regions)
                ch = res["forward_backward_ms"] = timed(lambda: ops.vb_forward_backward(lls, boff, sp, 0.9), a.reps, a.regions)
                se = res["forward_backward_serial_ms"] = timed(lambda: ops.vb_forward_backward_serial(lls, boff, sp, 0.9), a.reps, a.regions)
                res["blocks"] = Tb
                res["fb_spread"] = max((t[2] - t[1]) / t[0] for t in (ch, se))
                res["fb_serial_over_chunked"] = se[0] / ch[0]
                res["fb_chunked_wins"] = ch[2] < se[1]
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
