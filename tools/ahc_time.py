#!/usr/bin/env python3
"""Agglomerative clustering (ktf.diarization.agglomerative_cluster) on diarization-shaped batches: 64 recordings x 400 segments
and 4 x 5000, fp32 and fp64, threshold mode (threshold 0.0, Kaldi's default) and num_speakers mode (4 speakers). The scores are
PLDA-like similarities of rows drawn around four centroids. Prints ms per call (bench._time_ms), merges per recording, and each
kernel's share of the GPU time of one call (torch.profiler): python tools/ahc_time.py"""
import collections
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaldi-tflite_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import bench
import kaldi_tflite_amd as ktf


def scores(R, N, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(R):
        x = rng.standard_normal((4, 32))[rng.integers(0, 4, N)] + rng.standard_normal((N, 32))
        out.append(x @ x.T / 32 - 0.5)
    return torch.as_tensor(np.stack(out).reshape(-1), device="cuda")


def stage_shares(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    t = collections.Counter()
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA and "kernel" in ev.name:
            name = ev.name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0]
            t[name] += ev.device_time_total if hasattr(ev, "device_time_total") else ev.cuda_time_total
    tot = sum(t.values())
    return tot / 1e3, [(k, v / tot) for k, v in t.most_common()] if tot else []


for R, N in ((64, 400), (4, 5000)):
    flat64 = scores(R, N, 41 + N)
    for dt in (torch.float32, torch.float64):
        flat = flat64.to(dt)
        blocks = [flat[r * N * N:(r + 1) * N * N].view(N, N) for r in range(R)]
        for mode in ({"threshold": 0.0}, {"num_speakers": 4}):
            fn = lambda: ktf.diarization.agglomerative_cluster(blocks, **mode)  # noqa: E731
            ms = bench._time_ms(torch, fn, 3)
            counts = fn()[1].cpu().numpy()
            gpu_ms, shares = stage_shares(fn)
            print(f"{R} x {N} {str(dt):14s} {str(mode):20s}: {ms:8.2f} ms per call ({ms * 1e3 / (N - counts.mean()):.2f} us per "
                  f"merge step); clusters min/max {counts.min()}/{counts.max()}; kernels {gpu_ms:.2f} ms: "
                  + ", ".join(f"{k} {s:.1%}" for k, s in shares), flush=True)
