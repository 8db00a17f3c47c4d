#!/usr/bin/env python3
"""Dense PLDA scoring (PLDA.score_dense) on a diarization-shaped batch: 64 recordings x 400 segments (5 min at 0.75 s), D = 512,
fp64 and fp32, target energy 0.1 and 0.5 (and no PCA). Prints ms per call (bench._time_ms, the status read included) and each
kernel's share of the GPU time of one call (torch.profiler): python tools/plda_dense_time.py [recordings] [segments]"""
import collections
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaldi-tflite_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import bench
import kaldi_tflite_amd as ktf

R = int(sys.argv[1]) if len(sys.argv) > 1 else 64
N = int(sys.argv[2]) if len(sys.argv) > 2 else 400
D = 512
rng = np.random.default_rng(41)
T = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
mean, psi = rng.standard_normal(D) * 0.1, np.sort(rng.uniform(0.05, 30.0, D))[::-1].copy()
# a few speakers per recording plus noise with a decaying spectrum, rows length-normalised (the shape of x-vectors)
scales = 0.985 ** np.arange(D)
rows = []
for r in range(R):
    cent = rng.standard_normal((4, D)) * scales * 3.0
    x = cent[rng.integers(0, 4, N)] + rng.standard_normal((N, D)) * scales
    rows.append(x * (np.sqrt(D) / np.linalg.norm(x, axis=1, keepdims=True)))
x64 = torch.as_tensor(np.concatenate(rows), device="cuda")
lengths = [N] * R


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


print(f"{R} recordings x {N} segments, D = {D}")
for dt in (torch.float64, torch.float32):
    layer = ktf.layers.PLDA(D, mean, T, psi, dtype=dt)
    x = x64.to(dt)
    for target in (0.1, 0.5, None):
        fn = lambda: layer.score_dense(x, lengths=lengths, target_energy=target)  # noqa: E731
        ms = bench._time_ms(torch, fn, 3)
        dims = layer.last_dense_dims.cpu().numpy()
        gpu_ms, shares = stage_shares(fn)
        print(f"{str(dt):14s} target {str(target):4s}: {ms:8.2f} ms per call; d min/median/max {dims.min()}/{int(np.median(dims))}/"
              f"{dims.max()}; kernels {gpu_ms:.2f} ms: " + ", ".join(f"{k} {s:.1%}" for k, s in shares))
