#!/usr/bin/env python3
"""Sliding-window extraction for diarization (XvectorExtractor.extract_windows): 16 recordings of 5 min (the reference's speech
tiled with 1/f-coloured AM noise, as tests/synth.py makes them), 1.5 s windows every 0.75 s, f16mx as shipped (windows under 400
frames -> split-bf16) and f32. Prints windows/s, the existing path's 1.5 s-window throughput in the same process (1024 windows of 1.5 s
per call, tools/short_windows.py) and each kernel's share of the GPU time of one call (torch.profiler): python tools/diar_time.py"""
import collections
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaldi-tflite_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import bench
import synth
import kaldi_tflite_amd as ktf


def recordings(R=16, seconds=300):
    n = 16000 * seconds
    whole, _ = synth.speech_wavs()
    sp = whole[0]
    noise = synth.coloured_am_noise(R, n, seed=7)
    out = np.empty((R, n), np.float32)
    for r in range(R):
        tiled = np.roll(np.tile(sp, -(-n // sp.size))[:n], r * 12345)
        quiet = (np.arange(n) // (16000 * 7) + r) % 3 == 0                 # every third 7 s stretch: noise only (a pause)
        out[r] = np.clip(np.where(quiet, 0.05 * noise[r], tiled + 0.1 * noise[r]), -32767, 32767).round()
    return torch.as_tensor(out, device="cuda")


def stage_shares(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    t = collections.Counter()
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower():
            name = ev.name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0]
            t[name] += ev.device_time_total if hasattr(ev, "device_time_total") else ev.cuda_time_total
    tot = sum(t.values())
    return tot / 1e3, [(k, v / tot) for k, v in t.most_common()] if tot else []


cfg, w = synth.extractor_cfg(), synth.make_weights(seed=4321)
wavs = recordings()
g = torch.Generator(device="cuda").manual_seed(1234)
short = torch.clamp(torch.round(1000.0 * torch.randn((1024, 24000), generator=g, device="cuda")), -32767, 32767)
for gemm in ("f16mx", "f32"):
    m = synth.build_extractor(ktf, cfg, w, gemm=gemm)
    S = m.extract_windows(wavs).xvectors.shape[0]
    ms = bench._time_ms(torch, lambda: m.extract_windows(wavs), 3)
    ms_short = bench._time_ms(torch, lambda: m(short), 5)
    gpu_ms, shares = stage_shares(lambda: m.extract_windows(wavs))
    new = sum(s for k, s in shares if k.startswith("diar_"))
    wins = m.extract_windows(wavs).windows
    mean_len = float((wins[:, 2] - wins[:, 1]).float().mean())
    print(f"{gemm:6s}: 16 x 5 min, {S} windows (mean {mean_len:.1f} frames): {ms:8.2f} ms per call = {S / ms * 1e3:8.0f} windows/s | "
          f"kernels {gpu_ms:.2f} ms, diar_* {new:.2%}: " + ", ".join(f"{k} {s:.1%}" for k, s in shares[:12]), flush=True)
    gpu_short, shares_short = stage_shares(lambda: m(short))
    print(f"{gemm:6s}: existing path, 1024 x 1.5 s (148 voiced frames each, front end + VAD + CMVN per window): {ms_short:7.2f} ms = "
          f"{1024 / ms_short * 1e3:8.0f} windows/s | kernels {gpu_short:.2f} ms: " + ", ".join(f"{k} {s:.1%}" for k, s in shares_short[:12]),
          flush=True)
