#!/usr/bin/env python3
"""Attentive statistics pooling (ktf.autograd.attentive_stats_pooling: csrc/attn_pool.hip) against a torch composition of the same
rules -- a softmax over the masked time axis and weighted sums, fp32 -- in one process, alternating the two:

  training   forward and forward + backward at 64 x 300 x 1500 and 512 x 300 x 1500, H in {1, 1500}
  inference  the forward at 1024 x 1000 x 1500, H in {1, 1500}

Per case and side: the time of a call (device events around `--iters` calls, the median of `--rounds` rounds), the kernel launches
of one call (torch.profiler; null where the profiler gives no device events), the peak device memory a training step adds to its
inputs, and for the library the achieved bytes/s against the algorithmic bytes: x once and e twice forward, x, e, dx and de once
backward, over the valid rows. Prints one JSON line per case; `--out FILE` also writes the list there.

    python tools/bench_attn.py [--iters 10] [--rounds 5] [--small] [--out FILE]
"""

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-tflite_amd"))

import kaldi_tflite_amd as ktf  # noqa: E402

EPS = 1e-10


def torch_pool(x, e, lens, include_std=True):
    B, T, D = x.shape
    H = e.shape[2]
    mask = torch.arange(T, device=x.device)[None, :, None] < lens[:, None, None]
    w = torch.softmax(e.masked_fill(~mask, float("-inf")), dim=1)
    if 1 < H < D:
        w = w.repeat_interleave(D // H, dim=2)
    xm = torch.where(mask, x, torch.zeros((), device=x.device))
    mu = (w * xm).sum(1)
    if not include_std:
        return mu
    q = (w * xm * xm).sum(1)
    return torch.cat([mu, torch.sqrt(torch.clamp(q - mu * mu, min=0.0) + EPS)], dim=1)


def ktf_pool(x, e, lens, include_std=True):
    return ktf.autograd.attentive_stats_pooling(x, e, lens, include_std, EPS)


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in ev.name.lower()
                and "memset" not in ev.name.lower())
        return n or None
    except Exception:
        return None


def peak_extra(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def case(B, T, D, H, train, iters, rounds):
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(B * 7 + H)
    x = torch.randn((B, T, D), device=dev, generator=g)
    e = 2.0 * torch.randn((B, T, H), device=dev, generator=g)
    lens = torch.randint(T // 2, T + 1, (B,), device=dev, generator=g, dtype=torch.int32)
    gout = torch.randn((B, 2 * D), device=dev, generator=g)
    rows = int(lens.sum().item())
    fwd_bytes = rows * (D + 2 * H) * 4
    bwd_bytes = rows * 2 * (D + H) * 4

    def forward(pool):
        with torch.no_grad():
            return pool(x, e, lens)

    def step(pool):
        xr, er = x.detach().requires_grad_(True), e.detach().requires_grad_(True)
        pool(xr, er, lens).backward(gout)
        return xr.grad, er.grad

    sides = {"ktf": ktf_pool, "torch": torch_pool}
    modes = {"forward": forward} | ({"forward_backward": step} if train else {})
    a, b = forward(ktf_pool), forward(torch_pool)
    res = {"B": B, "T": T, "D": D, "H": H, "valid_rows": rows, "max_abs_diff_forward": float((a - b).abs().max()),
           "algorithmic_bytes": {"forward": fwd_bytes, "forward_backward": fwd_bytes + bwd_bytes}}
    del a, b
    for mode, run in modes.items():
        times = {k: [] for k in sides}
        for k, pool in sides.items():                 # warm-up: code objects, the allocator's blocks
            run(pool)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, pool in sides.items():             # alternating
                times[k].append(timed(lambda: run(pool), iters))
        res[mode] = {}
        for k, pool in sides.items():
            ms = statistics.median(times[k])
            res[mode][k] = {"ms": round(ms, 4), "ms_min": round(min(times[k]), 4), "ms_max": round(max(times[k]), 4),
                            "launches": launches(lambda: run(pool)), "peak_extra_bytes": peak_extra(lambda: run(pool))}
        res[mode]["ktf"]["bytes_per_s"] = round(res["algorithmic_bytes"][mode] / (res[mode]["ktf"]["ms"] * 1e-3))
        res[mode]["speedup_vs_torch"] = round(res[mode]["torch"]["ms"] / res[mode]["ktf"]["ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="toy sizes: a rehearsal of the script, not a measurement")
    ap.add_argument("--out")
    args = ap.parse_args()
    ktf._lib.require_gpu()
    if args.small:
        cases = [(4, 50, 60, 1, True), (4, 50, 60, 60, True), (2, 80, 60, 1, False)]
    else:
        cases = [(B, 300, 1500, H, True) for B in (64, 512) for H in (1, 1500)] + [(1024, 1000, 1500, H, False) for H in (1, 1500)]
    out = []
    for B, T, D, H, train in cases:
        r = case(B, T, D, H, train, args.iters, args.rounds)
        print(json.dumps(r), flush=True)
        out.append(r)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
