"""Times the squeeze-excitation gate (include/ktf_se.h) against the torch composition on the same inputs, in one process and
alternating: forward alone and forward + backward, device events after a warm-up, B in {64, 512} x T = 300 x C in {512, 1024},
H = C / 4, with and without the residual; one JSON line per shape.   python tools/bench_se.py [--reps 20] [--peak-tbs 8.0]

The kernels one by one come from a kernel trace of `--trace B C`, which runs nothing but the training forward and the backward of
that shape (with the residual) `--reps` times:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o se -- python tools/bench_se.py --trace 512 1024 --reps 50
    python tools/bench_se.py --shares DIR/**/se_kernel_stats.csv 512 1024
`--shares` prints each kernel's mean time and, for the two scale kernels, the bytes they move (from the shapes) over that time as
a share of the HBM peak."""

import argparse
import csv
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-tflite_amd"))

import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import ops  # noqa: E402


def timed(fn, reps):
    """Median milliseconds of fn() by device events."""
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def shares(path, B, C, peak_tbs):
    """One JSON line: mean microseconds of every se_* kernel in a rocprofv3 kernel_stats.csv, and the scale kernels' HBM shares."""
    T, out = 300, {"B": B, "T": 300, "C": C}
    for row in csv.DictReader(open(path)):
        name = row["Name"]
        if name.startswith("void se_") or name.startswith("se_"):
            key = name.replace("void ", "").split("(")[0]
            out[key + "_us"] = float(row["AverageNs"]) / 1e3
    nbytes = B * T * C * 4
    for key, passes in (("se_scale_kernel<true>", 3), ("se_scale_grad_kernel", 2)):
        if key + "_us" in out:
            out[key + "_share_of_peak"] = passes * nbytes / (out[key + "_us"] * 1e-6) / (peak_tbs * 1e12)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak in TB/s the shares are taken of")
    ap.add_argument("--trace", nargs=2, type=int, metavar=("B", "C"), help="only the kernels' own launches of this shape, for a kernel trace")
    ap.add_argument("--shares", nargs=3, metavar=("CSV", "B", "C"), help="per-kernel means of a trace's kernel_stats.csv for this shape")
    args = ap.parse_args()
    if args.shares:
        return shares(args.shares[0], int(args.shares[1]), int(args.shares[2]), args.peak_tbs)
    dev = "cuda"
    if args.trace:
        B, C = args.trace
        T, H = 300, C // 4
        rnd = lambda *s: torch.randn(*s, device=dev)      # noqa: E731
        leaves = [t.requires_grad_(True) for t in (rnd(B, T, C), rnd(C, H) / C ** 0.5, rnd(H), rnd(H, C) / H ** 0.5, rnd(C))]
        r, gy = rnd(B, T, C), rnd(B, T, C)
        for _ in range(args.reps):
            torch.autograd.grad(ktf.autograd.squeeze_excite(*leaves, None, r), leaves, gy)
        torch.cuda.synchronize()
        return
    for B in (64, 512):
        for C in (512, 1024):
            for res in (False, True):
                T, H = 300, C // 4
                g = torch.Generator(device=dev).manual_seed(1)
                rnd = lambda *s: torch.randn(*s, device=dev, generator=g)      # noqa: E731
                x, r, gy = rnd(B, T, C), (rnd(B, T, C) if res else None), rnd(B, T, C)
                w1, b1, w2, b2 = rnd(C, H) / C ** 0.5, rnd(H), rnd(H, C) / H ** 0.5, rnd(C)
                leaves = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]

                def ours(backward, leaves=leaves, r=r, gy=gy):
                    y = ktf.autograd.squeeze_excite(*leaves, None, r)
                    if backward:
                        torch.autograd.grad(y, leaves, gy)

                def torch_ref(backward, leaves=leaves, r=r, gy=gy):
                    xx, a1, c1, a2, c2 = leaves
                    y = xx * torch.sigmoid(torch.relu(xx.mean(1) @ a1 + c1) @ a2 + c2).unsqueeze(1)
                    y = y + r if r is not None else y
                    if backward:
                        torch.autograd.grad(y, leaves, gy)

                # the whole inference call (three launches)
                y = torch.empty_like(x)
                ws = torch.empty(ops.se_gate_floats(B, C), device=dev)
                fwd_all = lambda: ops.se_gate(x, r, None, w1, b1, w2, b2, y, ws)      # noqa: E731
                out = {"B": B, "T": T, "C": C, "H": H, "residual": res}
                for name, bw in (("fwd", False), ("fwd_bwd", True)):
                    for _ in range(3):
                        ours(bw), torch_ref(bw)
                    a, b = [], []
                    for _ in range(3):                                   # alternating
                        a.append(timed(lambda: ours(bw), args.reps))
                        b.append(timed(lambda: torch_ref(bw), args.reps))
                    out[name + "_ms"], out[name + "_torch_ms"] = sorted(a)[1], sorted(b)[1]
                    out[name + "_ratio"] = out[name + "_torch_ms"] / out[name + "_ms"]
                fwd_all()
                out["inference_ms"] = timed(fwd_all, args.reps)
                nbytes = B * T * C * 4
                out["scale_bytes"] = nbytes * (3 if res else 2)
                # a lower bound of the scale pass's share: its bytes over the whole inference call (per kernel: --trace / --shares)
                out["scale_share_of_peak_at_least"] = out["scale_bytes"] / (out["inference_ms"] * 1e-3) / (args.peak_tbs * 1e12)
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
