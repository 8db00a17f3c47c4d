"""Forward + backward of `ktf.autograd.res2_conv` (include/ktf_res2.h rules 7 - 13) next to the route it replaces
-- the slice composition through `ktf.autograd.tdnn_affine` and torch ops -- at the shapes of tools/bench_res2.py: B in {64, 512}
utterances of T = 300 frames, (C, scale, dilation) in {(512, 8, 2), (512, 8, 4), (1024, 8, 3)}, in every mode.

Per shape and mode, one JSON line: `new_ms` / `composition_ms` are [median, min, max] over `--regions` regions of `--reps`
forward + backward passes between two device events, the regions of the two alternating after a warm-up of both; `ratio` is median
over median (below 1: the new route is faster); `row_tile` and `slots` are what the backward kernels use.

    python tools/bench_res2_grad.py [--reps 5] [--regions 5] [--modes f32 bf16 bf16x3] [--batches 64 512]"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-tflite_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import ops  # noqa: E402
from bench_norm import alternate  # noqa: E402


def block(B, T, C, s, d, mode, a, dev, gen):
    w = C // s
    par = lambda *sh, k=1.0: (k * torch.randn(sh, device=dev, generator=gen)).requires_grad_(True)      # noqa: E731
    x, W, bias, nsh = par(B, T, C), par(s - 1, 3 * w, w, k=(3 * w) ** -0.5), par(s - 1, w, k=0.1), par(s - 1, w, k=0.1)
    nsc = (1.0 + 0.1 * torch.randn((s - 1, w), device=dev, generator=gen)).requires_grad_(True)
    g = torch.randn((B, T, C), device=dev, generator=gen)
    leaves = (x, W, bias, nsc, nsh)

    def new():
        torch.autograd.grad(ktf.autograd.res2_conv(x, W, bias, nsc, nsh, s, d, gemm=mode), leaves, g)

    def composition():
        ys = [x[:, :, :w]]
        for i in range(1, s):
            u = x[:, :, i * w:(i + 1) * w] + ys[-1] if i >= 2 else x[:, :, w:2 * w]
            z = ktf.autograd.tdnn_affine(u, W[i - 1].view(3, w, w).permute(2, 0, 1), bias[i - 1], [-d, 0, d], gemm=mode)
            ys.append(torch.relu(z) * nsc[i - 1] + nsh[i - 1])
        torch.autograd.grad(torch.cat(ys, 2), leaves, g)

    res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), B=B, T=T, C=C, scale=s, dilation=d, mode=mode, reps=a.reps,
               regions=a.regions, row_tile=ops.res2_grad_row_tile(w, s, d, ktf.layers.Res2Conv.MODES[mode]), slots=ops.res2_grad_slots(B, T, w, s))
    times = alternate(dict(new=new, composition=composition), a.reps, a.regions)
    res["new_ms"], res["composition_ms"] = times["new"], times["composition"]
    res["ratio"] = times["new"][0] / times["composition"][0]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--modes", nargs="+", default=["f32", "bf16", "bf16x3"], choices=("f32", "bf16", "bf16x3"))
    ap.add_argument("--batches", nargs="+", type=int, default=[64, 512])
    a = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(3)
    for B in a.batches:
        for C, s, d in ((512, 8, 2), (512, 8, 4), (1024, 8, 3)):
            for mode in a.modes:
                block(B, 300, C, s, d, mode, a, dev, gen)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
