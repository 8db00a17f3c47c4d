"""Multi-layer feature aggregation (include/ktf_agg.h: `ktf.layers.Aggregate`) next to the composition it replaces
-- `torch.cat` of the sources and one context-[0] `TDNN.forward` on the library's TDNN kernels in the same mode -- on B in {64, 512}
utterances of T = 300 frames, three sources of C in {512, 1024} channels each and 1536 units, in every mode.

Per shape and mode, one JSON line: `layer_ms` / `composition_ms` are [median, min, max] over `--regions` regions of `--reps` calls
between two device events, the regions of the two alternating after a warm-up of both; `ratio` is median over median (below 1: the
layer is faster); `tflops` is the layer's algorithmic 2 B T K units and `gbps` its algorithmic traffic (every source once, w once, y
once) over its median time; `bound` names the larger of the two times those figures take at `--peak-tflops` (of the mode's matrix
instruction) and `--peak-tbs`.

    python tools/bench_agg.py [--reps 10] [--regions 5] [--modes f32 bf16 bf16x3] [--batches 64 512]"""

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

PASSES = {"f32": 1, "bf16": 1, "bf16x3": 3}      # matrix passes over the algorithmic flops


def block(B, T, C, units, mode, a, dev, gen):
    layer = ktf.layers.Aggregate(units, ["s0", "s1"], activation="relu", batch_norm=True, name=f"agg_{C}")
    layer.build((None, None, C), [(None, None, C)] * 2)
    code, K = layer.MODES[mode], 3 * C
    kernel, bias, nsc, nsh = layer.get_weights()
    xs = [torch.randn((B, T, C), device=dev, generator=gen) for _ in range(3)]
    y = torch.empty((B, T, units), device=dev)
    t = ktf.layers.TDNN(units, [0], name=f"cat_{C}")
    t.set_weights([kernel[None, None], bias], fmt="tensorflow")
    bn = (torch.as_tensor(nsc, device=dev), torch.as_tensor(nsh, device=dev))
    out = {}

    def composition():
        out["y"] = t.forward(t.prepare_input(torch.cat(xs, 2), code), relu=True, bn=bn, gemm=code)

    res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), B=B, T=T, C=C, sources=3, units=units, mode=mode, reps=a.reps, regions=a.regions,
               row_tile=ops.agg_row_tile(units, K, code))
    times = alternate(dict(layer=lambda: layer.forward(xs[2], None, xs[:2], mode, out=y), composition=composition), a.reps, a.regions)
    res["layer_ms"], res["composition_ms"] = times["layer"], times["composition"]
    res["ratio"] = times["layer"][0] / times["composition"][0]
    sec = times["layer"][0] * 1e-3
    flops, nbytes = 2.0 * B * T * K * units, 4.0 * (B * T * K + units * K + B * T * units)
    res["tflops"], res["gbps"] = flops / sec / 1e12, nbytes / sec / 1e9
    peak = a.peak_tflops_f32 if mode == "f32" else a.peak_tflops
    t_mat, t_mem = PASSES[mode] * flops / (peak * 1e12), nbytes / (a.peak_tbs * 1e12)
    res["bound"] = "matrix" if t_mat >= t_mem else "memory"
    res["of_bound"] = max(t_mat, t_mem) / sec
    res["max_abs_diff"] = float((y - out["y"][:, :, :units].float()).abs().max())
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--modes", nargs="+", default=["f32", "bf16", "bf16x3"], choices=("f32", "bf16", "bf16x3"))
    ap.add_argument("--batches", nargs="+", type=int, default=[64, 512])
    ap.add_argument("--peak-tflops", type=float, default=2500.0, help="dense bf16 matrix peak of the device")
    ap.add_argument("--peak-tflops-f32", type=float, default=157.0, help="fp32 matrix peak of the device")
    ap.add_argument("--peak-tbs", type=float, default=8.0)
    a = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(3)
    for B in a.batches:
        for C in (512, 1024):
            for mode in a.modes:
                block(B, 300, C, 1536, mode, a, dev, gen)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
