"""The Res2Net dilated convolution (include/ktf_res2.h: `ktf.layers.Res2Conv`) next to the composition it replaces
-- per group a slice + add, one `TDNN.forward` on the library's TDNN kernels and a write-back into the output's slice -- on B in
{64, 512} utterances of T = 300 frames and (C, scale, dilation) in {(512, 8, 2), (512, 8, 4), (1024, 8, 3)}, in every mode.

Per shape and mode, one JSON line: `layer_ms` / `composition_ms` are [median, min, max] over `--regions` regions of `--reps` calls
between two device events, the regions of the two alternating after a warm-up of both; `ratio` is median over median (below 1: the
layer is faster); `layer_launches` / `composition_launches` count kernels per call (the composition: Y_0's copy, and per group the add
or copy of its input, the conversion of that input where the mode reads bf16 rows, the GEMM and the write-back); `gbps` and `tflops`
are the layer's algorithmic traffic (x once, y once) and flops (2 * 3 * w * w per row and group) over its median time.

    python tools/bench_res2.py [--reps 10] [--regions 5] [--modes f32 bf16 bf16x3]"""

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
    layer = ktf.layers.Res2Conv(s, dilation=d, name=f"res2_{C}_{s}_{d}")
    layer.build((None, None, C))
    code = layer.MODES[mode]
    kernel, bias, nsc, nsh = layer.get_weights()
    x = torch.randn((B, T, C), device=dev, generator=gen)
    y, yc = torch.empty_like(x), torch.empty_like(x)
    groups = []
    for i in range(1, s):
        t = ktf.layers.TDNN(w, [-d, 0, d], name=f"group{i}")
        t.set_weights([kernel[i - 1][None], bias[i - 1]], fmt="tensorflow")
        groups.append((t, (torch.as_tensor(nsc[i - 1], device=dev), torch.as_tensor(nsh[i - 1], device=dev))))

    def composition():
        yc[:, :, :w] = x[:, :, :w]
        for i, (t, bn) in enumerate(groups, start=1):
            u = (x[:, :, i * w:(i + 1) * w] + yc[:, :, (i - 1) * w:i * w]) if i >= 2 else x[:, :, w:2 * w].contiguous()
            yc[:, :, i * w:(i + 1) * w] = t.forward(t.prepare_input(u, code), relu=True, bn=bn, gemm=code)[:, :, :w]

    res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), B=B, T=T, C=C, scale=s, dilation=d, mode=mode, reps=a.reps,
               regions=a.regions, row_tile=ops.res2_row_tile(w, s, d, code), layer_launches=1,
               composition_launches=1 + (s - 1) * (3 + int(mode == "bf16")))
    times = alternate(dict(layer=lambda: layer.forward(x, None, mode, out=y), composition=composition), a.reps, a.regions)
    res["layer_ms"], res["composition_ms"] = times["layer"], times["composition"]
    res["ratio"] = times["layer"][0] / times["composition"][0]
    sec = times["layer"][0] * 1e-3
    res["gbps"] = 2 * B * T * C * 4 / sec / 1e9
    res["tflops"] = 2.0 * B * T * (s - 1) * 3 * w * w / sec / 1e12
    res["max_abs_diff"] = float((y - yc).abs().max())
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--modes", nargs="+", default=["f32", "bf16", "bf16x3"], choices=("f32", "bf16", "bf16x3"))
    a = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(3)
    for B in (64, 512):
        for C, s, d in ((512, 8, 2), (512, 8, 4), (1024, 8, 3)):
            for mode in a.modes:
                block(B, 300, C, s, d, mode, a, dev, gen)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
