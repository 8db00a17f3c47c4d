"""Global-context attention logits (include/ktf_gctx.h: `AttentiveStatsPooling(global_context=True).attend`, three
launches) next to the two things that existed before it, on B in {64, 512} utterances of T = 300 frames, D = H in {1536, 3072} channels
and heads, A = 128 hidden units, in both arithmetics of the attention:

  (a) `cat`:   torch.cat([x, mu, sigma]) into (B, T, 3 D) and the plain layer's attend with a (3 D, A) W1 (mu and sigma are handed to it
               for free: they are computed outside the timed region);
  (b) `plain`: the plain layer's attend without context, W1 (D, A) -- less work than the new path does, the floor of the TDNN kernels.

Per shape and mode, one JSON line: `*_ms` are [median, min, max] over `--regions` regions of `--reps` calls between two device events,
the regions of the three alternating after a warm-up of all; `ratio_cat` / `ratio_plain` are median over median (below 1: the new path
is faster); `*_extra_mib` is the peak of torch's allocator above its level before the first call, less the logits' own bytes (new: mu / sigma and
the bias; the others: the concatenation and the hidden rows); `tflops` is the new path's algorithmic
2 B T A (D + H) and `gbps` its algorithmic traffic (x twice -- statistics and logits --, e once) over its median time.

    python tools/bench_gctx.py [--reps 5] [--regions 3] [--modes f32 bf16x3] [--batches 64 512] [--dims 1536 3072]"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-tflite_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import _lib as L, ops  # noqa: E402
from bench_norm import alternate  # noqa: E402

MODES = {"f32": L.GEMM_F32, "bf16x3": L.GEMM_BF16X3}


def extra_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return (peak - base) / 2.0 ** 20


def block(B, T, D, A, mode, a, dev, gen):
    H, code = D, MODES[mode]
    new = ktf.layers.AttentiveStatsPooling(A, heads=H, global_context=True, name=f"gctx_{D}")
    new.build((None, None, D))
    w1, b1, w2, b2 = new.get_weights()
    cat_layer, plain = (ktf.layers.AttentiveStatsPooling(A, heads=H, name=f"{n}_{D}") for n in ("cat", "plain"))
    cat_layer.set_weights([w1, b1, w2, b2])
    plain.set_weights([w1[:D], b1, w2, b2])
    x = torch.randn((B, T, D), device=dev, generator=gen)
    ctx = ops.gctx_stats(x, None, new.epsilon, torch.empty((B, 2, D), dtype=torch.float64, device=dev)).float().reshape(B, 1, 2 * D)

    bufs = {}                                    # the outputs of attend() live in buffers that are reused, as in the fused runner

    def scratch(path):
        return lambda role, shape, dtype: bufs.setdefault((path, role), torch.zeros(shape, dtype=dtype, device=dev))

    def cat():
        rows = torch.cat([x, ctx.expand(B, T, 2 * D)], 2)
        return cat_layer.attend(cat_layer.hidden.prepare_input(rows, code)[:, :, :3 * D], None, code, scratch("cat"))

    fns = dict(new=lambda: new.attend(x, None, code, scratch("new")), cat=cat,
               plain=lambda: plain.attend(plain.hidden.prepare_input(x, code)[:, :, :D], None, code, scratch("plain")))
    res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), B=B, T=T, D=D, A=A, H=H, mode=mode, reps=a.reps, regions=a.regions,
               row_tile=ops.gctx_row_tile(A, H, code))
    for k, fn in fns.items():                    # (the first call of each: its buffers are allocated here; the logits are in all three)
        res[f"{k}_extra_mib"] = extra_mib(fn) - B * T * ops.round_up(H, 8) * 4 / 2.0 ** 20
    res["max_abs_diff_cat"] = float((fns["new"]() - fns["cat"]()).abs().max())
    times = alternate(fns, a.reps, a.regions)
    for k in fns:
        res[f"{k}_ms"] = times[k]
    res["ratio_cat"], res["ratio_plain"] = times["new"][0] / times["cat"][0], times["new"][0] / times["plain"][0]
    sec = times["new"][0] * 1e-3
    res["tflops"], res["gbps"] = 2.0 * B * T * A * (D + H) / sec / 1e12, 4.0 * B * T * (2 * D + H) / sec / 1e9
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--modes", nargs="+", default=list(MODES), choices=tuple(MODES))
    ap.add_argument("--batches", nargs="+", type=int, default=[64, 512])
    ap.add_argument("--dims", nargs="+", type=int, default=[1536, 3072])
    ap.add_argument("--units", type=int, default=128)
    a = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(3)
    for B in a.batches:
        for D in a.dims:
            for mode in a.modes:
                block(B, 300, D, a.units, mode, a, dev, gen)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
