"""Training global-context attention (include/ktf_gcgrad.h: `ktf.autograd.global_context_attention`, forward +
backward) next to the only way there was before it, on B in {64, 512} utterances of T = 300 frames, D = H in {1536, 3072} channels and
heads, A = 128 hidden units, in both arithmetics of the attention:

  `cat`: torch.cat([x, mu, sigma]) into (B, T, 3 D), two `tdnn_affine` calls and torch.tanh between them, differentiated by autograd (mu
         and sigma are torch ops on x inside the timed region, as a training step has to compute them).

Per shape and mode, one JSON line: `*_ms` are [median, min, max] over `--regions` regions of `--reps` forward + backward steps between
two device events, the regions of the two alternating after a warm-up of both; `ratio_cat` is median over median (below 1: the new path
is faster, above 1: it is SLOWER); `*_step_mib` is the peak of torch's allocator during one step above its level before it (x, the
weights and the incoming gradient are allocated before). `hidden_ms` / `data_ms` time the two big launches alone, `*_tflops` their
algorithmic 2 B T A (D + H) and 2 B T A D over the median, `*_peak_frac` that over the fp32 matrix peak of 157.3 TFLOP/s.

    python tools/bench_gcgrad.py [--reps 5] [--regions 3] [--modes f32 bf16x3] [--batches 64 512] [--dims 1536 3072]"""

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
PEAK_F32_MATRIX_TFLOPS = 157.3


def step_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def block(B, T, D, A, mode, a, dev, gen):
    H, code, eps = D, MODES[mode], 1e-5
    G = ktf.autograd
    layer = ktf.layers.AttentiveStatsPooling(A, heads=H, global_context=True, name=f"gcgrad_{D}")
    layer.build((None, None, D))
    w1, b1, w2, b2 = (torch.as_tensor(w, device=dev).requires_grad_(True) for w in layer.get_weights())
    x = torch.randn((B, T, D), device=dev, generator=gen).requires_grad_(True)
    de = torch.randn((B, T, H), device=dev, generator=gen)
    leaves = (x, w1, b1, w2, b2)

    def run(e):
        e.backward(de)
        grads = [t.grad for t in leaves]
        for t in leaves:
            t.grad = None
        return grads

    def new():
        return run(G.global_context_attention(x, w1, b1, w2, b2, None, "tanh", eps, mode))

    def cat():
        mu = x.mean(1, keepdim=True)
        sigma = ((x * x).mean(1, keepdim=True) - mu * mu).clamp(min=0).add(eps).sqrt()
        rows = torch.cat([x, mu.expand(B, T, D), sigma.expand(B, T, D)], 2)
        h = torch.tanh(G.tdnn_affine(rows, w1.T.unsqueeze(1), b1, [0], gemm=mode))
        return run(G.tdnn_affine(h, w2.T.unsqueeze(1), b2, [0], gemm=mode))

    fns = dict(new=new, cat=cat)
    res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), B=B, T=T, D=D, A=A, H=H, mode=mode, reps=a.reps, regions=a.regions,
               row_tile=ops.gcgrad_row_tile(A, H, code))
    gn, gc = new(), cat()
    res["max_rel_diff_cat"] = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(gn, gc))
    del gn, gc
    for k, fn in fns.items():
        res[f"{k}_step_mib"] = step_mib(fn)
    times = alternate(fns, a.reps, a.regions)
    for k in fns:
        res[f"{k}_ms"] = times[k]
    res["ratio_cat"] = times["new"][0] / times["cat"][0]

    # the two big launches alone, on operands made once
    with torch.no_grad():
        ctx = ops.gctx_stats(x, None, eps, torch.empty((B, 2, D), dtype=torch.float64, device=dev))
        g = ops.gctx_bias(ctx, w1[D:], b1, torch.empty((B, A), dtype=torch.float32, device=dev))
        dz, h, dx = torch.zeros((B, T, A), device=dev), torch.zeros((B, T, A), device=dev), torch.zeros((B, T, D), device=dev)
        coef = torch.zeros((B, 2, D), dtype=torch.float64, device=dev)
        act = L.ACT_TANH
        ops.gcgrad_hidden(x, None, w1[:D], g, act, w2, code, de, dz, h)
        ops.gcgrad_context(dz, None, ctx, w1[D:], eps, None, None, coef, ops.gcgrad_workspace(B, A, dev))
        big = alternate(dict(hidden=lambda: ops.gcgrad_hidden(x, None, w1[:D], g, act, w2, code, de, dz, h),
                             data=lambda: ops.gcgrad_data(dz, None, w1[:D], x, ctx, coef, code, dx, accumulate=False)), a.reps, a.regions)
    for k, flops in (("hidden", 2.0 * B * T * A * (D + H)), ("data", 2.0 * B * T * A * D)):
        res[f"{k}_ms"] = big[k]
        res[f"{k}_tflops"] = flops / (big[k][0] * 1e-3) / 1e12
        res[f"{k}_peak_frac"] = res[f"{k}_tflops"] / PEAK_F32_MATRIX_TFLOPS
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
