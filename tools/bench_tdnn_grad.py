"""Forward plus backward of the trainable TDNN affine on the sitw layer shapes -- 512 x (5 * 512), 512 x (3 * 512),
512 x 512 and 1500 x 512 -- for 64 utterances of 300 frames: `forward_ms` is ktf_tdnn with KTF_GEMM_F32 (the figure the gradients
stand next to), `data_ms` ktf_grad_tdnn_data, `weights_ms` ktf_grad_tdnn_weights, each on preallocated buffers, and `step_ms` one
tdnn_affine forward + backward through torch.autograd (padding, allocation and the three calls). Regions alternate after a warm-up
of all four, each `--reps` calls between two device events; median / min / max over `--regions` regions. TFLOP/s is the algorithmic
2 B T_out units nctx din per GEMM (three of them in a step) over the median time. One JSON line per shape. Reported, not gated.

`--gemm all` times the three modes of `tdnn_affine(gemm=)` -- "f32", "bf16", "bf16x3": the forward on fp32 x with that mode's weight
operand(s), ktf_grad_tdnn16_data / _weights -- in the same process, their regions alternating with the fp32 ones: the keys carry the
mode ("bf16_data_ms", ...; the fp32 ones keep their names), and `<mode>_<call>_vs_f32` is the median time over the fp32 median of the
same run (below 1: faster). `--gemm bf16` / `bf16x3`: that mode next to fp32. The default, `--gemm f32`, is the fp32 run alone.

    python tools/bench_tdnn_grad.py [--B 64] [--T 300] [--reps 10] [--regions 5] [--gemm f32|bf16|bf16x3|all]"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-tflite_amd"))
from kaldi_tflite_amd import _lib as L, autograd as A, ops  # noqa: E402

SHAPES = [(512, [-2, -1, 0, 1, 2], 512), (512, [-2, 0, 2], 512), (512, [0], 512), (1500, [0], 512)]      # units, context, din


def region(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def stats(v):
    return [float(np.median(v)), float(min(v)), float(max(v))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--gemm", choices=("f32", "bf16", "bf16x3", "all"), default="f32")
    a = ap.parse_args()
    modes16 = {"f32": (), "all": ("bf16", "bf16x3")}.get(a.gemm, (a.gemm,))
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(3)
    for units, context, din in SHAPES:
        B, T, nctx = a.B, a.T, len(context)
        d = A._desc(units, din, context, 1, "SAME")
        Up, Tout = ops.round_up(units, 256), ops.tdnn_out_len(T, d)
        x = torch.randn((B, T, d.din_pad), device=dev, generator=gen)
        w = torch.zeros((Up, nctx, d.din_pad), device=dev)
        w[:units] = torch.randn((units, nctx, d.din_pad), device=dev, generator=gen) / np.sqrt(nctx * din)
        bias = torch.randn((units,), device=dev, generator=gen)
        g = torch.randn((B, Tout, units), device=dev, generator=gen)
        y, dx, dw, db = torch.empty_like(g), torch.empty_like(x), torch.empty_like(w), torch.empty_like(bias)
        ws = ops.grad_tdnn_workspace(B, T, d, x.device)
        w2 = w.view(Up, nctx * d.din_pad)
        xa = x[:, :, :din].clone().requires_grad_(True)
        wa, ba = w[:units, :, :din].clone().requires_grad_(True), bias.clone().requires_grad_(True)

        def step():
            xa.grad = wa.grad = ba.grad = None
            A.tdnn_affine(xa, wa, ba, context).backward(g)

        fns = dict(forward=lambda: ops.tdnn(x, None, d, w2, None, bias, None, None, y),
                   data=lambda: ops.grad_tdnn_data(g, None, d, w2, dx, ws),
                   weights=lambda: ops.grad_tdnn_weights(x, None, d, g, dw.view(Up, -1), db, ws), step=step)
        for mode in modes16:
            code = A._gemm_code(mode)
            fd = A._desc(units, din, context, 1, "SAME")
            fd.gemm, fd.w_dtype = code, L.KTF_BF16
            wh = w2.to(torch.bfloat16)
            wl = (w2 - wh.to(torch.float32)).to(torch.bfloat16) if mode == "bf16x3" else None
            ws16 = ops.grad_tdnn16_workspace(B, T, d, code, x.device)

            def step16(mode=mode):
                xa.grad = wa.grad = ba.grad = None
                A.tdnn_affine(xa, wa, ba, context, gemm=mode).backward(g)

            fns.update({f"{mode}_forward": lambda fd=fd, wh=wh, wl=wl: ops.tdnn(x, None, fd, wh, wl, bias, None, None, y),
                        f"{mode}_data": lambda code=code, ws16=ws16: ops.grad_tdnn16_data(g, None, d, w2, dx, ws16, code),
                        f"{mode}_weights": lambda code=code, ws16=ws16: ops.grad_tdnn16_weights(x, None, d, g, dw.view(Up, -1), db, ws16, code),
                        f"{mode}_step": step16})
        fns["forward"]()
        forward_kernel = ops.last_kernel()
        for fn in fns.values():
            fn()
        res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), units=units, context=context, din=din, B=B, T=T,
                   forward_kernel=forward_kernel, workspace_mb=ws.numel() / 2 ** 20, reps=a.reps, regions=a.regions)
        times = {k: [] for k in fns}
        for _ in range(a.regions):                                  # alternating: all see the same neighbours on the machine
            for k, fn in fns.items():
                times[k].append(region(fn, a.reps))
        flop = 2.0 * B * Tout * units * nctx * din
        for k, v in times.items():
            res[k + "_ms"] = stats(v)
            res[k + "_tflops"] = (3 if k.endswith("step") else 1) * flop / (res[k + "_ms"][0] * 1e-3) / 1e12
        for mode in modes16:
            for k in ("forward", "data", "weights", "step"):
                res[f"{mode}_{k}_vs_f32"] = res[f"{mode}_{k}_ms"][0] / res[k + "_ms"][0]
        print(json.dumps(res), flush=True)
        del x, w, g, y, dx, dw, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
