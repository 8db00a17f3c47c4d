"""The ReLU + BatchNorm training block (include/ktf_norm.h) next to the torch composition it replaces,
`autograd.batch_norm(torch.relu(z), ...)` run forward and backward through torch.autograd, on 64 x 300 x 512, 64 x 300 x 1500 (with
per-utterance lengths, all of them T, as the training module passes them) and the pooled (64, 512).

Per shape, one JSON line: `fused_forward_ms` / `fused_backward_ms` are ktf_norm_relu_bn_forward / _backward on preallocated buffers,
`fused_step_ms` one relu_batch_norm forward + backward through torch.autograd (allocation included); `torch_forward_ms`,
`torch_backward_ms` (torch.autograd.grad on a kept graph) and `torch_step_ms` the composition. Regions alternate after a warm-up of
all of them, each `--reps` calls between two device events; median / min / max over `--regions` regions. `*_tbps` is the block's
minimal traffic over the median time: 3 passes over the B T D fp32 activation forward (z twice, y once), 5 backward (gy and z
twice, dz once), 8 a step. `*_vs_torch` is the fused median over the torch median (below 1: faster).

The last line is one training step (forward, loss, backward) of a five-GEMM x-vector stack of the recipe's widths with fused_norm
off and on, alternating: the step's time and `torch.cuda.max_memory_allocated` above what was allocated before the step.
Reported, not gated.

    python tools/bench_norm.py [--B 64] [--T 300] [--reps 10] [--regions 5]"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-tflite_amd"))
import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import autograd as A, ops  # noqa: E402


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


def alternate(fns, reps, regions):
    for fn in fns.values():
        fn()
    times = {k: [] for k in fns}
    for _ in range(regions):                                        # alternating: all see the same neighbours on the machine
        for k, fn in fns.items():
            times[k].append(region(fn, reps))
    return {k: stats(v) for k, v in times.items()}


def block(shape, a, dev, gen):
    D = shape[-1]
    z = torch.randn(shape, device=dev, generator=gen) + 0.25
    g = torch.randn(shape, device=dev, generator=gen)
    gamma = torch.rand((D,), device=dev, generator=gen) + 0.5
    lens = torch.full((shape[0],), shape[1], dtype=torch.int32, device=dev) if len(shape) == 3 else None
    z3, g3 = (z, g) if len(shape) == 3 else (z.unsqueeze(0), g.unsqueeze(0))
    B, T = z3.shape[:2]
    mm, mv = torch.zeros((D,), device=dev), torch.ones((D,), device=dev)
    y, dz, dgamma = torch.empty_like(z3), torch.empty_like(z3), torch.empty_like(gamma)
    saved = torch.empty((2, D), dtype=torch.float64, device=dev)
    ws = ops.norm_workspace(B, T, D, dev)
    za, ga = z.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    kept = A.batch_norm(torch.relu(za), lens, mm.clone(), mv.clone(), ga, training=True)

    def fused_step():
        za.grad = ga.grad = None
        A.relu_batch_norm(za, lens, mm, mv, ga, training=True).backward(g)

    def torch_step():
        za.grad = ga.grad = None
        A.batch_norm(torch.relu(za), lens, mm, mv, ga, training=True).backward(g)

    fns = dict(fused_forward=lambda: ops.norm_relu_bn_forward(z3, D, lens, True, True, gamma, mm, mv, 0.99, 1e-3, y, saved, ws),
               torch_forward=lambda: A.batch_norm(torch.relu(za), lens, mm, mv, ga, training=True),
               fused_backward=lambda: ops.norm_relu_bn_backward(g3, z3, D, lens, True, True, gamma, saved, dz, dgamma, ws),
               torch_backward=lambda: torch.autograd.grad(kept, (za, ga), g, retain_graph=True),
               fused_step=fused_step, torch_step=torch_step)
    res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), shape=list(shape), reps=a.reps, regions=a.regions,
               workspace_mb=ws.numel() / 2 ** 20)
    act = float(B * T * D * 4)
    for k, v in alternate(fns, a.reps, a.regions).items():
        res[k + "_ms"] = v
        if k.startswith("fused"):
            passes = dict(forward=3, backward=5, step=8)[k.split("_")[1]]
            res[k + "_tbps"] = passes * act / (v[0] * 1e-3) / 1e12
    for k in ("forward", "backward", "step"):
        res[f"{k}_vs_torch"] = res[f"fused_{k}_ms"][0] / res[f"torch_{k}_ms"][0]
    print(json.dumps(res), flush=True)


def network(a, dev):
    Lr, M = ktf.layers, ktf.models
    feat, classes = 30, 8

    def stack():
        layers = [M.Input(shape=(None, feat))]
        for i, (units, ctx) in enumerate(((512, [-2, -1, 0, 1, 2]), (512, [-2, 0, 2]), (1500, [0]))):
            layers += [Lr.TDNN(units, ctx, name=f"tdnn{i + 1}"), Lr.ReLU(name=f"relu{i + 1}"), Lr.BatchNorm(name=f"bn{i + 1}")]
        layers += [Lr.StatsPooling(0, 0, reduce_time_axis=True, name="stats"), Lr.TDNN(512, [0], name="affine1"), Lr.ReLU(name="relu4"),
                   Lr.BatchNorm(name="bn4"), Lr.TDNN(512, [0], name="affine2")]
        return M.Sequential(layers, name="xvector_five_gemms")

    gen = torch.Generator(device=dev).manual_seed(5)
    feats = torch.randn((a.B, a.T, feat), device=dev, generator=gen)
    lens = torch.full((a.B,), a.T, dtype=torch.int32, device=dev)
    head = torch.randn((classes, 512), device=dev, generator=gen) / 512 ** 0.5
    labels = torch.arange(a.B, device=dev) % classes
    nets = {k: A.TrainableSequential(stack(), device=dev, gemm="bf16", fused_norm=f).train() for k, f in (("torch", False), ("fused", True))}

    def step(net):
        for p in net.parameters():
            p.grad = None
        torch.nn.functional.cross_entropy(net(feats, lens) @ head.T, labels).backward()

    res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), network="five GEMMs 512/512/1500/512/512, gemm=bf16", B=a.B, T=a.T)
    for k, net in nets.items():
        step(net)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step(net)
        torch.cuda.synchronize()
        res[f"{k}_step_peak_mb"] = (torch.cuda.max_memory_allocated() - before) / 2 ** 20
    for k, v in alternate({k: (lambda net=net: step(net)) for k, net in nets.items()}, max(a.reps // 2, 1), a.regions).items():
        res[f"{k}_step_ms"] = v
    res["step_vs_torch"] = res["fused_step_ms"][0] / res["torch_step_ms"][0]
    res["peak_vs_torch"] = res["fused_step_peak_mb"] / res["torch_step_peak_mb"]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(3)
    for shape in ((a.B, a.T, 512), (a.B, a.T, 1500), (a.B, 512)):
        block(shape, a, dev, gen)
        torch.cuda.empty_cache()
    network(a, dev)


if __name__ == "__main__":
    main()
