"""The optimiser step of ktf.optim (include/ktf_optim.h) next to torch.optim on the parameters of the real model:
the x-vector network (4.5 M elements in 21 tensors) and a 7 323-class head (3.7 M), about 8.2 M elements in 22 tensors, 14 of them
512-element biases and gammas. The gradients are Gaussian until the first zero_grad and zeros from then on (the kernels' time does
not depend on the values); nothing but the optimiser runs.

One JSON line per configuration: `step_zero_ms` is `opt.step(); opt.zero_grad()` (torch: `zero_grad(set_to_none=False)`, preceded by
`clip_grad_norm_` where the configuration clips), `step_ms` the step alone (with the clipping). The ktf configurations are SGD with
momentum, the same with clipping, the same with max-change (per tensor and global), and Adam; the torch ones are SGD and Adam in
their default (foreach) and `fused=True` forms, SGD also with clipping. All regions alternate in one process after a warm-up of all
of them, each `--reps` calls between two device events; median / min / max over `--regions` regions. `vs_torch` is the ktf median over
the median of the torch configuration named in `against` (below 1: faster). `gbps` is the minimal traffic of the passes the
configuration runs over the median step time: 20 B per element for the SGD apply, 4 for the reduce over g, 12 for the max-change
reduce, 28 for the Adam apply. The arenas (33 MB each) fit the last-level cache, so these are not HBM rates. Reported, not gated.

`--only NAME --iters N` runs one configuration N times and nothing else: the run to put under a kernel trace, whose per-kernel call
counts over N give the launches of a step.

    python tools/bench_optim.py [--reps 20] [--regions 7] [--classes 7323] [--only NAME --iters 50]"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-tflite_amd"))
import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import ops  # noqa: E402

DEV = "cuda:0"


def model_shapes(classes):
    """The parameter tensors of the recipe's x-vector network (weight [u, k, d], bias, gamma per layer) and the head's weight."""
    shapes = []
    for units, nctx, din, bn in ((512, 5, 30, True), (512, 3, 512, True), (512, 3, 512, True), (512, 1, 512, True), (1500, 1, 512, True),
                                 (512, 1, 3000, True), (512, 1, 512, True)):
        shapes += [(units, nctx, din), (units,)] + ([(units,)] if bn else [])
    return shapes + [(classes, 512)]


def make_params(shapes, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, device=DEV, generator=gen) * 0.05) for s in shapes]


def set_grads(params, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    for p in params:
        g = torch.randn(p.shape, device=DEV, generator=gen) * 1e-3
        if p.grad is None:
            p.grad = g
        else:
            p.grad.copy_(g)


# |g| = 1e-3 sqrt(8.2 M) = 2.9: the clip and both max-change limits bite
CLIP, MC_TENSOR, MC_GLOBAL, LR = 1.0, 0.002, 0.005, 0.01
KTF = {
    "ktf_sgd": (dict(kind="sgd", momentum=0.9), 20, "torch_sgd_fused"),
    "ktf_sgd_clip": (dict(kind="sgd", momentum=0.9, clip_norm=CLIP), 24, "torch_sgd_fused_clip"),
    "ktf_sgd_maxchange": (dict(kind="sgd", momentum=0.9, max_change=MC_TENSOR, max_change_global=MC_GLOBAL), 32, "torch_sgd_fused"),
    "ktf_sgd_clip_maxchange": (dict(kind="sgd", momentum=0.9, clip_norm=CLIP, max_change=MC_TENSOR, max_change_global=MC_GLOBAL), 36,
                               "torch_sgd_fused_clip"),
    "ktf_adam": (dict(kind="adam"), 28, "torch_adam_fused"),
}
TORCH = {
    "torch_sgd": (torch.optim.SGD, dict(momentum=0.9), False),
    "torch_sgd_fused": (torch.optim.SGD, dict(momentum=0.9, fused=True), False),
    "torch_sgd_clip": (torch.optim.SGD, dict(momentum=0.9), True),
    "torch_sgd_fused_clip": (torch.optim.SGD, dict(momentum=0.9, fused=True), True),
    "torch_adam": (torch.optim.Adam, dict(), False),
    "torch_adam_fused": (torch.optim.Adam, dict(fused=True), False),
}


def build(name, shapes):
    """(step, step_zero, elements) of configuration `name` on parameters of its own."""
    params = make_params(shapes, 1)
    n = sum(p.numel() for p in params)
    if name in KTF:
        opt = ktf.optim.Optimizer(params, lr=LR, **KTF[name][0])
        set_grads(params, 2)

        def step():
            opt.step()

        def step_zero():
            opt.step()
            opt.zero_grad()
        return step, step_zero, n
    cls, kw, clip = TORCH[name]
    opt = cls(params, lr=LR, **kw)
    set_grads(params, 2)

    def step():
        if clip:
            torch.nn.utils.clip_grad_norm_(params, CLIP)
        opt.step()

    def step_zero():
        step()
        opt.zero_grad(set_to_none=False)
    return step, step_zero, n


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--classes", type=int, default=7323)
    ap.add_argument("--only", default=None)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    shapes = model_shapes(a.classes)
    if a.only:
        step, _, n = build(a.only, shapes)
        for _ in range(a.iters):
            step()
        torch.cuda.synchronize()
        print(json.dumps(dict(only=a.only, iters=a.iters, elements=n, tensors=len(shapes))), flush=True)
        return
    names = list(KTF) + list(TORCH)
    built = {}
    for k in names:
        try:
            built[k] = build(k, shapes)
            built[k][0](), built[k][1]()                   # warm-up of all of them
        except (TypeError, RuntimeError, ValueError) as e:  # a torch without fused=True for this optimiser
            print(json.dumps(dict(config=k, unavailable=str(e)[:200])), flush=True)
    torch.cuda.synchronize()
    times = {k: dict(step=[], step_zero=[]) for k in built}
    for _ in range(a.regions):                             # alternating: all see the same neighbours on the machine
        for k, (step, step_zero, _) in built.items():
            times[k]["step"].append(region(step, a.reps))
            times[k]["step_zero"].append(region(step_zero, a.reps))
    res = {}
    for k in built:
        n = built[k][2]
        res[k] = dict(config=k, build=ops.build_id(), gpu=torch.cuda.get_device_name(0), torch=torch.__version__, elements=n,
                      tensors=len(shapes), reps=a.reps, regions=a.regions, step_ms=stats(times[k]["step"]),
                      step_zero_ms=stats(times[k]["step_zero"]))
    for k in built:
        if k in KTF:
            _, bytes_per, against = KTF[k]
            res[k]["gbps"] = bytes_per * res[k]["elements"] / (res[k]["step_ms"][0] * 1e-3) / 1e9
            if against in res:
                res[k]["against"] = against
                res[k]["vs_torch"] = res[k]["step_ms"][0] / res[against]["step_ms"][0]
                res[k]["step_zero_vs_torch"] = res[k]["step_zero_ms"][0] / res[against]["step_zero_ms"][0]
        print(json.dumps(res[k]), flush=True)


if __name__ == "__main__":
    main()
