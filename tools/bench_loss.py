"""The classification head and its loss (include/ktf_loss.h: `ktf.autograd.ClassifierHead`) next to a torch
composition of the same cosine head -- `F.normalize` of the embeddings and of the weight, a matmul, the margin put on the target
column by `torch.where` over a one-hot mask, `F.cross_entropy` -- on B in {64, 512} x N in {7323, 7324} classes (contiguous logits:
ld = N, so 7323 is the case whose rows are not 16-byte aligned), D = 512, for kind "softmax", "am" and "aam".

Per shape and kind, one JSON line. `fused_*` is the ClassifierHead in gemm="f32" (GEMM by tdnn_affine, norms and loss by the
library's kernels), `torch_*` the composition (fp32 matmul by torch): `*_forward_ms` one forward with the graph kept,
`*_backward_ms` torch.autograd.grad of a kept graph with respect to the embeddings and the weight, `*_step_ms` both with fresh
gradients. `kernels_forward_ms` / `kernels_backward_ms` are the library calls around the GEMM alone on preallocated buffers (two
ktf_loss_row_inv_norm + ktf_loss_margin_softmax_forward; ktf_loss_margin_softmax_backward + two ktf_loss_row_inv_norm_backward),
`fused_gemm_step_ms` / `torch_gemm_step_ms` the head's GEMM alone, forward and backward (tdnn_affine in gemm="f32", which pads its
weight operand on every call, against torch's matmul): what the two heads spend outside the code this tool is about.
`kernels_*_gbps` their minimal traffic over the median time (forward: the logits once and both operands once; backward: logits read
and gradient written, both operands read and their norm gradients written). Regions alternate after a warm-up of all of them, each
`--reps` calls between two device events; median / min / max over `--regions` regions. `*_vs_torch` is the fused median over the
torch median (below 1: faster). `loss_diff` is |fused - torch| of the loss value.

The last line is one training step (forward, loss, backward) of a five-GEMM x-vector stack of the recipe's widths (gemm="bf16",
fused_norm=True) at 64 x 300 frames under each of the two AAM heads with 7323 classes, alternating, and under the 8-class
`cross_entropy` of tools/bench_norm.py. Reported, not gated.

    python tools/bench_loss.py [--D 512] [--reps 10] [--regions 5]"""

import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-tflite_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import _lib as L, autograd as A, ops  # noqa: E402
from bench_norm import alternate  # noqa: E402


def torch_head(emb, weight, labels, kind, margin, scale):
    """The cosine head as it is usually written in torch -> (mean loss, pred)."""
    c = F.normalize(emb) @ F.normalize(weight).T
    if kind == "am":
        phi = c - margin
    elif kind == "aam":
        cm, sm = math.cos(margin), math.sin(margin)
        phi = c * cm - torch.sqrt(torch.clamp(1.0 - c * c, min=L.LOSS_SIN2_FLOOR)) * sm
        phi = torch.where(c > -cm, phi, c - margin * sm)
    else:
        phi = c
    hot = F.one_hot(labels, c.shape[1]).bool()
    return F.cross_entropy(scale * torch.where(hot, phi, c), labels), c.argmax(1)


def head_block(B, N, D, kind, a, dev, gen):
    margin, scale = (0.0 if kind == "softmax" else 0.2), 30.0
    emb = torch.randn((B, D), device=dev, generator=gen).requires_grad_(True)
    labels = torch.randint(0, N, (B,), device=dev, generator=gen)
    head = A.ClassifierHead(D, N, kind=kind, margin=margin, scale=scale, normalize=True, gemm="f32", device=dev)
    w = head.weight
    kept = {"fused": head(emb, labels)[0], "torch": torch_head(emb, w, labels, kind, margin, scale)[0]}

    def step(fn):
        emb.grad = w.grad = None
        fn()[0].backward()

    # the library calls around the GEMM, on preallocated buffers
    with torch.no_grad():
        z = (emb @ w.T).contiguous()
    l32 = labels.to(torch.int32)
    ix, iw = torch.empty((B,), device=dev), torch.empty((N,), device=dev)
    loss, pred, lse = torch.empty((B,), device=dev), torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.float64, device=dev)
    dz, dix, diw, demb, dw = torch.empty_like(z), torch.empty_like(ix), torch.empty_like(iw), torch.empty_like(emb), torch.empty_like(w)
    gl = torch.full((B,), 1.0 / B, device=dev)
    ws = ops.loss_workspace(B, N, dev)
    xd, wd = emb.detach(), w.detach()

    def kernels_forward():
        ops.loss_row_inv_norm(xd, 1e-12, ix)
        ops.loss_row_inv_norm(wd, 1e-12, iw)
        ops.loss_margin_softmax_forward(z, l32, ix, iw, kind, margin, scale, loss, pred, lse, ws)

    def kernels_backward():
        ops.loss_margin_softmax_backward(z, l32, ix, iw, kind, margin, scale, lse, gl, dz, dix, diw, ws)
        ops.loss_row_inv_norm_backward(xd, 1e-12, ix, dix, demb)
        ops.loss_row_inv_norm_backward(wd, 1e-12, iw, diw, dw)

    kernels_forward()
    gz = torch.randn((B, N), device=dev, generator=gen) / N

    def gemm_step(fn):
        emb.grad = w.grad = None
        fn().backward(gz)

    fns = dict(fused_forward=lambda: head(emb, labels), torch_forward=lambda: torch_head(emb, w, labels, kind, margin, scale),
               fused_backward=lambda: torch.autograd.grad(kept["fused"], (emb, w), retain_graph=True),
               torch_backward=lambda: torch.autograd.grad(kept["torch"], (emb, w), retain_graph=True),
               fused_step=lambda: step(lambda: head(emb, labels)), torch_step=lambda: step(lambda: torch_head(emb, w, labels, kind, margin, scale)),
               kernels_forward=kernels_forward, kernels_backward=kernels_backward,
               fused_gemm_step=lambda: gemm_step(lambda: A.tdnn_affine(emb.unsqueeze(0), w.unsqueeze(1), None, [0]).squeeze(0)),
               torch_gemm_step=lambda: gemm_step(lambda: emb @ w.T))
    res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), B=B, N=N, D=D, kind=kind, margin=margin, scale=scale, reps=a.reps,
               regions=a.regions, workspace_mb=ws.numel() / 2 ** 20, loss_diff=abs(kept["fused"].item() - kept["torch"].item()))
    for k, v in alternate(fns, a.reps, a.regions).items():
        res[k + "_ms"] = v
    operands = float((B + N) * D * 4)
    res["kernels_forward_gbps"] = (B * N * 4 + operands) / (res["kernels_forward_ms"][0] * 1e-3) / 1e9
    res["kernels_backward_gbps"] = (2 * B * N * 4 + 2 * operands) / (res["kernels_backward_ms"][0] * 1e-3) / 1e9
    for k in ("forward", "backward", "step"):
        res[f"{k}_vs_torch"] = res[f"fused_{k}_ms"][0] / res[f"torch_{k}_ms"][0]
    print(json.dumps(res), flush=True)


def network(a, dev):
    Lr, M = ktf.layers, ktf.models
    feat, B, T, N = 30, 64, 300, 7323

    def stack():
        layers = [M.Input(shape=(None, feat))]
        for i, (units, ctx) in enumerate(((512, [-2, -1, 0, 1, 2]), (512, [-2, 0, 2]), (1500, [0]))):
            layers += [Lr.TDNN(units, ctx, name=f"tdnn{i + 1}"), Lr.ReLU(name=f"relu{i + 1}"), Lr.BatchNorm(name=f"bn{i + 1}")]
        layers += [Lr.StatsPooling(0, 0, reduce_time_axis=True, name="stats"), Lr.TDNN(512, [0], name="affine1"), Lr.ReLU(name="relu4"),
                   Lr.BatchNorm(name="bn4"), Lr.TDNN(512, [0], name="affine2")]
        return M.Sequential(layers, name="xvector_five_gemms")

    gen = torch.Generator(device=dev).manual_seed(5)
    feats = torch.randn((B, T, feat), device=dev, generator=gen)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    labels = torch.randint(0, N, (B,), device=dev, generator=gen)
    small = torch.randn((8, 512), device=dev, generator=gen) / 512 ** 0.5
    net = A.TrainableSequential(stack(), device=dev, gemm="bf16", fused_norm=True).train()
    heads = {g: A.ClassifierHead(512, N, kind="aam", margin=0.2, scale=30.0, gemm=g, device=dev) for g in ("f32", "bf16")}
    w = heads["f32"].weight

    def step(loss_of):
        for p in list(net.parameters()) + [w, heads["bf16"].weight]:
            p.grad = None
        loss_of(net(feats, lens)).backward()

    fns = dict(fused_head_f32=lambda: step(lambda e: heads["f32"](e, labels)[0]), fused_head_bf16=lambda: step(lambda e: heads["bf16"](e, labels)[0]),
               torch_head=lambda: step(lambda e: torch_head(e, w, labels, "aam", 0.2, 30.0)[0]),
               cross_entropy_8=lambda: step(lambda e: F.cross_entropy(e @ small.T, labels % 8)))
    res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), network="five GEMMs 512/512/1500/512/512, gemm=bf16, fused_norm", B=B, T=T,
               N=N, kind="aam")
    for k, v in alternate(fns, max(a.reps // 2, 1), a.regions).items():
        res[f"{k}_step_ms"] = v
    res["step_vs_torch"] = res["fused_head_f32_step_ms"][0] / res["torch_head_step_ms"][0]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(3)
    for B in (64, 512):
        for N in (7323, 7324):
            for kind in ("softmax", "am", "aam"):
                head_block(B, N, a.D, kind, a, dev, gen)
                torch.cuda.empty_cache()
    network(a, dev)


if __name__ == "__main__":
    main()
