"""The dense affine kernels of the classification head (include/ktf_dense.h: `ktf.autograd.dense_affine`,
`ClassifierHead(affine="dense")`) next to the route they stand beside -- `tdnn_affine` on one sequence of M rows, which pads and
copies its weight operand on every call -- and next to torch, on M in {64, 512} rows x N in {7323, 7324, 2 x 7323} weight rows
(the last one is a head with two sub-centres), D = 512.

Per shape, one JSON line. `dense_forward_ms` / `dense_grad_data_ms` / `dense_grad_weights_ms` are the three library calls alone on
preallocated buffers; `tdnn_*_ms` the same products through `tdnn_affine` (forward with its padding, without a graph;
torch.autograd.grad of a kept graph with respect to the embeddings and to the weight -- torch fixes `needs_input_grad` when the
graph is built, so EACH of the two runs both of `tdnn_affine`'s gradient calls: compare either with the sum of the two dense
calls); `torch_*_ms` torch.matmul on preallocated outputs. `head_{tdnn,dense,torch}_step_ms` is ClassifierHead (kind "aam")
forward + backward through autograd with fresh gradients under either route and the torch composition of tools/bench_loss.py.
`dense_*_gbps` is the algorithmic traffic -- the weight once per call -- over the median time. Regions alternate after a warm-up of all of them, each `--reps` calls between two
device events; median / min / max over `--regions` regions. `*_vs_tdnn` and `*_vs_torch` are medians over medians (below 1: the dense
route is faster).

    python tools/bench_dense.py [--D 512] [--gemm f32] [--reps 10] [--regions 5]"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-tflite_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kaldi_tflite_amd import autograd as A, ops  # noqa: E402
from bench_loss import torch_head, torch_head_from_cosines  # noqa: E402
from bench_norm import alternate  # noqa: E402


def block(M, N, K, D, a, dev, gen):
    rows = N * K
    code = A._gemm_code(a.gemm)
    emb = torch.randn((M, D), device=dev, generator=gen).requires_grad_(True)
    labels = torch.randint(0, N, (M,), device=dev, generator=gen)
    heads = {r: A.ClassifierHead(D, N, kind="aam", gemm=a.gemm, sub_centers=K, device=dev, affine=r) for r in ("tdnn", "dense")}
    w = heads["dense"].weight
    with torch.no_grad():
        heads["tdnn"].weight.copy_(w)
    g = torch.randn((M, rows), device=dev, generator=gen) / rows
    xd, wd = emb.detach(), w.detach()
    z, dx, dw = torch.empty((M, rows), device=dev), torch.empty_like(xd), torch.empty_like(wd)
    ws = ops.dense_workspace(M, rows, D, dev)
    kept = A.tdnn_affine(emb.unsqueeze(0), w.unsqueeze(1), None, [0], gemm=a.gemm).squeeze(0)

    def tdnn_forward():
        with torch.no_grad():
            A.tdnn_affine(xd.unsqueeze(0), wd.unsqueeze(1), None, [0], gemm=a.gemm)

    def head_step(fn, weight):
        emb.grad = weight.grad = None
        fn()[0].backward()

    def torch_step():                                               # sub-centres: the largest centre of every class
        if K == 1:
            return torch_head(emb, w, labels, "aam", 0.2, 30.0)
        cos = torch.nn.functional.normalize(emb) @ torch.nn.functional.normalize(w).T
        return torch_head_from_cosines(cos.view(M, N, K).amax(dim=2), labels, "aam", 0.2, 30.0)

    fns = dict(dense_forward=lambda: ops.dense_forward(xd, wd, None, code, z),
               dense_grad_data=lambda: ops.dense_grad_data(g, wd, code, dx, ws),
               dense_grad_weights=lambda: ops.dense_grad_weights(g, xd, code, dw),
               tdnn_forward=tdnn_forward,
               tdnn_grad_data=lambda: torch.autograd.grad(kept, emb, g, retain_graph=True),
               tdnn_grad_weights=lambda: torch.autograd.grad(kept, w, g, retain_graph=True),
               torch_forward=lambda: torch.matmul(xd, wd.T, out=z),
               torch_grad_data=lambda: torch.matmul(g, wd, out=dx),
               torch_grad_weights=lambda: torch.matmul(g.T, xd, out=dw),
               head_tdnn_step=lambda: head_step(lambda: heads["tdnn"](emb, labels), heads["tdnn"].weight),
               head_dense_step=lambda: head_step(lambda: heads["dense"](emb, labels), w),
               head_torch_step=lambda: head_step(torch_step, w))
    res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), M=M, N=N, sub_centers=K, D=D, gemm=a.gemm, reps=a.reps, regions=a.regions,
               workspace_mb=ws.numel() / 2 ** 20)
    for k, v in alternate(fns, a.reps, a.regions).items():
        res[k + "_ms"] = v
    for call in ("forward", "grad_data", "grad_weights"):
        res[f"dense_{call}_gbps"] = rows * D * 4 / (res[f"dense_{call}_ms"][0] * 1e-3) / 1e9
        res[f"{call}_vs_tdnn"] = res[f"dense_{call}_ms"][0] / res[f"tdnn_{call}_ms"][0]
        res[f"{call}_vs_torch"] = res[f"dense_{call}_ms"][0] / res[f"torch_{call}_ms"][0]
    res["head_step_vs_tdnn"] = res["head_dense_step_ms"][0] / res["head_tdnn_step_ms"][0]
    res["head_step_vs_torch"] = res["head_dense_step_ms"][0] / res["head_torch_step_ms"][0]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, default=512)
    ap.add_argument("--gemm", default="f32", choices=("f32", "bf16", "bf16x3"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(3)
    for M in (64, 512):
        for N, K in ((7323, 1), (7324, 1), (7323, 2)):
            block(M, N, K, a.D, a, dev, gen)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
