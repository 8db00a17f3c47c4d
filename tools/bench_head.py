"""The loss kernels with sub-centres, the inter-top-k penalty and label smoothing (include/ktf_head.h)
on B in {64, 512} x 7323 classes, the library calls on preallocated buffers and given logits, AAM at margin 0.2 and scale 30:

  `off_*`    K = 1, topk = 0, smoothing = 0: ktf_head_forward / ktf_head_backward (`head_*_ms`) against
             ktf_loss_margin_softmax_forward / _backward (`loss_*_ms`), the calls the defaults of `margin_softmax_loss` keep making;
             `off_step_vs_loss` is the new kernels' forward + backward over the old ones' (above 1: slower).
  `on_*`     K = 2, topk = 5, penalty = 0.06, smoothing = 0.1: the two calls (`head_*_ms`) against a torch composition of the same rules
             on the same logits and norms (`torch_*_ms`: amax over the centres, topk, scatter of the penalty, the margin on the target
             by torch.where, cross entropy with label_smoothing; backward by torch.autograd.grad with respect to z and both norms).
             `on_step_vs_torch` below 1: faster. `loss_diff` is |kernels - torch| of the mean loss.
  `launches` kernels launched per forward + backward: 3 for the library (forward, backward, finalize); for the composition counted by
             torch.profiler over one step (null if the profiler gives no device events).
  `topk64_*` the forward call at topk = 64: one selection round per member.

Regions alternate after a warm-up of all of them, each `--reps` calls between two device events; median / min / max over `--regions`
regions, as in tools/bench_loss.py. One JSON line per batch size. Reported, not gated.

    python tools/bench_head.py [--reps 10] [--regions 5]"""

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
from kaldi_tflite_amd import _lib as L, ops  # noqa: E402
from bench_norm import alternate  # noqa: E402


def torch_rules(z, ix, iw, labels, K, topk, penalty, eps, margin, scale):
    """The rules of ktf_head.h (AAM) as they are usually written in torch, on given logits -> the mean loss."""
    B, N = z.shape[0], z.shape[1] // K
    c = (z * ix[:, None] * iw[None, :]).view(B, N, K).amax(dim=2)
    cm, sm = math.cos(margin), math.sin(margin)
    phi = c * cm - torch.sqrt(torch.clamp(1.0 - c * c, min=L.LOSS_SIN2_FLOOR)) * sm
    phi = torch.where(c > -cm, phi, c - margin * sm)
    hot = F.one_hot(labels, N).bool()
    if topk:
        hardest = c.detach().masked_fill(hot, -float("inf")).topk(topk, dim=1).indices
        c = c + torch.zeros_like(c).scatter_(1, hardest, penalty)
    return F.cross_entropy(scale * torch.where(hot, phi, c), labels, label_smoothing=eps)


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if "cuda" in str(e.device_type).lower() and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception:                                              # no device tracing here: the figure is left out
        return None


def block(B, N, a, dev, gen):
    margin, scale, pen, eps = 0.2, 30.0, 0.06, 0.1
    labels = torch.randint(0, N, (B,), device=dev, generator=gen)
    l32 = labels.to(torch.int32)
    gl = torch.full((B,), 1.0 / B, device=dev)
    loss, pred, sub_y = torch.empty((B,), device=dev), torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)
    lse = torch.empty((B,), dtype=torch.float64, device=dev)
    ix = torch.rand((B,), device=dev, generator=gen) * 0.01 + 0.04           # |x| ~ sqrt(512)
    dix = torch.empty_like(ix)
    res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), B=B, N=N, kind="aam", margin=margin, scale=scale, reps=a.reps,
               regions=a.regions)
    fns = {}
    state = {}
    for name, K, topk in (("off", 1, 0), ("on", 2, 5), ("topk64", 2, 64)):
        z = torch.randn((B, N * K), device=dev, generator=gen) * 22.0         # x . w of unit-variance x and w at D = 512
        iw = torch.rand((N * K,), device=dev, generator=gen) * 0.01 + 0.04
        hard = torch.empty((B, max(topk, 1)), dtype=torch.int32, device=dev)
        dz, diw = torch.empty_like(z), torch.empty_like(iw)
        ws = ops.head_workspace(B, N, K, dev)
        p, e = (pen if topk else 0.0), (eps if topk else 0.0)
        state[name] = (z, iw, K, topk, p, e)

        def fwd(z=z, iw=iw, K=K, topk=topk, p=p, e=e, hard=hard, ws=ws):
            ops.head_forward(z, K, l32, ix, iw, "aam", margin, scale, topk, p, e, loss, pred, lse, hard, sub_y, ws)

        def bwd(z=z, iw=iw, K=K, topk=topk, p=p, e=e, hard=hard, ws=ws, dz=dz, diw=diw):
            ops.head_backward(z, K, l32, ix, iw, "aam", margin, scale, topk, p, e, lse, hard, gl, dz, dix, diw, ws)

        fns[f"{name}_head_forward"] = fwd
        if name != "topk64":
            fns[f"{name}_head_backward"] = bwd
        res[f"{name}_workspace_mb"] = ws.numel() / 2 ** 20
    z1, iw1 = state["off"][:2]
    dz1, diw1, ws1 = torch.empty_like(z1), torch.empty_like(iw1), ops.loss_workspace(B, N, dev)
    fns["off_loss_forward"] = lambda: ops.loss_margin_softmax_forward(z1, l32, ix, iw1, "aam", margin, scale, loss, pred, lse, ws1)
    fns["off_loss_backward"] = lambda: ops.loss_margin_softmax_backward(z1, l32, ix, iw1, "aam", margin, scale, lse, gl, dz1, dix, diw1, ws1)
    z2, iw2, K2, topk2 = state["on"][:4]
    tz, tix, tiw = (t.clone().requires_grad_(True) for t in (z2, ix, iw2))
    compose = lambda: torch_rules(tz, tix, tiw, labels, K2, topk2, pen, eps, margin, scale)  # noqa: E731
    kept = compose()
    fns["on_torch_forward"] = compose
    fns["on_torch_backward"] = lambda: torch.autograd.grad(kept, (tz, tix, tiw), retain_graph=True)
    fns["on_head_forward"]()
    torch.cuda.synchronize()
    res["loss_diff"] = abs(loss.double().mean().item() - kept.item())
    res["launches"] = dict(head=3, torch=count_launches(lambda: torch.autograd.grad(compose(), (tz, tix, tiw))))
    # the order matters to the lse the backward calls read: each backward follows its own forward in `fns`
    order = ["off_loss_forward", "off_loss_backward", "off_head_forward", "off_head_backward", "on_head_forward", "on_head_backward",
             "on_torch_forward", "on_torch_backward", "topk64_head_forward"]
    for k, v in alternate({k: fns[k] for k in order}, a.reps, a.regions).items():
        res[k + "_ms"] = v
    med = lambda k: res[k + "_ms"][0]  # noqa: E731
    res["off_step_vs_loss"] = (med("off_head_forward") + med("off_head_backward")) / (med("off_loss_forward") + med("off_loss_backward"))
    res["on_step_vs_torch"] = (med("on_head_forward") + med("on_head_backward")) / (med("on_torch_forward") + med("on_torch_backward"))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(3)
    for B in (64, 512):
        block(B, 7323, a, dev, gen)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
