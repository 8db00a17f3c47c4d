"""One full VBx iteration (speaker update + log-likelihoods + forward-backward + bound) on synthetic data, the HIP
path against a torch fp64 restatement of the same iteration on the same GPU, at 64 recordings x 2000 windows, D = 128, K = 10. The two
are timed in alternating regions after a warm-up of both, each region `--reps` (HIP) / `--torch-reps` (torch) iterations between two
device events; the figures are the median / min / max over `--regions` regions, the ratio is torch's median over HIP's, and
`hip_wins` says whether HIP's slowest region still beats torch's fastest. The restatement keeps the recordings as one (N, T, .) batch
and walks the HMM in the scaled domain, a few torch kernels per window. Before timing, one iteration of each is compared (gamma, pi,
ELBO). The stages' own times and their achieved bytes/s (the bytes the algorithm needs over the time) follow; one JSON line.

    python tools/bench_vbx.py [--N 64] [--T 2000] [--D 128] [--K 10] [--reps 20] [--torch-reps 1] [--regions 5]"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-tflite_amd"))
from kaldi_tflite_amd import ops  # noqa: E402


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


def torch_iteration(gamma, pi, rho, G, phi, Fa, Fb, lp):
    """gamma (N, T, K), pi (N, K), rho (N, T, D), G (N, T) -> gamma, pi, elbo (N)."""
    f = Fa / Fb
    Nk = gamma.sum(1)
    invL = 1.0 / (1.0 + f * Nk[:, :, None] * phi)
    alpha = f * invL * torch.bmm(gamma.transpose(1, 2), rho)
    c = 0.5 * ((invL + alpha * alpha) * phi).sum(2)
    kl = 0.5 * (torch.log(invL) - invL - alpha * alpha + 1.0).sum(2)
    lls = Fa * (torch.bmm(rho, alpha.transpose(1, 2)) - c[:, None, :] + G[:, :, None])
    N, T, K = lls.shape
    mx = lls.max(2, keepdim=True).values
    e = torch.exp(lls - mx)
    ah = torch.empty_like(e)
    cb = torch.zeros((N, T), dtype=e.dtype, device=e.device)
    a = pi * e[:, 0]
    s = a.sum(1, keepdim=True)
    a = a / s
    tll = torch.log(s[:, 0]) + mx[:, 0, 0]
    ah[:, 0] = a
    for t in range(1, T):
        sa = a.sum(1, keepdim=True)
        v = e[:, t] * (lp * a + (1.0 - lp) * sa * pi)
        s = v.sum(1, keepdim=True)
        a = v / s
        tll = tll + torch.log(s[:, 0]) + mx[:, t, 0]
        ah[:, t] = a
        cb[:, t] = (1.0 - lp) * sa[:, 0] / s[:, 0]
    bt = torch.ones_like(a)
    out = torch.empty_like(e)
    acc = torch.zeros_like(a)
    for t in range(T - 1, -1, -1):
        eb = e[:, t] * bt
        ab = ah[:, t] * bt
        tot = ab.sum(1, keepdim=True)
        out[:, t] = ab / tot
        acc = acc + (out[:, t] if t == 0 else cb[:, t, None] * pi * eb / tot)
        o = lp * eb + (1.0 - lp) * (pi * eb).sum(1, keepdim=True)
        bt = o / o.sum(1, keepdim=True)
    return out, acc / acc.sum(1, keepdim=True), tll + Fb * kl.sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=1)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    N, T, D, K = a.N, a.T, a.D, a.K
    Fa, Fb, lp = 0.3, 17.0, 0.99
    g = torch.Generator(device=dev).manual_seed(1)
    phi = torch.rand((D,), dtype=torch.float64, device=dev, generator=g) * 7.95 + 0.05
    means = torch.randn((N, K, D), dtype=torch.float64, device=dev, generator=g) * phi.sqrt()
    spk = torch.randint(0, K, (N, T // 20 + 1), device=dev, generator=g).repeat_interleave(20, 1)[:, :T]
    x = torch.gather(means, 1, spk[:, :, None].expand(N, T, D)) + torch.randn((N, T, D), dtype=torch.float64, device=dev, generator=g)
    gamma = torch.softmax(torch.randn((N * T, K), dtype=torch.float64, device=dev, generator=g), 1)
    pi = torch.full((N, K), 1.0 / K, dtype=torch.float64, device=dev)
    off = torch.arange(N + 1, dtype=torch.int32, device=dev) * T
    zero = torch.zeros((N,), dtype=torch.float64, device=dev)
    rho, G = ops.vbx_prepare(x.reshape(N * T, D), phi)

    def hip():
        alpha, _, c, kl = ops.vbx_speaker_update(gamma, rho, phi, Fa / Fb, off)
        lls = ops.vbx_loglike(rho, G, alpha, c, Fa, off)
        gn, pn, tll = ops.vb_forward_backward(lls, off, pi, lp)
        return gn, pn, ops.vb_bound(zero, tll, kl * Fb, 0.0)

    def ref():
        return torch_iteration(gamma.reshape(N, T, K), pi, rho.reshape(N, T, D), G.reshape(N, T), phi, Fa, Fb, lp)

    h, r = hip(), ref()                                             # (the warm-up of both, too)
    res = dict(build=ops.build_id(), N=N, T=T, D=D, K=K, reps=a.reps, torch_reps=a.torch_reps, regions=a.regions)
    res["gamma_diff"] = float((h[0].reshape(N, T, K) - r[0]).abs().max())
    res["pi_diff"] = float((h[1] - r[1]).abs().max())
    res["elbo_rel_diff"] = float(((h[2] - r[2]).abs() / r[2].abs()).max())
    hip()
    torch.cuda.synchronize()
    th, tt = [], []
    for _ in range(a.regions):                                      # alternating: both see the same neighbours on the machine
        th.append(region(hip, a.reps))
        tt.append(region(ref, a.torch_reps))
    res["hip_iteration_ms"], res["torch_iteration_ms"] = stats(th), stats(tt)
    res["torch_over_hip"] = res["torch_iteration_ms"][0] / res["hip_iteration_ms"][0]
    res["hip_wins"] = max(th) < min(tt)
    alpha, _, c, kl = ops.vbx_speaker_update(gamma, rho, phi, Fa / Fb, off)
    lls = ops.vbx_loglike(rho, G, alpha, c, Fa, off)
    stages = dict(update=lambda: ops.vbx_speaker_update(gamma, rho, phi, Fa / Fb, off), loglike=lambda: ops.vbx_loglike(rho, G, alpha, c, Fa, off),
                  forward_backward=lambda: ops.vb_forward_backward(lls, off, pi, lp))
    for k, fn in stages.items():
        fn()
        torch.cuda.synchronize()
        res[k + "_ms"] = stats([region(fn, a.reps) for _ in range(a.regions)])
    S = N * T
    nch = N * ((T + 255) // 256)
    need = dict(update=8 * (S * (D + K) + 2 * nch * 16 * (D + 16) + 2 * N * K * D), loglike=8 * (S * (D + 1 + K) + N * K * (D + 1)))
    for k, b in need.items():                                       # the bytes the stage must move, over its median time
        res[k + "_gbytes_per_s"] = b / res[k + "_ms"][0] / 1e6
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
