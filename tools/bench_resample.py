"""Sample-rate conversion at the recipes' shape: B = 1024 rows of 10 s, 16000 -> 8000, 44100 -> 16000,
48000 -> 8000 and 16000 -> 17600 (speed 10/11), int16 in and out and fp32 in and out. `kernel_ms` is ktf_rs_resample alone on a
preallocated output, `call_ms` the whole Resampler call (lengths, allocation, launch). The yardstick on the same GPU is what a user
would write in torch: one strided fp32 `conv1d` per phase over the zero-padded batch, written into the interleaved output
(`torch_ms`; for int16 it includes the conversions in and out). Regions alternate after a warm-up of both, each `--reps` calls
between two device events; median / min / max over `--regions` regions. Achieved bytes/s is the algorithmic traffic (every input
sample read once, every output sample written once) over the kernel's median time, against the 6.3 TB/s the part sustains;
`fma_per_s` is the fp64 fused multiply-adds of rule 4 over the same time. One JSON line per case. Reported, not gated.

    python tools/bench_resample.py [--B 1024] [--seconds 10] [--reps 5] [--regions 5] [--pairs 16000:8000 ...]"""

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

HBM_BYTES_PER_S = 6.3e12
PAIRS = ["16000:8000", "44100:16000", "48000:8000", "16000:17600"]


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


def torch_polyphase(rs, n, m, dev):
    """The plan as one strided conv1d per phase -> fn(x (B, n) fp32) -> (B, m) fp32."""
    first, taps = rs.first.astype(np.int64), rs.taps.astype(np.int64)
    w = torch.as_tensor(rs.weights, device=dev)
    counts = [len(range(i, m, rs.ou)) for i in range(rs.ou)]
    left = int(max(0, -first.min()))
    right = int(max(0, max(first[i] + (counts[i] - 1) * rs.iu + w.shape[1] for i in range(rs.ou) if counts[i]) - n))

    def fn(x):
        xp = torch.nn.functional.pad(x, (left, right))[:, None, :]
        out = torch.empty((x.shape[0], m), dtype=torch.float32, device=dev)
        for i in range(rs.ou):
            if counts[i]:
                s = int(first[i]) + left
                seg = xp[:, :, s:s + (counts[i] - 1) * rs.iu + w.shape[1]]
                out[:, i::rs.ou] = torch.nn.functional.conv1d(seg, w[i][None, None, :], stride=rs.iu)[:, 0, :counts[i]]
        return out
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--pairs", nargs="+", default=PAIRS)
    a = ap.parse_args()
    dev = "cuda:0"
    for pair in a.pairs:
        fi, fo = (int(v) for v in pair.split(":"))
        rs = ktf.augment.Resampler(fi, fo)
        B, n = a.B, int(a.seconds * fi)
        m = rs.num_out(n)
        g = torch.Generator(device=dev).manual_seed(2)
        xf = torch.randn((B, n), device=dev, generator=g) * 3000.0
        nn = np.full(B, n, np.int32)
        n_dev = torch.as_tensor(nn, device=dev)
        plan_dev = [torch.as_tensor(v, device=dev) for v in (rs.first, rs.taps, rs.weights)]
        poly = torch_polyphase(rs, n, m, dev)
        for i16 in (True, False):
            x = xf.round().clamp(-32768, 32767).to(torch.int16) if i16 else xf
            out = torch.empty((B, m), dtype=x.dtype, device=dev)
            kernel = lambda: ops.rs_resample(x, nn, n_dev, rs.iu, rs.ou, rs.first, rs.taps, *plan_dev, out)  # noqa: E731
            call = lambda: rs(x)[0]  # noqa: E731
            if i16:
                base = lambda: poly(x.float()).round().clamp(-32768, 32767).to(torch.int16)  # noqa: E731
            else:
                base = lambda: poly(x)  # noqa: E731
            got, want = call().float(), base().float()              # (the warm-up of both, too)
            kernel()
            res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), fi=fi, fo=fo, dtype="int16" if i16 else "float32", B=B,
                       n=n, m=m, iu=rs.iu, ou=rs.ou, max_taps=int(rs.taps.max()), tile=ops.rs_tile(), reps=a.reps, regions=a.regions)
            res["max_abs_diff_vs_torch"] = float((got - want).abs().max())
            tk, tc, tb = [], [], []
            for _ in range(a.regions):                              # alternating: all see the same neighbours on the machine
                tk.append(region(kernel, a.reps))
                tc.append(region(call, a.reps))
                tb.append(region(base, a.reps))
            res["kernel_ms"], res["call_ms"], res["torch_ms"] = stats(tk), stats(tc), stats(tb)
            res["torch_over_kernel"] = res["torch_ms"][0] / res["kernel_ms"][0]
            res["kernel_wins"] = max(tk) < min(tb)
            bytes_moved = B * (n + m) * x.element_size()
            res["algorithmic_gb"] = bytes_moved / 1e9
            res["bytes_per_s"] = bytes_moved / (res["kernel_ms"][0] * 1e-3)
            res["of_hbm_rate"] = res["bytes_per_s"] / HBM_BYTES_PER_S
            fmas = B * float(sum(int(rs.taps[s % rs.ou]) for s in range(min(m, rs.ou)))) * m / min(m, rs.ou)
            res["fma_per_s"] = fmas / (res["kernel_ms"][0] * 1e-3)
            print(json.dumps(res), flush=True)
            del out
        del xf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
