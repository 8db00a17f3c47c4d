#!/usr/bin/env python3
"""Times every instantiation of the fp32 and bf16-pair TDNN kernels in isolation (tools/gemm_layers.py does the 16-bit families): the
sitw layer shapes at the batch sizes that reach each kernel -- one 998-frame utterance for the small tiles, 5 x 200 frames for the
64 x 64 ones, a 96-wide input for the K-step-32 form, tdnn6 of one utterance for the row-vector kernel, 64 x 300 frames for the
128 x 128 tiles (DMA-staged and, with KTF_TDNN_REF_TILES, register-staged). One line per kernel: median / min / max ms of REGIONS
regions of ITERS launches, and the name ktf_tdnn_last_kernel() reports.   usage: [KTF_LIBRARY=...] tdnn32_time.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kaldi-tflite_amd")):
    sys.path.insert(0, p)
import torch
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L, ops

ITERS, REGIONS = int(os.environ.get("ITERS", 50)), int(os.environ.get("REGIONS", 7))
dev = torch.device("cuda", 0)
C3 = [-2, 0, 2]
# (B, T, din, units, context, pair operands, pooled, flags)
SHAPES = [(1, 998, 512, 512, C3, x4, False, 0) for x4 in (False, True)] + [(1, 998, 512, 1500, [0], x4, x4, 0) for x4 in (False, True)]
SHAPES += [(5, 200, 512, 512, [0], x4, False, 0) for x4 in (False, True)] + [(1, 998, 96, 512, C3, x4, False, 0) for x4 in (False, True)]
SHAPES += [(1, 1, 3000, 512, [0], False, False, 0)]
SHAPES += [(64, 300, 512, 512, C3, False, False, f) for f in (0, L.TDNN_REF_TILES)] + [(1, 998, 512, 512, C3, False, False, L.TDNN_REF_TILES)]

for B, T, din, units, ctx, x4, pooled, flags in SHAPES:
    t = ktf.layers.TDNN(units, context=ctx, activation="relu")
    t.build((B, T, din))
    gemm = L.GEMM_BF16X4 if x4 else L.GEMM_F32
    x = torch.zeros((B, T, ops.round_up(din, 32)), device=dev)
    x[:, :, :din] = torch.randn((B, T, din), device=dev)
    x = ops.pair_encode(x) if x4 else x
    w, w_lo, bias = t.device_weights(dev, gemm)
    d = t.desc(gemm, L.PAIR if x4 else torch.float32, torch.float32, flags=flags | (L.TDNN_DET_STATS if pooled else 0))
    if pooled:
        sums = torch.zeros((B, ops.tdnn_stats_slots(T, gemm), 2, units), dtype=torch.float64, device=dev)
        f = lambda: ops.tdnn_stats(x, None, d, w, w_lo, bias, None, None, sums, zero=False)
    else:
        y = torch.zeros((B, T, units), device=dev)
        f = lambda: ops.tdnn(x, None, d, w, w_lo, bias, None, None, y)
    for _ in range(5):
        f()
    ms = []
    for _ in range(REGIONS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(ITERS):
            f()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e) / ITERS)
    ms.sort()
    print(f"{ops.last_kernel()}{' pooled' if pooled else ''} B={B} T={T} {len(ctx)}x{din}->{units}: {ms[len(ms) // 2]:.4f} ms (min {ms[0]:.4f}, max {ms[-1]:.4f})")
