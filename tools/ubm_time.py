"""Times the full form of ktf_gmm_acc_f64 (fp64 MFMA, [1, x]^T diag(p) [1, x] per bucket: occ, mean_acc and cov_acc in one product)
against ktf_ivector_acc_second_order (one workgroup per Gaussian, fp64 VALU: the second-order term alone) on the same (frame, slot)
pairs: F frames, n slots, I Gaussians, D dims, posteriors of a random diagonal UBM (ktf_ivector_post_f32). The two are timed in
turn, alternating, after a warm-up of each; device events around `inner` calls per sample. Prints one JSON line with the median and
the spread of each, and the diagonal form and the bucketing alone for scale.

    python tools/ubm_time.py [--F 200000] [--n 20] [--I 2048] [--D 72] [--reps 7] [--inner 3]
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kaldi-tflite_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import _ivector_ref as R                                        # noqa: E402
from kaldi_tflite_amd import ops                                # noqa: E402


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--F", type=int, default=200000)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--I", type=int, default=2048)
    ap.add_argument("--D", type=int, default=72)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    a = ap.parse_args()
    dev = "cuda:0"
    rng = np.random.default_rng(1)
    (w, mi, iv), _ = R.random_models(rng, a.I, a.D, 2, full_sigma=False)
    gc = (np.log(w) - 0.5 * a.D * np.log(2 * np.pi) + 0.5 * np.log(iv).sum(1) - 0.5 * (mi * mi / iv).sum(1)).astype(np.float32)
    W = torch.as_tensor(np.ascontiguousarray(np.concatenate([mi.T, -0.5 * iv.T]).astype(np.float32)), device=dev)
    x = (torch.randn((a.F, a.D), device=dev) * 1.3).contiguous()
    gauss, post = ops.ivector_post(x, W, torch.as_tensor(gc, device=dev), a.n, 0.025)
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)  # noqa: E731
    occ, mean, cov, var, ssec = z(a.I), z(a.I, a.D), z(a.I, a.D, a.D), z(a.I, a.D), z(a.I, a.D, a.D)
    jobs = {"gmm_acc_full_mfma": lambda: ops.gmm_acc(x, gauss, post, occ, mean, cov),
            "ivector_acc_second_order_valu": lambda: ops.ivector_acc_second_order(x, gauss, post, 1.0, ssec),
            "gmm_acc_diag": lambda: ops.gmm_acc(x, gauss, post, occ, mean, var)}
    for fn in jobs.values():                                    # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in jobs}
    for _ in range(a.reps):                                     # alternating
        for k, fn in jobs.items():
            ms[k].append(timed(fn, a.inner))
    pairs = int((gauss >= 0).sum())
    cnt = torch.bincount(gauss[gauss >= 0].long(), minlength=a.I)
    out = dict(F=a.F, n=a.n, I=a.I, D=a.D, pairs=pairs, largest_bucket=int(cnt.max()), empty_buckets=int((cnt == 0).sum()))
    for k, v in ms.items():
        v = sorted(v)
        out[k] = dict(median_ms=round(v[len(v) // 2], 4), min_ms=round(v[0], 4), max_ms=round(v[-1], 4))
    out["flops_full"] = 2.0 * pairs * (a.D + 1) * (a.D + 2) / 2
    out["gmm_acc_full_tflops"] = round(out["flops_full"] / (out["gmm_acc_full_mfma"]["median_ms"] * 1e-3) / 1e12, 3)
    out["cov_acc_vs_Ssec_rel"] = float(((cov - ssec).abs().max() / ssec.abs().max()))     # the same sums, another order
    print(json.dumps(out))


if __name__ == "__main__":
    main()
