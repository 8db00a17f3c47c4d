#!/usr/bin/env python3
"""Speaker-verification scoring (ktf.verification, PLDA.score_trials) on two synthetic workloads of dimension 128 (the sitw LDA
dimension), vectors drawn around speaker centroids: (a) VoxCeleb1-O-shaped, 4,874 single-utterance models and 37,720 trials;
(b) SRE-shaped, 10,000 speakers x 3 enrollment utterances, 10,000 tests, 2,000,000 trials. For fp64 and fp32: ms per call of
speaker_means, the enrollment transform (with counts), the test transform and score_trials, PLDA.score on (b)'s full M x N block
for comparison, and each kernel's share of the GPU time (torch.profiler): python tools/verif_time.py"""
import collections
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kaldi-tflite_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import bench
import kaldi_tflite_amd as ktf

D = 128


def stage_shares(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    t = collections.Counter()
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower():
            name = ev.name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0].split("<")[0]
            t[name] += ev.device_time_total if hasattr(ev, "device_time_total") else ev.cuda_time_total
    tot = sum(t.values())
    return tot / 1e3, [(k, v / tot) for k, v in t.most_common()] if tot else []


def workload(S, per, N, T, seed):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((S, D)) * 2.0
    raw = torch.as_tensor((np.repeat(cent, per, axis=0) + rng.standard_normal((S * per, D))).astype(np.float32), device="cuda")
    who = rng.integers(0, S, N)
    test = torch.as_tensor(cent[who] + rng.standard_normal((N, D)), device="cuda")
    spk2utt = (np.arange(S + 1) * per, np.arange(S * per))
    tj = rng.integers(0, S, T).astype(np.int32)
    tj[: T // 10] = who[rng.integers(0, N, T // 10)]                       # (a tenth of targets, as it were)
    ti = rng.integers(0, N, T).astype(np.int32)
    return raw, spk2utt, test, torch.as_tensor(tj, device="cuda"), torch.as_tensor(ti, device="cuda")


rng = np.random.default_rng(1)
Tm = rng.standard_normal((D, D)) / np.sqrt(D) + np.eye(D)
mean, psi = rng.standard_normal(D) * 0.1, np.sort(rng.uniform(0.05, 30.0, D))[::-1].copy()
cases = {"a: VoxCeleb1-O 4874 models x 1, 37720 trials": (4874, 1, 4874, 37720),
         "b: SRE 10000 speakers x 3, 10000 tests, 2e6 trials": (10000, 3, 10000, 2_000_000)}
for dtype in (torch.float64, torch.float32):
    plda = ktf.layers.PLDA(D, mean, Tm, psi, dtype=dtype)
    for name, (S, per, N, T) in cases.items():
        raw, spk2utt, test, tj, ti = workload(S, per, N, T, seed=S + T)
        means, nu = ktf.verification.speaker_means(raw, spk2utt)
        nd = nu.to(dtype)
        e_tr = plda.transform(means, num_examples=nd)
        y_tr = plda.transform(test)
        ms = {
            "speaker_means": bench._time_ms(torch, lambda: ktf.verification.speaker_means(raw, spk2utt), 20),
            "transform_n (enroll)": bench._time_ms(torch, lambda: plda.transform(means, num_examples=nd), 20),
            "transform (test)": bench._time_ms(torch, lambda: plda.transform(test), 20),
            "score_trials": bench._time_ms(torch, lambda: plda.score_trials(y_tr, e_tr, tj, ti, enroll_num_examples=nd), 10),
        }
        line = ", ".join(f"{k} {v:.3f} ms" for k, v in ms.items())
        if T > 1_000_000:
            ms_blk = bench._time_ms(torch, lambda: plda.score(y_tr, e_tr, enroll_num_examples=nd), 5)
            line += f" | full {N} x {S} block score_n {ms_blk:.3f} ms ({'trials faster' if ms['score_trials'] < ms_blk else 'block faster'})"
        gpu_ms, shares = stage_shares(lambda: plda.score_trials(y_tr, e_tr, tj, ti, enroll_num_examples=nd))
        print(f"{str(dtype)[6:]:7s} {name}: {line}", flush=True)
        print(f"        score_trials kernels {gpu_ms:.3f} ms: " + ", ".join(f"{k} {s:.1%}" for k, s in shares[:6]), flush=True)
