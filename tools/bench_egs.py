"""Training batches (include/ktf_egs.h: `ktf.egs.ChunkSampler.batch`, one launch of ktf_egs_sample) next to a
torch composition of the same rules written here -- `randint` for the speaker, `searchsorted` for the count of its utterances of at
least T rows, `rand` and index arithmetic for the utterance and the offset, `index_select` of the B * T rows and the conversion to
fp32 -- on B in {64, 128, 512} x T in {200, 400} x D = 30, for an fp32 and an fp16 bank of 1000 utterances of 400 - 800 rows from
200 speakers. (The composition draws from torch's generator: the same distribution, not the same chunks. Neither pads the columns:
tdnn_affine pads its input itself.)

Per shape and bank dtype, one JSON line: `fused_ms` / `torch_ms` [median, min, max] over `--regions` regions of `--reps` calls
between two device events, the regions of the two alternating after a warm-up of both; `fused_vs_torch` the ratio of the medians
(below 1: faster); `*_launches` the device kernels of one call as torch.profiler counts them (null where it cannot); `*_gbps` the
bytes a batch has to move (B * T * D elements read once and written once as fp32) over the median time. Reported, not gated.

    python tools/bench_egs.py [--D 30] [--reps 20] [--regions 7]"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kaldi-tflite_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import ops  # noqa: E402
from bench_norm import alternate  # noqa: E402

BIG = 1 << 20           # above any utterance length: the key of the composition's searchsorted


def make_view(D, dtype, dev, gen):
    rng = np.random.default_rng(1)
    lens = rng.integers(400, 801, 1000)
    labels = rng.permutation(1000) % 200
    row0 = np.concatenate([[0], np.cumsum(lens)[:-1]])
    storage = torch.randn((int(lens.sum()), D), device=dev, generator=gen).to(dtype)
    return ktf.egs.BankView(row0, lens, labels, list(range(200)), storage=storage)


def torch_batch_fn(view, B, T, gen):
    d = view.device_arrays()
    bank, dev = view.storage, view.storage.device
    n_spk = view.eligible_speakers(T)
    order, off, utts, ulen, row0 = (d[k].long() for k in ("spk_order", "spk_off", "spk_utts", "spk_utt_len", "row0"))
    spk_of = torch.repeat_interleave(torch.arange(view.num_speakers, device=dev), off[1:] - off[:-1])
    key = spk_of * BIG + (BIG - 1 - ulen)                          # ascending: by speaker, then by length descending
    t = torch.arange(T, device=dev)

    def fn():
        s = order[torch.randint(0, n_spk, (B,), device=dev, generator=gen)]
        first = off[s]
        m = torch.searchsorted(key, s * BIG + (BIG - 1 - T), right=True) - first
        k = first + (torch.rand((B,), device=dev, generator=gen) * m).long()
        u = utts[k]
        offset = (torch.rand((B,), device=dev, generator=gen) * (ulen[k] - T + 1)).long()
        rows = (row0[u] + offset)[:, None] + t[None, :]
        feats = bank.index_select(0, rows.reshape(-1)).view(B, T, -1).float()
        return feats, torch.full((B,), T, dtype=torch.int32, device=dev), s.to(torch.int32)
    return fn


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception:                                               # a profiler that cannot run says nothing about the code
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    a = ap.parse_args()
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(3)
    for dtype in (torch.float32, torch.float16):
        view = make_view(a.D, dtype, dev, gen)
        for B in (64, 128, 512):
            for T in (200, 400):
                sampler = ktf.egs.ChunkSampler(view, B, T, T, seed=5)
                steps = iter(range(1 << 40))
                fns = {"fused": lambda: sampler.batch(next(steps)), "torch": torch_batch_fn(view, B, T, gen)}
                feats, lens, labels = fns["fused"]()
                tf, tl, ty = fns["torch"]()
                assert feats.shape == tf.shape and feats.dtype == tf.dtype and lens.tolist() == tl.tolist() and int(labels.min()) >= 0
                res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), B=B, T=T, D=a.D, bank=str(dtype).split(".")[1],
                           bank_mb=view.storage.numel() * view.storage.element_size() / 2 ** 20, reps=a.reps, regions=a.regions)
                for k, v in alternate(fns, a.reps, a.regions).items():
                    res[k + "_ms"] = v
                moved = B * T * a.D * (view.storage.element_size() + 4)
                for k in fns:
                    res[k + "_gbps"] = moved / (res[k + "_ms"][0] * 1e-3) / 1e9
                    res[k + "_launches"] = launches(fns[k])
                res["fused_vs_torch"] = res["fused_ms"][0] / res["torch_ms"][0]
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
