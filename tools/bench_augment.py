"""Waveform augmentation at the recipes' shape: B = 1024 utterances of 10 s at 16 kHz, each convolved with one
of 8 RIRs of `--rir-s` seconds (0.5 and 1.0) and mixed with one babble-style plan of additives, against what a user would write
today: a full-length `torch.fft` convolution on the same GPU (one rfft of the zero-padded batch shared by the full and the early
filter, the RIRs' rffts, product, irfft), then the same adds, power normalisation and window in torch, with everything that does
not depend on the signals (row lists, noise offsets, SNR factors) made once outside the timed call. The like-for-like figure is
the convolution alone (`convolve_ms` against `torch_fft_convolution_ms`, ratio `torch_fft_over_convolve`); the whole-call ratio
also measures how the baseline mixes, which a user could write in other ways. Both are timed in alternating regions after a warm-up of
both, each region `--reps` calls between two device events; the figures are the median / min / max over `--regions` regions,
utterances/s from the median, and `new_wins` says whether the new path's slowest region still beats the baseline's fastest.
Achieved GB/s is the convolution's algorithmic traffic (x read once, X written and read AUG_J-amortised, H from the
L2, y written, read, and the output written) over the new path's median time. The stages alone follow (the two library calls
on the whole batch in one workspace, the call without additives, the baseline's convolution); one JSON line per RIR length. Reported, not gated.

    python tools/bench_augment.py [--B 1024] [--seconds 10] [--rir-s 0.5 1.0] [--no-additives] [--reps 5] [--regions 5]"""

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

FS = 16000


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


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rir-s", type=float, nargs="+", default=[0.5, 1.0])
    ap.add_argument("--rirs", type=int, default=8)
    ap.add_argument("--no-additives", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--regions", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda:0"
    B, n = a.B, int(a.seconds * FS)
    P = ops.aug_partition()
    rng = np.random.default_rng(1)
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn((B, n), device=dev, generator=g) * 3000.0
    noises = ktf.augment.NoiseBank([(rng.standard_normal(int(s * FS)) * 300).astype(np.float32) for s in (3.0, 7.5, 12.0, 20.0)], FS)
    plan = None if a.no_additives else ktf.augment.plan_additives("babble", [a.seconds] * B, noises.lengths_s, seed=3)
    for rir_s in a.rir_s:
        Lh = int(rir_s * FS)
        hs = []
        for r in range(a.rirs):
            h = rng.standard_normal(Lh) * np.exp(-6.0 * np.arange(Lh) / Lh)
            h[40 + r] = np.abs(h).max() * 1.5
            hs.append(h.astype(np.float32))
        bank = ktf.augment.RirBank(hs, FS)
        ids = np.arange(B) % a.rirs
        ids_dev = torch.as_tensor(ids, device=dev)
        H = torch.as_tensor(np.stack(hs), device=dev)
        peaks = torch.as_tensor(bank.peak.astype(np.int64), device=dev)
        ylen = n + Lh - 1
        nfft = 1 << int(np.ceil(np.log2(ylen)))

        def new():
            return ktf.augment.augment(x, rirs=bank, rir_ids=ids, noises=noises, additives=plan)[0]

        # what the baseline needs that does not change from call to call, made once: the early filters, and per position j in the
        # rows' additive lists the rows that have one, their noise ids, offsets, lengths and SNRs on the device
        early = torch.zeros_like(H)
        for r in range(a.rirs):
            k = int(bank.peak[r])
            early[r, max(0, k - 16):k + 800] = H[r, max(0, k - 16):k + 800]
        positions = []
        for j in range(max(len(r) for r in plan) if plan is not None else 0):
            rows = [b for b in range(B) if len(plan[b]) > j]
            nid = torch.as_tensor([plan[b][j][0] for b in rows], device=dev)
            snr = torch.as_tensor([plan[b][j][1] for b in rows], device=dev, dtype=torch.float64)
            positions.append((torch.as_tensor(rows, device=dev), noises.offsets_dev[nid],
                              noises.offsets_dev[nid + 1] - noises.offsets_dev[nid], 10.0 ** (-snr / 10.0)))
        t_n = torch.arange(n, device=dev)

        def baseline():
            Xf = torch.fft.rfft(x, n=nfft)                              # shared by the full and the early filter
            y = torch.fft.irfft(Xf * torch.fft.rfft(H, n=nfft)[ids_dev], n=nfft)[:, :ylen]
            p_before = (x.double() ** 2).mean(1)
            if plan is not None:
                e = torch.fft.irfft(Xf * torch.fft.rfft(early, n=nfft)[ids_dev], n=nfft)[:, :ylen]
                p_sig = (e.double() ** 2).sum(1) / (n + 816 - 1)
                for rows, off, m, factor in positions:                  # one batched add per position in the rows' lists
                    ev = noises.flat[off[:, None] + t_n[None, :] % m[:, None]]
                    gain = torch.sqrt(factor * p_sig[rows] / (ev.double() ** 2).mean(1))
                    y[rows, :n] += gain[:, None].float() * ev
            scale = torch.sqrt(p_before / (y.double() ** 2).mean(1)).float()
            idx = peaks[ids_dev][:, None] + t_n[None, :]
            return torch.gather(y, 1, idx) * scale[:, None]

        got, want = new(), baseline()                               # (the warm-up of both, too)
        res = dict(build=ops.build_id(), gpu=torch.cuda.get_device_name(0), B=B, seconds=a.seconds, rir_s=rir_s, taps=Lh, P=P,
                   additives=0 if plan is None else sum(len(r) for r in plan), reps=a.reps, regions=a.regions, baseline_nfft=nfft)
        res["max_rel_diff_vs_baseline"] = float(((got - want).abs().amax(1) / want.abs().amax(1)).max())
        res["new_peak_mb"], res["baseline_peak_mb"] = peak_mb(new), peak_mb(baseline)
        tn, tb = [], []
        for _ in range(a.regions):                                  # alternating: both see the same neighbours on the machine
            tn.append(region(new, a.reps))
            tb.append(region(baseline, a.reps))
        res["new_ms"], res["baseline_ms"] = stats(tn), stats(tb)
        res["new_utt_per_s"], res["baseline_utt_per_s"] = B / res["new_ms"][0] * 1e3, B / res["baseline_ms"][0] * 1e3
        res["baseline_over_new"] = res["baseline_ms"][0] / res["new_ms"][0]
        res["new_wins"] = max(tn) < min(tb)
        # algorithmic bytes of one call (fp32): x in, X out, X in twice (full and early pass, each block once per workgroup that
        # needs it: (AUG_J + partitions - 1) / AUG_J times), y out, y in and out again in the adds, y in and the output out
        nxb, np_full, J = -(-n // P) + 1, -(-Lh // P), 4
        xbytes = nxb * 2 * P * 4
        per_row = n * 4 + xbytes + xbytes * (J + np_full - 1) / J + xbytes * (J + 1 - 1) / J + ylen * 4 * (1 + (2 if plan else 1) + 1) + n * 4
        res["algorithmic_gb"] = B * per_row / 1e9
        res["new_gb_per_s"] = res["algorithmic_gb"] / (res["new_ms"][0] * 1e-3)
        # the two library calls alone, on one chunk of the batch as augment() issues them
        nn, idn = np.full(B, n, np.int32), ids.astype(np.int32)
        n_dev, id_dev = torch.as_tensor(nn, device=dev), torch.as_tensor(idn, device=dev)
        ws = torch.empty((ops.aug_workspace_bytes(nn, idn, bank.lengths, FS, 0),), dtype=torch.uint8, device=dev)
        st = torch.empty((B, 4), dtype=torch.float64, device=dev)
        out = torch.empty((B, n), dtype=torch.float32, device=dev)
        zero_off = np.zeros(B + 1, np.int32)
        zero_dev = torch.as_tensor(zero_off, device=dev)
        stage = dict(
            convolve=lambda: ops.aug_convolve(x, nn, n_dev, idn, id_dev, bank.lengths, FS, bank.taps, bank.offsets_dev, bank.meta,
                                              bank.spectra, bank.tables, 0, st, ws),
            mix_no_additives=lambda: ops.aug_mix(nn, n_dev, idn, id_dev, bank.lengths, FS, bank.meta, zero_off, zero_dev,
                                                 np.zeros((0, 4), np.int32), None, None, np.zeros(1, np.int64), None, True, True, 0.0, out,
                                                 st, ws),
            augment_no_additives=lambda: ktf.augment.augment(x, rirs=bank, rir_ids=ids),
            torch_fft_convolution=lambda: torch.fft.irfft(torch.fft.rfft(x, n=nfft) * torch.fft.rfft(H, n=nfft)[ids_dev], n=nfft))
        if plan is not None:
            add_off, adds = ktf.augment._additive_rows(plan, B, FS)
            off_dev, adds_dev = torch.as_tensor(add_off, device=dev), torch.as_tensor(adds, device=dev)
            ws_a = torch.empty((ops.aug_workspace_bytes(nn, idn, bank.lengths, FS, adds.shape[0]),), dtype=torch.uint8, device=dev)
            ops.aug_convolve(x, nn, n_dev, idn, id_dev, bank.lengths, FS, bank.taps, bank.offsets_dev, bank.meta, bank.spectra, bank.tables,
                             adds.shape[0], st, ws_a)
            # (y grows from call to call here: the adds land on the same workspace again; the time does not depend on the values)
            stage["mix_with_additives"] = lambda: ops.aug_mix(nn, n_dev, idn, id_dev, bank.lengths, FS, bank.meta, add_off, off_dev, adds,
                                                              adds_dev, noises.flat, noises.offsets, noises.offsets_dev, True, True, 0.0,
                                                              out, st, ws_a)
        for k, fn in stage.items():
            fn()
            torch.cuda.synchronize()
            res[f"{k}_ms"] = stats([region(fn, a.reps) for _ in range(a.regions)])
        conv_gb = B * (n * 4 + xbytes + xbytes * (J + np_full - 1) / J + xbytes + ylen * 4) / 1e9
        res["torch_fft_over_convolve"] = res["torch_fft_convolution_ms"][0] / res["convolve_ms"][0]
        res["convolve_algorithmic_gb"], res["convolve_gb_per_s"] = conv_gb, conv_gb / (res["convolve_ms"][0] * 1e-3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
