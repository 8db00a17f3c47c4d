"""Times i-vector extraction (ktf.layers.IvectorExtractor) on one GPU: B utterances x T frames at I Gaussians, D feature dims, for
each i-vector dim S given; per stage (posteriors = ktf_ivector_post_f32; extract = ktf_ivector_extract: stats, linear and quadratic
terms, solve) and end to end as i-vectors/s, batch-1 latency, and the host NumPy restatement (tests/_ivector_ref.py) on a few
utterances for scale. The model is random (built on the device: no files). Prints one JSON line per S.
--full-ubm adds a random SPD full-covariance UBM (the diagonal one is its toDiag()): the recipe's posterior stage, timed as the
preselection (ktf_ivector_post_f32 with min_post 0), the new stage (ktf_fgmm_post_f32) and the whole call, next to the diagonal
posterior stage on the same frames.

--train times extractor training on the same batch: one `accumulate`, synchronised, and its parts: the
posterior stage, the stages shared with extraction (the `extract` figure), everything ktf_ivector_acc_stats launches (shared stages,
covariance and scatter, the A^T B accumulations), the R job of ktf_atb_f64 alone on one chunk (TFLOP/s and its fraction of the 78.6 TF
fp64 MFMA rate), the second-order statistics, and one ivector_extractor_est (host NumPy; --no-est skips it).

    python tools/ivector_time.py [--B 1024] [--T 1000] [--I 2048] [--D 60] [--S 400 600] [--reps 3] [--full-ubm] [--train [--no-est]]
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kaldi-tflite_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import _fgmm_ref as G                                           # noqa: E402
import _ivector_ref as R                                        # noqa: E402
import kaldi_tflite_amd as ktf                                  # noqa: E402
from kaldi_tflite_amd import _lib as L, ops                    # noqa: E402
from kaldi_tflite_amd.io import KaldiDiagGmmReader, KaldiFullGmmReader, KaldiIvecExtractorReader   # noqa: E402


def full_model(I, D, seed=3):
    """A random SPD full UBM (tests/_fgmm_ref.random_full_ubm) as a reader object, no file round trip."""
    (w, mic, ic), _ = G.random_full_ubm(np.random.default_rng(seed), I, D)
    full = KaldiFullGmmReader.__new__(KaldiFullGmmReader)
    full.path, full.storedGconsts = "<random>", None
    full.weights, full.means_invcovars, full.inv_covars = w, mic, ic
    full.numGauss, full.featDim = I, D
    full.gconsts = full.computeGconsts()
    return full


def model(I, D, S, dev, seed=1, full=None):
    """Reader objects filled directly (no file round trip): sigmaInvM and U derived on the device in fp64."""
    rng = np.random.default_rng(seed)
    (w, mi, iv), _ = R.random_models(rng, I, D, 2, full_sigma=False)
    if full is not None:
        ubm = full.toDiag()
        mi, iv = ubm.means_invvars, ubm.inv_vars
    else:
        ubm = KaldiDiagGmmReader.__new__(KaldiDiagGmmReader)
        ubm.weights, ubm.means_invvars, ubm.inv_vars, ubm.numGauss, ubm.featDim = w, mi, iv, I, D
        ubm.gconsts = ubm.computeGconsts()
    g = torch.Generator(device=dev).manual_seed(seed)
    M = torch.randn((I, D, S), generator=g, device=dev, dtype=torch.float64) * 0.3
    M[:, :, 0] = torch.as_tensor(mi / iv, device=dev, dtype=torch.float64) / 100.0
    sig = torch.diag_embed(torch.rand((I, D), generator=g, device=dev, dtype=torch.float64) + 0.5)
    sim = sig @ M
    r, c = np.tril_indices(S)
    U = torch.empty((I, S * (S + 1) // 2), dtype=torch.float64, device=dev)
    for i0 in range(0, I, 128):
        U[i0:i0 + 128] = (M[i0:i0 + 128].transpose(1, 2) @ sim[i0:i0 + 128])[:, r, c]
    ie = KaldiIvecExtractorReader.__new__(KaldiIvecExtractorReader)
    ie.w, ie.wVec, ie.priorOffset = np.zeros((0, 0)), np.full(I, 1.0 / I), 100.0
    ie.numGauss, ie.featDim, ie.ivecDim = I, D, S
    ie.M, ie.sigmaInv = M.cpu().numpy(), sig.cpu().numpy()
    ie.sigmaInvM, ie.U = sim.cpu().numpy(), U.cpu().numpy()
    return ie, ubm


def timed(fn, reps):
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def train_times(a, layer, ie, x, flat, off, g, p, t_call):
    """The --train figures (milliseconds unless named otherwise)."""
    dev = flat.device
    I, D, S = layer.numGauss, layer.featDim, layer.ivecDim
    P = S * (S + 1) // 2
    _, _, sim, U, _ = layer._consts(dev)
    st = ktf.training.IvectorStats(ie)
    layer.accumulate(st, x[:2])                                                 # warm-up, allocates the accumulators
    chunks = layer._train_chunks(a.B)
    posts = lambda lo, hi: (g[lo:hi], p[lo:hi])                                 # noqa: E731

    def acc_stats():
        for b0, b1 in chunks:
            lo, hi = int(off[b0]), int(off[b1])
            o = torch.as_tensor((off[b0:b1 + 1] - lo).astype(np.int32), device=dev)
            ops.ivector_acc_stats(flat[lo:hi], o, g[lo:hi], p[lo:hi], layer.posteriorScale, sim, U, layer.priorOffset, st.gamma, st.Y, st.R,
                                  st.ivector_sum, st.ivector_scatter, st.totals)

    def second():
        for b0, b1 in chunks:
            lo, hi = int(off[b0]), int(off[b1])
            ops.ivector_acc_second_order(flat[lo:hi], g[lo:hi], p[lo:hi], layer.posteriorScale, st.Ssec)
    t_stats, _ = timed(acc_stats, a.reps)
    t_sec, _ = timed(second, a.reps)
    t_from, _ = timed(lambda: layer._accumulate(st, flat, off, posts), a.reps)
    t_acc, _ = timed(lambda: layer.accumulate(st, x), a.reps)
    bc = chunks[0][1] - chunks[0][0]
    gen = torch.Generator(device=dev).manual_seed(5)
    A = torch.rand((bc, I), generator=gen, device=dev, dtype=torch.float64)
    Bm = torch.rand((bc, P), generator=gen, device=dev, dtype=torch.float64)
    t_atb, _ = timed(lambda: ops.atb_f64(A, Bm, st.R), a.reps)
    tf = 2.0 * I * P * bc / t_atb / 1e12
    out = {"train_chunks": len(chunks), "chunk_utts": bc, "accumulate_ms": round(t_acc * 1e3, 3),
           "accumulate_from_posteriors_ms": round(t_from * 1e3, 3), "acc_stats_ms": round(t_stats * 1e3, 3),
           "second_order_ms": round(t_sec * 1e3, 3), "atb_R_job_ms": round(t_atb * 1e3, 3), "atb_R_tflops": round(tf, 2),
           "atb_R_fraction_of_78.6": round(tf / 78.6, 3), "accumulate_over_call": round(t_acc / t_call, 2)}
    del A, Bm
    if not a.no_est:
        st2 = ktf.training.IvectorStats(ie)
        layer.accumulate(st2, x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = st2.host()
        t_copy = time.perf_counter() - t0
        new = ktf.training.ivector_extractor_est(ie, st2, gaussian_min_count=0.0)
        out.update(est_s=round(new.estInfo["seconds"], 3), est_backend=new.estInfo["backend"], est_copy_to_host_s=round(t_copy, 3),
                   objf=st2.objf())
        del h, st2
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--I", type=int, default=2048)
    ap.add_argument("--D", type=int, default=60)
    ap.add_argument("--S", type=int, nargs="+", default=[400, 600])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-utts", type=int, default=2)
    ap.add_argument("--full-ubm", action="store_true")
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--no-est", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L.load()
    full = full_model(a.I, a.D) if a.full_ubm else None
    for S in a.S:
        ie, ubm = model(a.I, a.D, S, dev, full=full)
        layer = ktf.layers.IvectorExtractor(ie, ubm, full_ubm=full)
        rng = np.random.default_rng(2)
        mean = ubm.means_invvars / ubm.inv_vars
        comp = rng.integers(0, a.I, (a.B, a.T))
        x = torch.as_tensor((mean[comp] + rng.standard_normal((a.B, a.T, a.D)) / np.sqrt(ubm.inv_vars[comp])).astype(np.float32),
                            device=dev)
        W, gc, sim, U, fullc = layer._consts(dev)
        flat = x.reshape(-1, a.D)
        layer(x[:2])                                                            # warm-up (LDS attributes, allocator)
        t_post, (g, p) = timed(lambda: ops.ivector_post(flat, W, gc, layer.numGselect, layer.minPost), a.reps)
        extra = {}
        if full is not None:                                                    # the recipe's stage, on the same frames
            mic, icov, fgc = fullc
            t_sel, (sel, _) = timed(lambda: ops.ivector_post(flat, W, gc, layer.numGselect, 0.0), a.reps)
            t_full, (g, p) = timed(lambda: ops.fgmm_post(flat, sel, mic, icov, fgc, layer.minPost), a.reps)
            extra = {"preselect_ms": round(t_sel * 1e3, 3), "fgmm_post_ms": round(t_full * 1e3, 3),
                     "fgmm_over_diag_post": round(t_full / t_post, 3), "frame_chunks": -(-flat.shape[0] // layer._frameStep),
                     "kept_per_frame": round(float((g >= 0).sum().item()) / flat.shape[0], 2)}
            del mic, icov, fgc, sel
        off = np.arange(a.B + 1) * a.T
        t_ext, iv = timed(lambda: layer._extract(flat, off, lambda lo, hi: (g[lo:hi], p[lo:hi]), torch.float32), a.reps)
        t_all, _ = timed(lambda: layer(x), a.reps)
        t_b1, _ = timed(lambda: layer(x[:1]), a.reps)
        # host restatement on a few utterances
        h = a.host_utts
        xs = x[:h].cpu().numpy()
        t0 = time.perf_counter()
        gmm = (ubm.gconsts, ubm.means_invvars, ubm.inv_vars)
        for b in range(h):
            gg, pp = R.posteriors(xs[b], gmm, 20, 0.025)
            gamma, F = R.stats(xs[b], gg, pp, a.I)
            R.extract_packed(gamma, F, ie.sigmaInvM, ie.U, ie.priorOffset)
        t_host = (time.perf_counter() - t0) / h
        if a.train:
            extra.update(train_times(a, layer, ie, x, flat, off, g, p, t_all))
        print(json.dumps({
            "build_id": L.load().ktf_build_id().decode(), "device": torch.cuda.get_device_name(dev),
            "B": a.B, "T": a.T, "I": a.I, "D": a.D, "S": S, "chunks": len(layer._chunks(a.B)),
            "posteriors_ms": round(t_post * 1e3, 3), "extract_ms": round(t_ext * 1e3, 3), "call_ms": round(t_all * 1e3, 3),
            "ivectors_per_s": round(a.B / t_all, 1), "batch1_ms": round(t_b1 * 1e3, 3),
            "host_numpy_s_per_utt": round(t_host, 3), "finite": bool(torch.isfinite(iv).all().item()), **extra}), flush=True)
        del layer, x, flat, g, p, iv, W, gc, sim, U, fullc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
