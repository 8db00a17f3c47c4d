"""Every LDS placement of the fused VAD / CMVN kernel and of the stand-alone CMVN kernel (csrc/vad_cmvn.hip), on the GPU.

`ktf_vad_cmvn` decides per call, from (B, T, D, ldo), where four things live -- the frame map (LDS or idx_work), the staged rows (LDS or
the global `work` buffer), the 32-row block sums (present or absent) and the energy column (LDS or read from the feature rows) -- and
from them the kernel instantiation and the number of workgroups per utterance: nine outcomes. `ktf_cmvn_f32` has four. The tests here
take their T from the launchers' own plan queries (tests/_vc_plans.py), run both sides of every change of plan, and assert that what
they ran covers every plan -- so a retuned limit moves the tested sizes with it, and a plan that is no longer reached fails a test.

Reference: oracle VAD (vad.py:156-203) -> gather -> oracle CMVN (cmvn.py:186-250) evaluated in float64.
Bounds: the project's own -- fused 2e-4 * max(1, |want|max) for fp32 output and 1.5e-1 for bf16 (test_gpu_round4.py), stand-alone
3e-5 absolute on N(-1, 4) input (test_gpu_parity.py). The placements without block sums add the 300 terms of a chunk's first window
serially (expected: about sqrt(300) * 2^-24 * |x| = 1e-5); every test prints the largest error of each plan before it asserts (pytest -s).
INTEGRATION.md ("Placements of the VAD / CMVN kernels") has the table of plans.
"""

import itertools

import numpy as np
import pytest
import torch

import _vc_plans as P
from kaldi_tflite_amd import ops
from kaldi_tflite_amd import layers as Ls
from oracle import ktf_oracle as O

pytestmark = pytest.mark.gpu

SENT, ISENT = 9.0, -7          # what the buffers hold before the call (exact in bf16)
GUARD = 1024                   # elements of guard band behind every buffer
TOL = {torch.float32: 2e-4, torch.bfloat16: 1.5e-1}
TOL_ALONE = 3e-5
VOTE = dict(energy_mean_scale=0.5, energy_threshold=5.5, frames_context=2, proportion_threshold=0.12)
PLAIN = dict(energy_mean_scale=0.0, energy_threshold=5.5, frames_context=0, proportion_threshold=0.12)    # kept == above the threshold
N = 300                        # the CMVN window of the planted utterances


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def batch_of(T):
    """Five utterances (eight workgroups each in the LDS forms) up to 2000 frames, three beyond."""
    return 3 if T > 2000 else 5


def guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[:n].view(shape)


def run_fused(feats, vcfg, ccfg, ldo, out_dtype):
    """ktf_vad_cmvn on buffers of exactly the extractor's sizes (models.py, XvectorExtractor._features), each followed by a guard band."""
    B, T, D = feats.shape
    fills = (SENT, ISENT, ISENT, SENT)
    bufs = [guarded((B, T, ldo), out_dtype, SENT), guarded((B,), torch.int32, ISENT), guarded((B, T), torch.int32, ISENT),
            guarded((B * T * 2 * D + 2 * D,), torch.float32, SENT)]
    out, lens, idx, work = (v for _, v in bufs)
    ops.vad_cmvn(dev(feats), Ls.VAD(**vcfg).cfg(), ccfg, out, lens, idx, work)
    torch.cuda.synchronize()
    for (buf, view), fill, name in zip(bufs, fills, ("out", "lens", "idx_work", "work")):
        assert bool((buf[view.numel():] == fill).all()), f"the guard band behind `{name}` was written"
    return out.float().cpu().numpy(), lens.cpu().numpy(), idx.cpu().numpy()


def kept_frames(feats, vcfg):
    keep = O.vad(feats, **vcfg, return_indexes=False)[..., 0] > 0
    return [np.nonzero(k)[0] for k in keep]


def oracle_rows(x, sel, window, nv, pad):
    if not len(sel):
        return np.zeros((0, x.shape[-1]))
    with np.errstate(invalid="ignore", divide="ignore"):       # (one frame and norm_vars: 0 / 0 in the reference too)
        return O.cmvn(x[None, sel], norm_vars=nv, window=window, padding=pad, dtype=np.float64)[0]


def check_fused(got, lens, idx, sels, wants, D, what):
    """Structure (asserted here) and the largest deviation of the batch as a multiple of max(1, |want|max) (returned)."""
    worst = 0.0
    for b, (sel, want) in enumerate(zip(sels, wants)):
        n = want.shape[0]
        assert lens[b] == n, (what, b, int(lens[b]), n)
        assert np.array_equal(idx[b, :len(sel)], sel), (what, b, "kept frame numbers")
        if n:
            g, nan = got[b, :n, :D], np.isnan(want)
            assert np.array_equal(np.isnan(g), nan), (what, b, "NaN where the reference has NaN, and only there")
            if not nan.all():
                worst = max(worst, float(np.abs(g[~nan] - want[~nan]).max() / max(1.0, np.abs(want[~nan]).max())))
            assert not got[b, :n, D:].any(), (what, b, "pad columns are written as zeros")
        assert (got[b, n:] == SENT).all(), (what, b, "rows beyond the utterance's output length are not written")
    return worst


def report(title, worst, tol):
    """Prints the largest error of every plan, then asserts the bound."""
    print(f"\n{title}")
    for (k, name), e in sorted(worst.items()):
        print(f"  plan {k} {name:<9s} max error {e:.3e}  (bound {tol[name] if isinstance(tol, dict) else tol:.1e})")
    for (k, name), e in worst.items():
        assert e < (tol[name] if isinstance(tol, dict) else tol), (title, k, name, e)


def name_of(dt):
    return {torch.float32: "f32", torch.bfloat16: "bf16"}[dt]


TOL_BY_NAME = {name_of(dt): t for dt, t in TOL.items()}


def noisy_batch(rng, B, T, D):
    """N(6, 4) features; utterance 1 loses two thirds of its frames, utterance 2 all of them. The float32 threshold of the kernel and of
    the oracle sum the energies in different orders: frames within 5e-3 of it are moved away so that both make the same decisions."""
    feats = (rng.standard_normal((B, T, D)) * 4 + 6).astype(np.float32)
    feats[1, T // 3:, 0] = -50.0
    feats[2, :, 0] = -50.0
    for b in range(B):
        e = feats[b, :, 0].astype(np.float64)
        thr = VOTE["energy_threshold"] + VOTE["energy_mean_scale"] * e.mean()
        feats[b, np.abs(e - thr) < 5e-3, 0] = np.float32(thr + 1e-2)
        e = feats[b, :, 0].astype(np.float64)
        thr = VOTE["energy_threshold"] + VOTE["energy_mean_scale"] * e.mean()
        assert np.abs(e - thr).min() > 2e-3
    return feats


def plan_sizes(runs, at_least):
    """One T per plan: its first, or where that is too short for the planted utterances its last."""
    ts = [r[0] if r[0] >= at_least else r[1] for r in runs]
    assert all(t >= at_least for t in ts), ts
    return ts


def ran_every_plan(ran, runs, count):
    assert ran == {r[2] for r in runs} and len(ran) == count, f"ran {len(ran)} of the {len(runs)} plans"


# ----------------------------------------------------------------------------- (a) every placement against the oracle
@pytest.mark.parametrize("D,ldo,both_sides", [(30, 32, True), (40, 64, False), (80, 96, False), (23, 32, False), (32, 32, False)])
def test_every_fused_placement_matches_the_oracle(D, ldo, both_sides):
    """The shipped width on both sides of every change of plan; several 32-column groups with wide pad bands (40 -> 64, 80 -> 96), an odd
    width and one without a pad column at the first T of every plan (and the last of the first). Vote VAD with the mean term, three CMVN configurations, fp32 and
    bf16 output."""
    runs = P.fused_runs(D, ldo)
    sizes = P.both_sides(runs) if both_sides else [runs[0][1]] + P.first_of_each(runs)     # (the first plan also where it is fullest: its first T is 1)
    rng = np.random.default_rng(1000 + D)
    ran, worst = set(), {}
    for T in sizes:
        B = batch_of(T)
        plan = ops.vad_cmvn_plan(B, T, D, ldo)
        ran.add(P.placement(plan))
        assert plan.nsplit == (8 if plan.lds_form else 1)
        feats = noisy_batch(rng, B, T, D)
        sels = kept_frames(feats, VOTE)
        for window, nv, pad in [(300, False, "SAME"), (300, True, "VALID"), (64, True, "SAME")]:
            wants = [oracle_rows(feats[b], sels[b], window, nv, pad) for b in range(B)]
            ccfg = Ls.CMVN(window=window, norm_vars=nv, padding=pad).cfg()
            for dt in TOL:
                got, lens, idx = run_fused(feats, VOTE, ccfg, ldo, dt)
                e = check_fused(got, lens, idx, sels, wants, D, (D, ldo, T, window, nv, pad, name_of(dt)))
                k = (P.plan_number(runs, T), name_of(dt))
                worst[k] = max(worst.get(k, 0.0), e)
    ran_every_plan(ran, runs, 9)
    report(f"fused VAD/CMVN D={D} ldo={ldo}: error / max(1, |want|max) per plan", worst, TOL_BY_NAME)


# ----------------------------------------------------------------------------- (b) plain threshold VAD, planted utterance lengths
def planted_batch(rng, T, D, counts, coeff):
    """Utterances with exactly counts[b] kept frames at random places (frame T-1 among them for the first): energies of 10..30 on the
    kept frames, -50 on the others, N(6, 4) in every other column of every frame."""
    feats = (rng.standard_normal((len(counts), T, D)) * 4 + 6).astype(np.float32)
    feats[:, :, coeff] = -50.0
    sels = []
    for b, n in enumerate(counts):
        pos = np.sort(rng.choice(T - 1, n - (b == 0), replace=False))
        if b == 0:
            pos = np.append(pos, T - 1)
        feats[b, pos, coeff] = rng.uniform(10.0, 30.0, n).astype(np.float32)
        sels.append(pos)
    return feats, sels


def test_plain_threshold_vad_and_utterances_around_the_window_in_every_placement():
    """frames_context = 0 and energy_mean_scale = 0: the kept set is the set of frames above the threshold, exactly (with an LDS energy
    column the threshold phase only copies the column). Planted in every placement: N - 1, N and N + 1 kept frames (whole-utterance
    statistics, and VALID's 0 / 1 / 2 output rows), N + 33 (two chunks of window starts for eight workgroups, where the plan splits), one
    frame (norm_vars: NaN in the kernel and in the reference alike), and -- beyond 2000 frames -- two thirds of the buffer. One run per
    plan takes the energy from column 3."""
    D, ldo = 30, 32
    runs = P.fused_runs(D, ldo)
    rng = np.random.default_rng(2024)
    ran, worst = set(), {}
    for T in plan_sizes(runs, N + 33):
        B = batch_of(T)
        plan = ops.vad_cmvn_plan(B, T, D, ldo)
        ran.add(P.placement(plan))
        assert plan.nsplit == (8 if plan.lds_form else 1)
        batches = [[N - 1, N, N + 1, N + 33, 1]] if B == 5 else [[N - 1, N, N + 1], [N + 33, 1, 2 * T // 3]]
        for counts, (coeff, cfgs) in itertools.product(batches, [(0, [(True, "VALID"), (True, "SAME")]), (3, [(False, "SAME")])]):
            feats, planted = planted_batch(rng, T, D, counts, coeff)
            vcfg = dict(PLAIN, energy_coeff=coeff)
            sels = kept_frames(feats, vcfg)
            assert all(np.array_equal(s, p) for s, p in zip(sels, planted))
            for nv, pad in cfgs:
                wants = [oracle_rows(feats[b], sels[b], N, nv, pad) for b in range(len(counts))]
                if pad == "VALID" and counts[:3] == [N - 1, N, N + 1]:
                    assert [w.shape[0] for w in wants[:3]] == [0, 1, 2]
                ccfg = Ls.CMVN(window=N, norm_vars=nv, padding=pad).cfg()
                for dt in TOL:
                    got, lens, idx = run_fused(feats, vcfg, ccfg, ldo, dt)
                    e = check_fused(got, lens, idx, sels, wants, D, (T, counts, coeff, nv, pad, name_of(dt)))
                    k = (P.plan_number(runs, T), name_of(dt))
                    worst[k] = max(worst.get(k, 0.0), e)
    ran_every_plan(ran, runs, 9)
    report("fused VAD/CMVN, plain threshold VAD, planted lengths: error / max(1, |want|max) per plan", worst, TOL_BY_NAME)


# ----------------------------------------------------------------------------- (c) the same utterance in every placement
def test_one_utterance_gives_the_same_bits_in_every_placement_of_a_summation_order():
    """One fixed set of 1100 kept rows embedded (at random frames) in buffers whose T falls in each of the nine plans, every other frame
    at energy -50: cmvn_block sees the same rows and the same length, and the only input of its arithmetic that varies is whether the
    block sums are given. So the output is bit-identical among the placements with block sums and among those without, whatever the
    instantiation, the home of the rows and the number of workgroups; between the two groups the oracle bound applies."""
    D, ldo, n = 30, 32, 1100
    runs = P.fused_runs(D, ldo)
    rng = np.random.default_rng(31)
    rows = (rng.standard_normal((n, D)) * 4 + 6).astype(np.float32)
    rows[:, 0] = rng.uniform(10.0, 30.0, n).astype(np.float32)
    cfgs = [(True, "SAME"), (False, "VALID")]
    wants = {c: oracle_rows(rows, np.arange(n), N, *c) for c in cfgs}
    ran, worst, outs, sums = set(), {}, {}, {}
    for T in plan_sizes(runs, n):
        B = batch_of(T)
        plan = ops.vad_cmvn_plan(B, T, D, ldo)
        ran.add(P.placement(plan))
        k = P.plan_number(runs, T)
        sums[k] = plan.bs_floats > 0
        feats = (rng.standard_normal((B, T, D)) * 4 + 6).astype(np.float32)
        feats[:, :, 0] = -50.0
        sels = [np.sort(rng.choice(T, n, replace=False)) for _ in range(B)]
        for b in range(B):
            feats[b, sels[b]] = rows
        for c, dt in itertools.product(cfgs, TOL):
            nv, pad = c
            got, lens, idx = run_fused(feats, PLAIN, Ls.CMVN(window=N, norm_vars=nv, padding=pad).cfg(), ldo, dt)
            e = check_fused(got, lens, idx, sels, [wants[c]] * B, D, (T, nv, pad, name_of(dt)))
            worst[(k, name_of(dt))] = max(worst.get((k, name_of(dt)), 0.0), e)
            m = wants[c].shape[0]
            for b in range(1, B):
                assert np.array_equal(got[b, :m], got[0, :m]), (T, c, b, "the same rows at other frames of the buffer")
            outs[(c, name_of(dt), k)] = got[0, :m].copy()
    ran_every_plan(ran, runs, 9)
    report("fused VAD/CMVN, one utterance in every placement: error / max(1, |want|max) per plan", worst, TOL_BY_NAME)
    differ = []
    for c, dt in itertools.product(cfgs, TOL):
        for with_sums in (True, False):
            group = [k for k in sorted(sums) if sums[k] == with_sums]
            assert len(group) >= 4
            differ += [(c, name_of(dt), group[0], k, int((outs[(c, name_of(dt), k)] != outs[(c, name_of(dt), group[0])]).sum()))
                       for k in group[1:] if not np.array_equal(outs[(c, name_of(dt), k)], outs[(c, name_of(dt), group[0])])]
    assert not differ, f"(config, dtype, plan, plan, differing values): {differ}"


# ----------------------------------------------------------------------------- (d) the stand-alone layer
@pytest.mark.parametrize("D", [30, 40, 80])
def test_standalone_cmvn_in_every_placement(D):
    """ktf_cmvn_f32 (rows in LDS or in the workspace, with or without block sums) on both sides of every change of plan: the layer on
    whole buffers, and ops.cmvn with ragged lengths (the placement follows T, the block-sum layout the utterance's own length)."""
    runs = P.cmvn_runs(D, D)
    rng = np.random.default_rng(50 + D)
    ran, worst = set(), {}
    for T in P.both_sides(runs):
        B = batch_of(T)
        ran.add(P.placement(ops.cmvn_plan(T, D)))
        k = P.plan_number(runs, T)
        x = (rng.standard_normal((B, T, D)) * 4 - 1).astype(np.float32)
        xlens = np.array([T, 2 * T // 3, N + 1, N, 1][:B], dtype=np.int32)
        for nv, pad in itertools.product((False, True), ("SAME", "VALID")):
            layer = Ls.CMVN(window=N, norm_vars=nv, padding=pad)
            got = layer(dev(x)).cpu().numpy()
            want = O.cmvn(x, norm_vars=nv, window=N, padding=pad, dtype=np.float64)
            assert got.shape == want.shape, (D, T, nv, pad, got.shape, want.shape)
            e = float(np.abs(got - want).max())
            out, out_lens = ops.cmvn(dev(x), layer.cfg(), lens=dev(xlens), want_lens=True)
            out, out_lens = out.cpu().numpy(), out_lens.cpu().numpy()
            for b in range(B):
                w = oracle_rows(x[b], np.arange(xlens[b]), N, nv, pad)
                m = w.shape[0]
                assert out_lens[b] == m, (D, T, nv, pad, b, int(out_lens[b]), m)
                if m:
                    nan = np.isnan(w)
                    assert np.array_equal(np.isnan(out[b, :m]), nan), (D, T, nv, pad, b)
                    if not nan.all():
                        e = max(e, float(np.abs(out[b, :m][~nan] - w[~nan]).max()))
            worst[(k, "f32")] = max(worst.get((k, "f32"), 0.0), e)
    ran_every_plan(ran, runs, 4)
    report(f"stand-alone CMVN D={D}: absolute error per plan", worst, TOL_ALONE)
