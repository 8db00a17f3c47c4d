"""tests/_pool_ref.py on the CPU: the reference that test_gpu_pool_post.py holds the pooling, finalize, post and tail kernels
against agrees with the project's oracle, its case tables reach every kernel instance and path, its bounds admit a correct
evaluation in another order of every case and reject every single mutation of it -- so no case of the GPU test is vacuous --, and
the layout guards of the ops.py wrappers fire before the library is called.

Admitted: pooling and finalize as the kernels compute them (fp64 sums in the kernel's grouping, rounded once); post and tail as
sequential NumPy float32 (products rounded, one running sum per output, the norm a running sum too): another order than the
kernels' lanes and butterflies. Mutations (each alone): an input column of W (post: of A) zeroed; a row of W (post: a column of A)
rotated by one input; one row beyond len pooled; one sampled row dropped; the pooling's sums carried in fp32; one slot more or
fewer than an utterance uses in the finalize."""

import contextlib
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "kaldi-tflite_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from kaldi_tflite_amd import _lib as L, ops  # noqa: E402
from oracle import ktf_oracle as O  # noqa: E402
import _pool_ref as P  # noqa: E402
import _tdnn_grad_ref as G  # noqa: E402
from _recorder import STREAM, Recorder  # noqa: E402

F32, F64 = np.float32, np.float64


def _close(a, b, rel=1e-12):
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    assert (np.abs(a[ok] - b[ok]) <= rel * np.maximum(1.0, np.abs(b[ok]))).all(), float(np.abs(a[ok] - b[ok]).max())


# ----------------------------------------------------------------------------- the reference against the oracle
@pytest.mark.parametrize("period,include_std", [(1, True), (3, True), (1, False)])
def test_pool_agrees_with_the_oracle(period, include_std):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, 50, 7)).astype(F32)
    want, _ = P.pool(x, None, period, include_std, 1e-10)
    _close(want, O.stats_pooling(x, input_period=period, include_std=include_std, reduce_time_axis=True, epsilon=float(F32(1e-10)),
                                 dtype=F64)[:, 0])
    lens = [50, 1, 33]
    want, _ = P.pool(x, lens, period, include_std, 1e-10)
    _close(want, G.pool_forward(x, lens, include_std, float(F32(1e-10)), period))
    # the exact=False form (sums about the first row) is the same to fp64
    _close(P.pool(x, lens, period, include_std, exact=False)[0], want)
    assert np.isnan(P.pool(x, [0, -1, 2], period, include_std)[0][:2]).all()


def test_pool_moments_are_exact_where_they_cancel():
    """A column of 3 + 1e-4 N(0, 1): E[x^2] - mean^2 in fp64 keeps seven digits of the variance; the reference agrees with rational
    arithmetic to 1e-13."""
    from fractions import Fraction
    rng = np.random.default_rng(2)
    x = P.columns(rng, (1, 70, 5))
    want, _ = P.pool(x, None, 1, True, 0.0)
    for c in range(5):
        v = [Fraction(float(a)) for a in x[0, :, c]]
        mean = sum(v) / 70
        var = sum(a * a for a in v) / 70 - mean * mean
        assert abs(want[0, c] - float(mean)) <= 1e-15 * abs(float(mean))
        assert abs(want[0, 5 + c] ** 2 - float(var)) <= 1e-13 * float(var) or float(var) == 0 == want[0, 5 + c]


@pytest.mark.parametrize("name", sorted(n for n, c in P.WINDOWED_CASES.items() if c["exact"]))
def test_windowed_agrees_with_the_oracle(name):
    c = P.WINDOWED_CASES[name]
    x = np.random.default_rng(c["seed"]).standard_normal((c["B"], c["T"], c["D"])).astype(F32)
    start, T_out = P.window_steps(c["T"], c["left"], c["right"], c["output_period"], c["padding"])
    want, _ = P.pool_windowed(x, c["left"], c["right"], c["input_period"], c["output_period"], start, T_out, c["include_std"], 1e-10)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = O.stats_pooling(x, c["left"], c["right"], c["input_period"], c["output_period"], c["include_std"], c["padding"],
                              float(F32(1e-10)), dtype=F64)
    if c["padding"] == "SAME":
        ref = ref[:, ::c["output_period"]]                       # (the oracle repeats every row output_period times)
    _close(want, ref)


def test_finalize_agrees_with_the_pooling():
    for c in P.FINALIZE_CASES.values():
        d = P.finalize_data(c)
        x = np.random.default_rng(c["seed"] + 50).standard_normal(d["x"].shape).astype(F32)        # well conditioned
        if c["form"] == "flat":
            sums, used, _ = P.flat_sums(x, d["lens"], d["slots"])
        else:
            sums, used = P.slot_sums(x, d["lens"], d["slots"], c["slot_rows"] or 128)
        assert used == d["used"]
        _close(P.finalize(sums, d["lens"], used, c["include_std"])[0], P.pool(x, d["lens"], 1, c["include_std"])[0], rel=1e-11)


def test_post_and_tail_agree_with_the_oracle():
    rng = np.random.default_rng(3)
    B, in_dim, units, out_dim = 4, 30, 20, 9
    x, W, b = rng.standard_normal((B, in_dim)), rng.standard_normal((units, in_dim)), rng.standard_normal(units)
    mean, A, off = rng.standard_normal(units), rng.standard_normal((units, out_dim)), rng.standard_normal(out_dim)
    lda = np.concatenate([A.T, off[:, None]], 1)                 # transform.mat: (out, in + 1), the last column the offset
    h = rng.standard_normal((B, units))
    _close(P.post(h, mean, A, off)["y"], O.xvector_post(h, mean, lda, dtype=F64))
    _close(P.post(h, None, A, None)["y"], O.xvector_post(h, np.zeros(units), np.concatenate([A.T, np.zeros((out_dim, 1))], 1), dtype=F64))
    # xvector_forward's tail: the layers behind the pooling (tdnn6), then xvector_post
    h6 = O.sequential_forward([dict(kind="tdnn", W=W, b=b, context=[0])], x[:, None, :], dtype=F64)
    r = P.tail(x, W, b, mean, A, off)
    _close(r["h"], h6[:, 0])
    _close(r["y"], O.xvector_post(h6, mean, lda, dtype=F64))


# ----------------------------------------------------------------------------- the tables reach every instance and path
def test_the_pool_cases_cover_every_instance():
    cs = list(P.POOL_CASES.values())
    assert {(c["dtype"], c["vec"], c["narrow"]) for c in cs} == {(d, v, n) for d in ("f32", "bf16") for v in (True, False) for n in (True, False)}
    for c in cs:
        assert (c["narrow"], c["vec"]) == P.pool_instance(c["B"], c["D"], c["ldx"], c["offset"], 4 if c["dtype"] == "f32" else 2)
        assert c["ldx"] >= c["D"] and (c["narrow"] or c["B"] * P.cdiv(c["D"], 128) >= 256)
    for dtype in ("f32", "bf16"):
        mine = [c for c in cs if c["dtype"] == dtype]
        assert {c["D"] for c in mine if c["narrow"]} == set(P.POOL_DS)
        assert {c["D"] % 128 for c in mine if not c["narrow"]} >= {33, 2}                 # partly filled 128-column blocks
        assert any(0 < c["D"] % 32 < 32 for c in mine if c["narrow"])                      # ... and 32-column ones
        assert {"D" if c["ldx"] == c["D"] else "D+2" for c in mine if c["vec"] and c["ldx"] - c["D"] in (0, 2)} == {"D", "D+2"}
        assert {(c["ldx"] % 2, c["offset"]) for c in mine if not c["vec"]} == {(1, 0), (0, 1)}
        assert {(c["period"], c["include_std"]) for c in mine} == {(p, s) for p in (1, 3) for s in (True, False)}
        assert any(c["ld_out_extra"] for c in mine) and any(c["lens"] is None for c in mine)
    seen = {n for c in cs if c["lens"] is not None for n in c["lens"]} | {None}
    assert seen == set(P.POOL_LENS)
    # B = 3, T = 70: the row groups j mod 64 hold 0, 1 or 2 rows
    assert all(c["B"] == 3 and c["T"] == 70 for c in cs if c["narrow"])


def test_the_other_cases_cover_every_path():
    ws = list(P.WINDOWED_CASES.values())
    assert {c["padding"] for c in ws} == {"SAME", "VALID"} and {(c["left"], c["right"]) for c in ws if c["exact"]} == set(P.WINDOWS)
    for left, right in P.WINDOWS:
        assert {c["T"] for c in ws if (c["left"], c["right"]) == (left, right)} >= {1, 2, right, right + 1, 61} - {0}
    assert any(c["input_period"] == 3 and c["left"] % 3 for c in ws) and {c["output_period"] for c in ws} == {1, 3}
    assert {c["D"] for c in ws if c["exact"]} == {1, 23}
    above = [c for c in ws if c["B"] * P.window_steps(c["T"], c["left"], c["right"], c["output_period"], c["padding"])[1] * c["D"] > P.GRID_CAP]
    assert len(above) == 1
    c = P.WINDOWED_CASES["win_4_5_T2_SAME"]
    want, _ = P.pool_windowed(P.windowed_data(c), -4, 5, c["input_period"], c["output_period"], 0, 1)
    assert c["input_period"] == 3 and np.isnan(want).all()                                # a window without a frame

    fs = list(P.FINALIZE_CASES.values())
    assert {(c["form"], c["slot_rows"]) for c in fs} == {("sums", 0), ("slots", 64), ("slots", 128), ("flat", 128)}
    assert {c["D"] for c in fs} == {1, 33} and {c["include_std"] for c in fs} == {True, False} and any(c["ld_out_extra"] for c in fs)
    d = P.finalize_data(P.FINALIZE_CASES["fin_flat128_D33"])
    assert 0 in d["used"] and any(int(s) % 128 + n > 128 and int(s) % 128 for s, n in zip(d["starts"], d["lens"]))   # straddles a block

    ps = list(P.POST_CASES.values())
    assert {c["out_dim"] for c in ps} >= {1, 64, 65, 150, 1000, 1025} and {c["in_dim"] for c in ps} >= {1, 3, 23, 512}
    assert {c["B"] for c in ps} >= {1, 257, 259} and {c["B"] % 4 for c in ps if c["eb"] == 4} >= {1, 2, 3}
    assert {c["eb"] for c in ps} == {1, 4} and any(c["eb"] == 1 and c["B"] > 256 for c in ps)
    assert all(c["eb"] == P.post_eb(c["B"], c["in_dim"], c["out_dim"]) and P.post_fits(c["in_dim"], c["out_dim"]) for c in ps)
    assert any(not c["mean"] for c in ps) and any(not c["off"] for c in ps) and {c["regime"] for c in ps} == {"gauss", "int"}
    assert any(c["out_dim"] > 1024 for c in ps)                                            # a second j0 round
    assert any(c["in_dim"] < 1024 // min(1024, -(-c["out_dim"] // 64) * 64) for c in ps)   # in_dim < P: empty parts

    ts = list(P.TAIL_CASES.values())
    assert {c["in_dim"] for c in ts} == {2, 6, 70, 301, 3072} and {c["units"] for c in ts} == {1, 7, 63, 64, 65, 130, 512}
    assert {c["out_dim"] for c in ts} == {1, 33, 150, 256} and {c["source"] for c in ts} == set(P.TAIL_SOURCES)
    assert {c["group"] for c in ts} == {1, 2, 32, 1024} and {c["two_phase"] for c in ts} == {True, False}
    assert all(c["two_phase"] == (c["group"] > 1) for c in ts) and all(c["B"] % c["group"] for c in ts if c["group"] > 1)
    assert {c["B"] for c in ts if c["group"] == 1} >= {1, 5} and {c["include_std"] for c in ts} == {True, False}
    for what in ("bias", "mean", "off", "h_out"):
        assert any(not c[what] for c in ts)
    assert all(c["regime"] == "int" for c in ts if c["in_dim"] == 3072 or c["units"] == 512)
    assert {c["ldw_extra"] for c in ts} >= {0, 4, 8}
    skip = [c for c in ts if c["skip_empty"]]
    assert {c["two_phase"] for c in skip} == {True, False} and {c["source"][:4] for c in skip} == {"pool", "sums", "slot"}
    g = P.TAIL_CASES["t70_u65_o33_slots64_skip_g2"]
    groups = [g["lens"][i:i + 2] for i in range(0, g["B"], 2)]
    assert any(max(q) == 0 for q in groups) and any(min(q) == 0 < max(q) for q in groups) and groups[-1] == (0,)
    assert any(not c["skip_empty"] and c["lens"] and 0 in c["lens"] and c["source"] not in ("pooled", "pooled_ld5") for c in ts)


# ----------------------------------------------------------------------------- evaluations the bounds must admit, and mutations
def kernel_pool(x, lens, period, include_std, eps, acc=F64, extra_row=False, drop_row=False):
    """ktf_stats_pool as written: rows in 64 interleaved groups, ((g + g+16) + g+32) + g+48 over g = 0..15; `acc` the type of the
    sums (the kernel: fp64). extra_row: the next sampled row beyond len is pooled too; drop_row: the middle sampled row is not."""
    B, T, D = x.shape
    out = np.full((B, 2 * D if include_std else D), np.nan, dtype=F32)
    for b in range(B):
        idx = list(range(0, P.clamp_len(None if lens is None else lens[b], T), period))
        if extra_row and len(idx) * period < T:
            idx.append(len(idx) * period)
        if drop_row and idx:
            del idx[len(idx) // 2]
        n = len(idx)
        if n == 0:
            continue
        s, q = np.zeros((64, D), dtype=acc), np.zeros((64, D), dtype=acc)
        for j, t in enumerate(idx):
            v = x[b, t].astype(acc)
            s[j % 64] += v
            q[j % 64] += v * v
        S, Q = np.zeros(D, dtype=acc), np.zeros(D, dtype=acc)
        for g in range(16):
            S += ((s[g] + s[g + 16]) + s[g + 32]) + s[g + 48]
            Q += ((q[g] + q[g + 16]) + q[g + 32]) + q[g + 48]
        mean = S / acc(n)
        out[b, :D] = mean
        if include_std:
            out[b, D:] = np.sqrt(np.maximum(Q / acc(n) - mean * mean, acc(0)) + acc(F32(eps)))
    return out


def kernel_windowed(x, c, start, T_out, acc=F64, extra_row=False, drop_row=False):
    B, T, D = x.shape
    out = np.full((B, T_out, 2 * D), np.nan, dtype=F32)
    offs = list(range(c["left"], min(c["right"] + 1, T), c["input_period"]))
    for j in range(T_out):
        ts = [start + j * c["output_period"] + o for o in offs]
        ts = [t for t in ts if 0 <= t < T]
        if extra_row and ts and len(ts) < T:
            ts.append(min(set(range(T)) - set(ts)))             # a frame the window does not sample
        if drop_row and ts:
            del ts[0]
        if not ts:
            continue
        s, q = np.zeros((B, D), dtype=acc), np.zeros((B, D), dtype=acc)
        for t in ts:
            v = x[:, t].astype(acc)
            s += v
            q += v * v
        mean = s / acc(len(ts))
        out[:, j, :D] = mean
        out[:, j, D:] = np.sqrt(np.maximum(q / acc(len(ts)) - mean * mean, acc(0)) + acc(F32(1e-10)))
    return out


def kernel_finalize(sums, lens, used, include_std, eps, delta=0):
    sums = np.asarray(sums)
    sums = sums[:, None] if sums.ndim == 3 else sums
    B, _, _, D = sums.shape
    out = np.full((B, 2 * D if include_std else D), np.nan, dtype=F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            s, q = np.zeros(D), np.zeros(D)
            for k in range(max(used[b] + delta, 0) if lens[b] > 0 else 0):
                s, q = s + sums[b, k, 0], q + sums[b, k, 1]
            mean = s / F64(lens[b])
            out[b, :D] = mean
            if include_std:
                out[b, D:] = np.sqrt(np.maximum(q / F64(lens[b]) - mean * mean, 0.0) + F64(F32(eps)))
    return out


def seq_dot32(X, Wt):
    """X (B, K) @ Wt (K, N) in float32, one running sum per output, k ascending."""
    acc = np.zeros((X.shape[0], Wt.shape[1]), dtype=F32)
    for k in range(X.shape[1]):
        acc += X[:, k:k + 1] * Wt[k]
    return acc


def norm32(t):
    t = t.astype(F32)
    with np.errstate(invalid="ignore"):
        tot = np.cumsum(t * t, axis=1, dtype=F32)[:, -1:]
        return t / (np.sqrt(tot) / np.sqrt(F32(t.shape[1])))


def post32(x, mean, A, off):
    d = x if mean is None else x - mean
    t = seq_dot32(d.astype(F32), A)
    return norm32(t if off is None else t + off)


def tail32(x, W, bias, mean, A, off):
    h = seq_dot32(x.astype(F32), np.ascontiguousarray(W.T))
    h = h if bias is None else h + bias
    t = seq_dot32(h if mean is None else h - mean, A)
    return h, norm32(t if off is None else t + off)


@pytest.mark.parametrize("name", sorted(P.POOL_CASES))
def test_pool_bounds_admit_the_kernel_and_reject_its_mutations(name):
    c = P.POOL_CASES[name]
    x, lens = P.pool_data(c)
    want, bound = P.pool(x, lens, c["period"], c["include_std"])
    args = (x, lens, c["period"], c["include_std"], 1e-10)
    clean = P.ratio(kernel_pool(*args), want, bound)
    assert clean <= 1.0, clean
    ns = [len(range(0, P.clamp_len(None if lens is None else lens[b], c["T"]), c["period"])) for b in range(c["B"])]
    assert max(ns) >= 21
    muts = dict(fp32=kernel_pool(*args, acc=F32), dropped=kernel_pool(*args, drop_row=True))
    if any(n * c["period"] < c["T"] for n in ns):
        muts["beyond_len"] = kernel_pool(*args, extra_row=True)
    for tag, got in muts.items():
        r = P.ratio(got, want, bound)
        assert r > 100, (tag, r)


@pytest.mark.parametrize("name", sorted(P.WINDOWED_CASES))
def test_windowed_bounds_admit_the_kernel_and_reject_its_mutations(name):
    c = P.WINDOWED_CASES[name]
    x = P.windowed_data(c)
    start, T_out = P.window_steps(c["T"], c["left"], c["right"], c["output_period"], c["padding"])
    want, bound = P.pool_windowed(x, c["left"], c["right"], c["input_period"], c["output_period"], start, T_out, True, 1e-10, exact=c["exact"])
    clean = kernel_windowed(x, c, start, T_out)
    assert P.ratio(clean, want, bound) <= 1.0
    # (a window without a frame has none to drop, one that holds all T frames none to add: the mutation is the clean evaluation)
    muts = dict(dropped=kernel_windowed(x, c, start, T_out, drop_row=True))
    rows = max(sum(0 <= start + j * c["output_period"] + o < c["T"] for o in range(c["left"], min(c["right"] + 1, c["T"]), c["input_period"]))
               for j in range(T_out))
    if c["exact"] and rows >= 2:
        # (the cancelling columns: the case above the cap is N(0, 1); a window of one row has nothing to accumulate, fp32 or not)
        muts["fp32"] = kernel_windowed(x, c, start, T_out, acc=F32)
    muts["beyond"] = kernel_windowed(x, c, start, T_out, extra_row=True)
    for tag, got in muts.items():
        if tag != "fp32" and np.array_equal(got, clean, equal_nan=True):
            assert rows == 0 or (tag == "beyond" and rows == c["T"]), (tag, rows)
            continue
        r = P.ratio(got, want, bound)
        assert r > 100, (tag, r)


@pytest.mark.parametrize("name", sorted(P.FINALIZE_CASES))
def test_finalize_bounds_admit_the_kernel_and_reject_its_mutations(name):
    c = P.FINALIZE_CASES[name]
    d = P.finalize_data(c)
    want, bound = P.finalize(d["sums"], d["lens"], d["used"], c["include_std"])
    assert P.ratio(kernel_finalize(d["sums"], d["lens"], d["used"], c["include_std"], 1e-10), want, bound) <= 1.0
    # ... and it is the pooling of the rows behind the sums, within both bounds
    pw, pb = P.pool(d["x"], d["lens"], 1, c["include_std"])
    assert P.ratio(want, pw, pb + bound) <= 1.0
    if c["form"] != "sums":
        for delta in (1, -1):
            r = P.ratio(kernel_finalize(d["sums"], d["lens"], d["used"], c["include_std"], 1e-10, delta), want, bound)
            assert r > 100, (delta, r)


@pytest.mark.parametrize("name", sorted(P.POST_CASES))
def test_post_bounds_admit_fp32_and_reject_its_mutations(name):
    c = P.POST_CASES[name]
    x, mean, A, off = P.post_data(c)
    r = P.post(x, mean, A, off)
    bound = P.EXACT_Y * np.abs(r["y"]) if c["regime"] == "int" else r["e_y"]
    clean = P.ratio(post32(x, mean, A, off), r["y"], bound)
    print(f"{name}: fp32 in another order at {clean:.3f} of the bound")
    assert clean <= 1.0, clean
    i, j = c["in_dim"] // 2, c["out_dim"] // 2
    zeroed = A.copy()
    zeroed[i] = 0
    muts = dict(zeroed=zeroed)
    if c["in_dim"] > 1:
        muts["rotated"] = A.copy()
        muts["rotated"][:, j] = np.roll(A[:, j], 1)
    for tag, Am in muts.items():
        got = P.ratio(post32(x, mean, Am, off), r["y"], bound)
        assert got > 10, (tag, got)


@pytest.mark.parametrize("name", sorted(P.TAIL_CASES))
def test_tail_bounds_admit_fp32_and_reject_its_mutations(name):
    c = P.TAIL_CASES[name]
    d = P.tail_data(c)
    r = P.tail_reference(c, d)
    live = np.ones(c["B"], bool) if not c["skip_empty"] else np.array(d["lens"]) > 0
    integer = c["regime"] == "int"
    b_h = np.zeros_like(r["h"]) if integer else r["e_h"]
    b_y = P.EXACT_Y * np.abs(r["y"]) if integer else r["e_y"]
    pooled = np.asarray(d["pooled"], dtype=F64).astype(F32)

    def ratios(W, pooled=pooled):
        with np.errstate(invalid="ignore"):
            h, y = tail32(pooled, W, d["bias"], d["mean"], d["A"], d["off"])
        rh = P.ratio(h[live], r["h"][live], b_h[live]) if c["h_out"] else 0.0
        return max(rh, P.ratio(y[live], r["y"][live], b_y[live]))

    clean = ratios(d["W"])
    print(f"{name}: fp32 in another order at {clean:.3f} of the bound")
    assert clean <= 1.0, clean
    W = d["W"]
    i = int(np.flatnonzero(np.abs(W).sum(0))[c["in_dim"] // 2 % np.count_nonzero(np.abs(W).sum(0))])
    zeroed, rotated = W.copy(), W.copy()
    zeroed[:, i] = 0
    u = int(np.flatnonzero(W[:, i])[0])
    rotated[u] = np.roll(W[u], 1)
    for tag, Wm in (("zeroed", zeroed), ("rotated", rotated)):
        got = ratios(Wm)
        assert got > 10, (tag, got)
    if d["e_pooled"] is not None and c["source"] != "sums":
        # one slot fewer in the tail's own finalize
        less = kernel_finalize(d["sums"], d["lens"], d["used"], c["include_std"], d["eps"], -1)
        got = ratios(W, pooled=less)
        assert got > 10, ("used - 1", got)


# ----------------------------------------------------------------------------- the wrappers' layout guards
def _t(*shape, dt=torch.float32):
    return torch.zeros(shape, dtype=dt)


def _guard_cases():
    """wrapper -> (keyword arguments every one of which the library can be told about, {argument: a view it cannot})."""
    B, T, D, ld = 3, 9, 4, 6
    i32 = torch.int32
    long = _t(B, 2 * T, ld)
    pool_ok = [dict(x=_t(B, T, D), out=_t(B, 2 * D)), dict(x=_t(B, T, ld), out=_t(B, 2 * D + 3)[:, :2 * D]), dict(x=_t(B, T, ld)[:, :, :D], out=_t(B, 2 * D)),
               dict(x=long[:1, :T], out=_t(1, 2 * D)), dict(x=_t(B, 0, D), out=_t(B, 2 * D)), dict(x=_t(B, 1, D), out=_t(B, 2 * D)),
               dict(x=_t(B, T, D, dt=torch.bfloat16), out=_t(B, 2 * D), lens=_t(B, dt=i32))]
    pool_bad = dict(x=[long[:, :T], _t(B, D, T).transpose(1, 2), _t(B, T, 2 * D)[:, :, ::2]], out=[_t(2 * D, B).t()], lens=[_t(2 * B, dt=i32)[::2]])
    pool = lambda kw: {**dict(D=D, lens=None, input_period=1, include_std=True, eps=1e-10), **kw}  # noqa: E731
    grad = pool
    win = lambda kw: dict(left=-1, right=1, input_period=1, output_period=1, start=0, T_out=T, include_std=True, eps=1e-10, **kw)  # noqa: E731
    units, od = 5, 3
    tail = lambda kw: {**dict(pooled=_t(B, 2 * D), sums=None, slots=0, lens=None, T=T, D=D, include_std=True, eps=1e-10, W=_t(units, 2 * D), bias=_t(units),  # noqa: E731
                              units=units, mean=_t(units), A=_t(units, od), off=_t(od), partial=_t(B, 64, od), counters=_t(B, dt=i32), out=_t(B, od),
                              h_out=_t(B, units)), **kw}
    return {
        "stats_pool": ([pool(kw) for kw in pool_ok], {k: [pool({**pool_ok[0], k: v}) for v in vs] for k, vs in pool_bad.items()}),
        "grad_stats_pool": ([grad(dict(x=_t(B, T, D), gout=_t(B, 2 * D), dx=_t(B, T, D))), grad(dict(x=long[:1], gout=_t(1, 2 * ld), dx=_t(1, 2 * T, ld)))],
                            {"x": [grad(dict(x=_t(B, T, ld)[:, :, :D], gout=_t(B, 2 * D), dx=_t(B, T, D))), grad(dict(x=long[:, :T, :D], gout=_t(B, 2 * D), dx=_t(B, T, D)))],
                             "gout": [grad(dict(x=_t(B, T, D), gout=_t(B, 2 * D + 1)[:, :2 * D], dx=_t(B, T, D)))],
                             "dx": [grad(dict(x=_t(B, T, D), gout=_t(B, 2 * D), dx=_t(B, T, ld)[:, :, :D]))]}),
        "stats_pool_windowed": ([win(dict(x=_t(B, T, D))), win(dict(x=long[:1, :T, :]))], {"x": [win(dict(x=long[:, :T])), win(dict(x=_t(B, T, ld)[:, :, :D]))]}),
        "xvec_post": ([dict(x=_t(B, units), mean=_t(units), A=_t(units, od), off=_t(od)), dict(x=_t(2 * B, units)[B:], mean=None, A=_t(units, od), off=None, out=_t(B, od))],
                      {"x": [dict(x=_t(B, units + 2)[:, :units], mean=_t(units), A=_t(units, od), off=_t(od))],
                       "A": [dict(x=_t(B, units), mean=_t(units), A=_t(od, units).t(), off=_t(od))],
                       "mean": [dict(x=_t(B, units), mean=_t(2 * units)[::2], A=_t(units, od), off=_t(od))],
                       "out": [dict(x=_t(B, units), mean=_t(units), A=_t(units, od), off=_t(od), out=_t(B, od + 1)[:, :od])]}),
        "xvec_tail": ([tail({}), tail(dict(pooled=_t(B, 2 * D + 5)[:, :2 * D], W=_t(units, 2 * D + 4)[:, :2 * D])),
                       tail(dict(pooled=None, sums=_t(B, 2, D, dt=torch.float64), lens=_t(B, dt=i32), h_out=None, bias=None, mean=None, off=None))],
                      {"pooled": [tail(dict(pooled=_t(B, 4 * D)[:, ::2]))], "W": [tail(dict(W=_t(2 * D, units).t()))], "A": [tail(dict(A=_t(od, units).t()))],
                       "sums": [tail(dict(pooled=None, sums=_t(B, 2, D + 1, dt=torch.float64)[:, :, :D]))], "out": [tail(dict(out=_t(B, od + 1)[:, :od]))],
                       "h_out": [tail(dict(h_out=_t(B, units + 1)[:, :units]))], "partial": [tail(dict(partial=_t(B, 64, od + 1)[:, :, :od]))],
                       "bias": [tail(dict(bias=_t(2 * units)[::2]))]}),
    }


def _recorded(monkeypatch, fn, kw):
    """ops.`fn`(**kw) on CPU tensors with the library replaced by the recorder -> (the symbols it called, the ValueError's text)."""
    rec = Recorder(None, re.compile(r"(?!)"), names=lambda addr: "ptr")
    with monkeypatch.context() as m:
        m.setattr(L, "_lib", rec)
        m.setattr(L, "load", lambda: rec)
        m.setattr(L, "require_gpu", lambda: None)
        m.setattr(L, "stream_ptr", lambda: STREAM)
        m.setattr(L, "on_device", lambda device: contextlib.nullcontext())
        m.setattr(L, "ptr", lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() or 1))
        try:
            getattr(ops, fn)(**kw)
        except ValueError as e:
            return rec.called, str(e)
    return rec.called, None


@pytest.mark.parametrize("fn", ["stats_pool", "grad_stats_pool", "stats_pool_windowed", "xvec_post", "xvec_tail"])
def test_layout_guards_fire_before_the_library_call(monkeypatch, fn):
    good, bad = _guard_cases()[fn]
    symbol = {"stats_pool": "ktf_stats_pool", "grad_stats_pool": "ktf_grad_stats_pool", "stats_pool_windowed": "ktf_stats_pool_windowed_f32",
              "xvec_post": "ktf_xvec_post_f32", "xvec_tail": "ktf_xvec_tail_f32"}[fn]
    for kw in good:
        called, err = _recorded(monkeypatch, fn, kw)
        assert err is None and called == {symbol}, (kw, err)
    assert bad
    if fn == "xvec_tail":
        for kw in (dict(good[0], pooled=None), dict(good[0], sums=_t(3, 2, 4, dt=torch.float64))):
            called, err = _recorded(monkeypatch, fn, kw)
            assert not called and err.startswith("pooled / sums:"), (called, err)
    for arg, kws in bad.items():
        for kw in kws:
            called, err = _recorded(monkeypatch, fn, kw)
            assert not called and err is not None and err.startswith(arg + ":"), (arg, called, err)
