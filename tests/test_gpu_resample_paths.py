"""The branches of csrc/resample.hip that test_gpu_resample.py does not reach, against the fp64 restatement of
tests/_resample_ref.py: the weight table read from global memory (WLDS = false, four of the eight rs_kernel instances), more phases
than a tile has outputs, phases of 2 to 4 and of 255 and 256 taps, a hand-made plan of one tap per phase, and a plan whose first[]
does not ascend (ordered = 0) through ops.rs_resample. tests/test_augment_paths_cpu.py proves that each plan selects its branch.

The bound is test_gpu_resample.py's: |out - ref| <= 2^-24 |ref| + 2^-45 sum|w x| per sample, ref = resample64 with the table the
kernel was given (derived there for up to 2^8 = KTF_RS_MAX_TAPS taps). Rows as there: 0, 1, 2, T - 1, T, T + 1 and 2T + 17 outputs
(T = ktf_rs_tile()) and one of five samples; fp32 and int16 in, fp32 and int16 out. Measured on an MI355X: the worst error / bound
per plan is 0.958 to 0.997, what a correctly rounded fp32 of the fp64 sum gives."""

import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "kaldi-tflite_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import ops  # noqa: E402
import _resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
aug = ktf.augment
T = ops.rs_tile()
LIBRARY_PLANS = R.GLOBAL_TABLE_PLANS + R.WIDE_OU_PLANS + R.FEW_TAPS_PLANS + R.MOST_TAPS_PLANS
UNORDERED = (16000, 17600, 6, None)


def plan_id(p):
    return f"{p[0]}-{p[1]}-z{p[2]}" + (f"-c{p[3]}" if p[3] is not None else "")


@functools.lru_cache(maxsize=None)
def host_plan(key):
    """key: a (fi, fo, zeros, cutoff) of the library, "one_tap", or "unordered" -> (iu, ou, first, taps, w)."""
    if key == "one_tap":
        plan = R.one_tap_plan()
    elif key == "unordered":
        iu, ou, first, taps, w = host_plan(UNORDERED)
        plan = (iu, ou) + R.unordered_plan(first, taps, w, ou // 2)
    else:
        fi, fo, zeros, cutoff = key
        plan = ops.rs_plan(fi, fo, R.default_cutoff(fi, fo) if cutoff is None else cutoff, zeros)
    return plan


@functools.lru_cache(maxsize=None)
def reference(key, i16):
    """(rows, [(fp64 sums, sum |w x|)]) of the plan's batch through resample64 with the plan's table."""
    iu, ou, first, taps, w = host_plan(key)
    rng = np.random.default_rng(1000 * iu + ou)
    xs = [(rng.standard_normal(n) * 3000).astype(np.float32) for n in R.rows_for(iu, ou, T)]
    if i16:
        xs = [np.clip(np.rint(x), -32768, 32767).astype(np.int16) for x in xs]
    refs = [R.resample64(x.astype(np.float32), first, taps, w, iu, ou, 0 if x.size == 0 else -(-x.size * ou // iu)) for x in xs]
    return xs, refs


def run_plan(xs, key, out_dtype=torch.float32, pad=0):
    """The rows through ops.rs_resample with the caller's plan, as Resampler.__call__ hands it the library's. pad: the table's rows
    lie that many floats further apart than its widest phase (ldw > max taps), NaN in between."""
    iu, ou, first, taps, w = host_plan(key)
    n = np.array([x.size for x in xs], np.int32)
    x = torch.zeros((len(xs), int(n.max())), dtype=torch.int16 if xs[0].dtype == np.int16 else torch.float32, device="cuda")
    for b, row in enumerate(xs):
        x[b, :row.size] = torch.as_tensor(row, device="cuda")
    m = [0 if v == 0 else -(-int(v) * ou // iu) for v in n]
    out = torch.empty((len(xs), max(m)), dtype=out_dtype, device="cuda")
    dev = [torch.as_tensor(a, device="cuda") for a in (n, first, taps, w)]
    if pad:
        wide = torch.full((ou, w.shape[1] + pad), float("nan"), device="cuda")
        wide[:, :w.shape[1]] = dev[3]
        dev[3] = wide[:, :w.shape[1]]
    ops.rs_resample(x, n, dev[0], iu, ou, first, taps, dev[1], dev[2], dev[3], out)
    return out, m


def check(tag, key, i16, out, lens):
    """Every sample of every row within the bound; zeros past a row's length. -> the worst err / bound."""
    xs, refs = reference(key, i16)
    out = out.cpu().numpy()
    assert out.dtype == np.float32 and out.shape == (len(xs), max(lens))
    worst = 0.0
    ok = True
    for b, (y, mag) in enumerate(refs):
        assert lens[b] == y.size and not out[b, lens[b]:].any()
        if not lens[b]:
            continue
        err = np.abs(out[b, :lens[b]].astype(np.float64) - y)
        bound = 2.0 ** -24 * np.abs(y) + 2.0 ** -45 * mag
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, ratio)
        print(f"{tag} {'i16' if i16 else 'f32'} n={xs[b].size} m={lens[b]}: worst err / bound {ratio:.3f}"
              + ("" if (err <= bound).all() else f" (first bad output {int(np.argmax(err > bound))})"))
        ok &= bool((err <= bound).all())
    print(f"{tag} {'i16' if i16 else 'f32'}: worst err / bound = {worst:.3f} (limit 1)")
    assert ok
    return worst


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("plan", LIBRARY_PLANS, ids=plan_id)
def test_parity(plan, i16):
    fi, fo, zeros, cutoff = plan
    xs, refs = reference(plan, i16)
    rs = aug.Resampler(fi, fo, lowpass_cutoff=cutoff, num_zeros=zeros)
    iu, ou, first, taps, w = host_plan(plan)
    assert (rs.iu, rs.ou) == (iu, ou) and np.array_equal(rs.first, first) and np.array_equal(rs.taps, taps) and np.array_equal(rs.weights, w)
    assert min(x.size for x in xs if x.size) < int(taps.min())              # a row shorter than the filter
    out, lens = rs(xs, out_dtype=torch.float32)
    assert lens == [R.num_out(x.size, fi, fo) for x in xs] == [rs.num_out(x.size) for x in xs]
    assert [v >= t for v, t in zip(lens, (0, 1, 2, T - 1, T, T + 1, 2 * T + 17))] == [True] * 7
    check(f"parity {plan_id(plan)}", plan, i16, out, lens)
    # int16 out (the other output instance of the same branch): the fp32 output rounded to nearest even and saturated
    o16, l16 = rs(xs, out_dtype=torch.int16)
    assert o16.dtype == torch.int16 and l16 == lens and np.array_equal(o16.cpu().numpy(), R.to_int16(out.cpu().numpy()))
    if i16:                                                                 # the same values as fp32: the same bits
        same, _ = rs([x.astype(np.float32) for x in xs], out_dtype=torch.float32)
        assert torch.equal(same, out)


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("plan", R.GLOBAL_TABLE_PLANS[:2] + R.WIDE_OU_PLANS[:1], ids=plan_id)
def test_table_rows_further_apart_than_the_widest_phase(plan, i16):
    """Resampler's table has ldw = max taps; a caller's may not. Both the kernel's pointer into global memory and its copy into LDS
    step by ldw, and never read the floats between the rows."""
    xs, _ = reference(plan, i16)
    out, lens = run_plan(xs, plan, pad=5)
    check(f"ldw = max taps + 5, {plan_id(plan)}", plan, i16, out, lens)
    tight, lens2 = run_plan(xs, plan)
    assert lens2 == lens and torch.equal(out, tight)


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
def test_one_tap_per_phase(i16):
    xs, refs = reference("one_tap", i16)
    out, lens = run_plan(xs, "one_tap")
    check("one tap per phase 300 -> 301", "one_tap", i16, out, lens)
    # one product per output, rounded once: the fp32 product itself
    iu, ou, first, taps, w = host_plan("one_tap")
    b = int(np.argmax(lens))
    s = np.arange(lens[b])
    k = first[s % ou] + (s // ou) * iu
    want = np.where(k < xs[b].size, w[s % ou, 0] * xs[b].astype(np.float32)[np.minimum(k, xs[b].size - 1)], np.float32(0))
    assert want.dtype == np.float32 and np.array_equal(out[b, :lens[b]].cpu().numpy(), want)
    o16, _ = run_plan(xs, "one_tap", torch.int16)
    assert np.array_equal(o16.cpu().numpy(), R.to_int16(out.cpu().numpy()))


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
def test_unordered_plan(i16):
    xs, refs = reference("unordered", i16)
    iu, ou, first, taps, w = host_plan("unordered")
    assert not R.is_ordered(first, taps, iu) and R.is_ordered(*host_plan(UNORDERED)[2:4], iu)
    out, lens = run_plan(xs, "unordered")
    check("unordered 16000 -> 17600", "unordered", i16, out, lens)
    # against the library's plan on the same rows: the phases left alone have the same bits (the span a tile loads does not
    # show in its sums), and the moved phase, whose added products are exact zeros, too
    lib, lens2 = run_plan(xs, UNORDERED)
    rs_out, lens3 = aug.Resampler(16000, 17600)(list(xs), out_dtype=torch.float32)
    assert lens2 == lens == lens3 and torch.equal(lib, rs_out)
    phase = np.arange(out.shape[1]) % ou
    keep = torch.as_tensor(phase != ou // 2, device="cuda")
    differ = int((out[:, ~keep] != lib[:, ~keep]).sum())
    print(f"unordered {'i16' if i16 else 'f32'}: outputs of the moved phase that differ from the library plan's: {differ}")
    assert torch.equal(out[:, keep], lib[:, keep]) and differ == 0
    o16, _ = run_plan(xs, "unordered", torch.int16)
    assert np.array_equal(o16.cpu().numpy(), R.to_int16(out.cpu().numpy()))


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("plan", [R.GLOBAL_TABLE_PLANS[0], R.WIDE_OU_PLANS[2]], ids=plan_id)
def test_rows_are_isolated(plan, i16):
    fi, fo, zeros, cutoff = plan
    xs, _ = reference(plan, i16)
    rs = aug.Resampler(fi, fo, lowpass_cutoff=cutoff, num_zeros=zeros)
    out, lens = rs(xs)
    again, lens2 = rs(xs)
    assert lens == lens2 and torch.equal(out, again)
    # the same rows in a wider tensor whose padding past n must never be read, in another order
    order = list(reversed(range(len(xs))))
    ldx = max(x.size for x in xs) + 37
    pad = 32767 if i16 else float("nan")
    wide = torch.full((len(xs), ldx), pad, dtype=torch.int16 if i16 else torch.float32, device="cuda")
    for r, b in enumerate(order):
        wide[r, :xs[b].size] = torch.as_tensor(xs[b], device="cuda")
    got, glens = rs(wide[:, :ldx - 3], lengths=[xs[b].size for b in order])
    assert glens == [lens[b] for b in order]
    for r, b in enumerate(order):
        one, l1 = rs(xs[b])
        assert l1 == [lens[b]] and one.shape == (1, lens[b])
        assert torch.equal(one[0], out[b, :lens[b]]) and torch.equal(got[r, :lens[b]], one[0])
        assert not got[r, lens[b]:].any() and not out[b, lens[b]:].any()
