"""Everything behind the TDNN stack on the GPU, one kernel instance at a time, against the exact / fp64 restatement and the bounds of
tests/_pool_ref.py (derived there; test_pool_ref_cpu.py shows that they admit a correct evaluation of every case below and reject
every single mutation of it): ktf_stats_pool (eight instances), ktf_stats_pool_windowed_f32, ktf_stats_finalize{,_slots,_flat},
ktf_xvec_post_f32 (one and four embeddings per workgroup) and ktf_xvec_tail_f32 (ticket and two-launch reduction; pooled rows, fp64
sums, slot sums), through the ops.* wrappers.

Two regimes: Gaussian data (with columns whose E[x^2] - mean^2 cancels) against the bounds, and small integers, where every fp32
product and sum is exact: the tail's h_out equals the reference bit for bit, y is within the rounding of the normalisation alone
(_pool_ref.EXACT_Y) and a pooled mean is float32(S / n). Inputs hold NaN in every row at and beyond len, in every row the input
period skips and in every pad column; outputs start as a sentinel (pad columns, rows that must stay) or NaN (what must be written).
Every test prints the worst |err| / bound of its family; no tolerance here was taken from a GPU run."""

import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "kaldi-tflite_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from kaldi_tflite_amd import ops  # noqa: E402
import _pool_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENT = 777.0
F32, F64 = np.float32, np.float64
EPS = 1e-10
WORST = {}


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _i32(a):
    return None if a is None else torch.as_tensor(list(a), dtype=torch.int32, device=DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    """The same bits; a NaN equals a NaN whatever its payload."""
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


def _note(family, tag, **ratios):
    for k, v in ratios.items():
        WORST[family, k] = max(WORST.get((family, k), 0.0), v)
    print(f"RATIO {family} {tag}: " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))


def _filled(shape, value, dtype=torch.float32, offset=0):
    """A dense device tensor of `shape` holding `value`, `offset` elements into its allocation."""
    n = int(np.prod(shape))
    return torch.full((n + offset,), value, dtype=dtype, device=DEV)[offset:].view(*shape)


# ----------------------------------------------------------------------------- ktf_stats_pool
def run_pool(x, lens, D, ldx, offset, period, include_std, bf16=False, ld_out_extra=0):
    """x (B, T, D) host fp32 -> the (B, ld_out) output, pad columns included. The device buffer has rows of ldx elements and starts
    `offset` elements into its allocation; all but the sampled valid rows' first D columns is NaN."""
    B, T, _ = x.shape
    host = np.full((B, T, ldx), NAN, dtype=F32)
    for b in range(B):
        n = P.clamp_len(None if lens is None else lens[b], T)
        host[b, 0:n:period, :D] = x[b, 0:n:period]
    dt = torch.bfloat16 if bf16 else torch.float32
    xv = _filled((B, T, ldx), NAN, dt, offset)
    xv.copy_(torch.as_tensor(host).to(dt))
    od = (2 if include_std else 1) * D
    out = _filled((B, od + ld_out_extra), SENT)
    ops.stats_pool(xv, D, _i32(lens), period, include_std, EPS, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _pool_ref(name):
    c = P.POOL_CASES[name]
    x, lens = P.pool_data(c)
    want, bound = P.pool(x, lens, c["period"], c["include_std"], EPS)
    for a in (x, want, bound):
        a.setflags(write=False)
    return x, lens, want, bound


@pytest.mark.parametrize("name", sorted(P.POOL_CASES))
def test_stats_pool_instances(name):
    c = P.POOL_CASES[name]
    x, lens, want, bound = _pool_ref(name)
    got = run_pool(x, lens, c["D"], c["ldx"], c["offset"], c["period"], c["include_std"], c["dtype"] == "bf16", c["ld_out_extra"])
    od = want.shape[1]
    assert (got[:, od:] == SENT).all()
    D = c["D"]
    r = dict(mean=P.ratio(got[:, :D], want[:, :D], bound[:, :D]))
    if c["include_std"]:
        r["std"] = P.ratio(got[:, D:od], want[:, D:], bound[:, D:])
    _note("stats_pool", f"{name} narrow={c['narrow']} vec={c['vec']}", **r)
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("name", sorted(n for n, c in P.POOL_CASES.items() if c["D"] in (33, 130) and c["offset"] == 0))
def test_stats_pool_integers(name):
    """Integers of up to three bits: S and Q are exact, a mean is float32(S / n) bit for bit."""
    c = P.POOL_CASES[name]
    x = np.random.default_rng(c["seed"]).integers(-7, 8, (c["B"], c["T"], c["D"])).astype(F32)
    lens = None if c["lens"] is None else list(c["lens"])
    got = run_pool(x, lens, c["D"], c["ldx"], c["offset"], c["period"], c["include_std"], c["dtype"] == "bf16")
    want, bound = P.pool(x, lens, c["period"], c["include_std"], EPS)
    D = c["D"]
    for b in range(c["B"]):
        rows = x[b, 0:P.clamp_len(None if lens is None else lens[b], c["T"]):c["period"]].astype(F64)
        if len(rows):
            assert _same_bits(got[b, :D], (rows.sum(0) / len(rows)).astype(F32)), b
        else:
            assert np.isnan(got[b]).all()
    if c["include_std"]:
        assert P.ratio(got[:, D:], want[:, D:], bound[:, D:]) <= 1.0


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [33, 130])
def test_stats_pool_mappings_give_the_same_bits(D, bf16):
    """An utterance's statistics in the 32- and the 128-column mapping, with pair and with scalar loads, alone and inside a batch:
    the same bits (the kernel's comment: one association of the 64 row groups, whatever the thread mapping)."""
    Bw = 256 // P.cdiv(D, 128)
    rng = np.random.default_rng(70 + D)
    x = P.columns(rng, (Bw, P.POOL_T, D), first=0)
    x = P.to_bf16(x) if bf16 else x
    lens = [(P.POOL_T, 65, 1, 64, 63, 0, 33)[b % 7] for b in range(Bw)]
    even, odd = D + D % 2, D + 1 - D % 2
    item = 2 if bf16 else 4
    want = {}
    for ldx, offset in ((even, 0), (odd, 0), (even + 2, 1)):
        for B in (Bw, 1, 3):
            narrow, vec = P.pool_instance(B, D, ldx, offset, item)
            got = run_pool(x[:B], lens[:B], D, ldx, offset, 3, True, bf16)
            want.setdefault("ref", got)
            assert _same_bits(got, want["ref"][:B]), (ldx, offset, B, narrow, vec)
            want[narrow, vec] = True
    assert {k for k in want if k != "ref"} == {(n, v) for n in (True, False) for v in (True, False)}


def test_stats_pool_refusals():
    D = 4
    out = _filled((3, 2 * D), SENT)
    x = _filled((3, 5, D), 0.0)
    with pytest.raises(ValueError, match="B too large"):
        ops.stats_pool(torch.empty((65536, 0, D), device=DEV), D, None, 1, False, EPS, torch.empty((65536, D), device=DEV))
    with pytest.raises(ValueError, match="bad sizes"):
        ops.stats_pool(x, D + 1, None, 1, False, EPS, _filled((3, 2 * D), SENT))               # ldx < D
    with pytest.raises(ValueError, match="ld_out too small"):
        ops.stats_pool(x, D, None, 1, True, EPS, _filled((3, 2 * D - 1), SENT))
    with pytest.raises(ValueError, match="input_period"):
        ops.stats_pool(x, D, None, 0, True, EPS, out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all()


# ----------------------------------------------------------------------------- ktf_stats_pool_windowed_f32
@pytest.mark.parametrize("name", sorted(P.WINDOWED_CASES))
def test_stats_pool_windowed(name):
    c = P.WINDOWED_CASES[name]
    x = P.windowed_data(c)
    start, T_out = P.window_steps(c["T"], c["left"], c["right"], c["output_period"], c["padding"])
    want, bound = P.pool_windowed(x, c["left"], c["right"], c["input_period"], c["output_period"], start, T_out, c["include_std"], EPS,
                                  exact=c["exact"])
    got = ops.stats_pool_windowed(_dev(x), c["left"], c["right"], c["input_period"], c["output_period"], start, T_out, c["include_std"], EPS)
    got = got.cpu().numpy()
    assert got.shape == want.shape
    D = c["D"]
    r = dict(mean=P.ratio(got[..., :D], want[..., :D], bound[..., :D]), std=P.ratio(got[..., D:], want[..., D:], bound[..., D:]))
    _note("stats_pool_windowed", f"{name} rows without a frame: {int(np.isnan(want[..., 0]).sum())}", **r)
    assert max(r.values()) <= 1.0, r


# ----------------------------------------------------------------------------- ktf_stats_finalize{,_slots,_flat}
@pytest.mark.parametrize("name", sorted(P.FINALIZE_CASES))
def test_stats_finalize(name):
    c = P.FINALIZE_CASES[name]
    d = P.finalize_data(c, flat_slots=ops.flat_stats_slots(c["T"]) if c["form"] == "flat" else None)
    want, bound = P.finalize(d["sums"], d["lens"], d["used"], c["include_std"], EPS)
    B, D = c["B"], c["D"]
    od = want.shape[1]
    out = _filled((B, od + c["ld_out_extra"]), SENT)
    sums = _dev(d["sums"])                                       # (the slots an utterance does not use hold NaN)
    if c["form"] == "flat":
        ops.stats_finalize_flat(sums, _i32(d["starts"]), c["T"], D, c["include_std"], EPS, out, d["slots"])
    else:
        ops.stats_finalize(sums, _i32(d["lens"]), c["T"], D, c["include_std"], EPS, out, slots=d["slots"], slot_rows=c["slot_rows"] or 128)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:, od:] == SENT).all()
    r = dict(mean=P.ratio(got[:, :D], want[:, :D], bound[:, :D]))
    if c["include_std"]:
        r["std"] = P.ratio(got[:, D:od], want[:, D:], bound[:, D:])
    _note("stats_finalize", f"{name} used={d['used']}", **r)
    assert max(r.values()) <= 1.0, r
    assert np.isnan(got[1, :od]).all()                           # the utterance without a row


# ----------------------------------------------------------------------------- ktf_xvec_post_f32
def run_post(x, mean, A, off):
    out = _filled((x.shape[0], A.shape[1]), NAN)
    res = ops.xvec_post(_dev(x), _dev(mean), _dev(A), _dev(off), out=out)
    torch.cuda.synchronize()
    assert res is out
    return out.cpu().numpy()


@pytest.mark.parametrize("name", sorted(P.POST_CASES))
def test_xvec_post(name):
    c = P.POST_CASES[name]
    x, mean, A, off = P.post_data(c)
    r = P.post(x, mean, A, off)
    got = run_post(x, mean, A, off)
    bound = P.EXACT_Y * np.abs(r["y"]) if c["regime"] == "int" else r["e_y"]
    ratio = P.ratio(got, r["y"], bound)
    _note("xvec_post_" + c["regime"], f"{name} eb={c['eb']}", y=ratio)
    assert ratio <= 1.0, ratio
    # an embedding's bits are the same in every batch
    if c["B"] > 1:
        for b in (0, 1, c["B"] - 1):
            assert _same_bits(run_post(x[b:b + 1], mean, A, off)[0], got[b]), b
        assert _same_bits(run_post(x[:256], mean, A, off), got[:256])                     # one embedding per workgroup


def test_xvec_post_refusals():
    x, A = _filled((1, 16000), 0.0), _filled((16000, 1), 0.0)
    assert not P.post_fits(16000, 1)
    with pytest.raises(ValueError, match="dims too large"):
        ops.xvec_post(x, None, A, None)


# ----------------------------------------------------------------------------- ktf_xvec_tail_f32
def _w_buffer(W, extra):
    """(units, in_pad + extra) device tensor: W, then 1e30 up to the multiple of four the kernel loads (it multiplies them by the
    zeros behind the pooled vector), then NaN."""
    units, in_dim = W.shape
    in_pad = (in_dim + 3) & ~3
    host = np.full((units, in_pad + extra), NAN, dtype=F32)
    host[:, :in_pad] = 1e30
    host[:, :in_dim] = W
    return _dev(host)


def run_tail(c, d, group=None, rows=None, launches=1):
    """The case's launch (or with another `group`, or of the utterances `rows` alone) -> (y, h_out or None) as numpy. Outputs start
    as NaN -- as SENT with skip_empty, whose rows must stay --; `launches` > 1 repeats the launch on the same counters, zeroed
    once, with the outputs poisoned again."""
    rows = list(range(c["B"])) if rows is None else rows
    B, I = len(rows), c["in_dim"]
    group = c["group"] if group is None else group
    lens = None if d["lens"] is None else [d["lens"][b] for b in rows]
    pooled = sums = None
    slots, slot_rows = 0, 128
    if c["source"] in ("pooled", "pooled_ld5"):
        ld = I + (5 if c["source"] == "pooled_ld5" else 0)
        host = np.full((B, ld), NAN, dtype=F32)
        host[:, :I] = d["pooled"][rows]
        pooled = _dev(host)[:, :I]
    else:
        sums, slots, slot_rows = _dev(d["sums"][rows]), d["slots"], d["slot_rows"]
    W = _w_buffer(d["W"], c["ldw_extra"])
    bias, mean, A, off = _dev(d["bias"]), _dev(d["mean"]), _dev(d["A"]), _dev(d["off"])
    fill = SENT if c["skip_empty"] else NAN
    counters = torch.zeros((B,), dtype=torch.int32, device=DEV)
    for _ in range(launches):
        partial = _filled((B, 64, c["out_dim"]), NAN)
        y = _filled((B, c["out_dim"]), fill)
        h = _filled((B, c["units"]), fill) if c["h_out"] else None
        ops.xvec_tail(pooled, sums, slots, _i32(lens), P.TAIL_T, c["D"], c["include_std"], d["eps"], W, bias, c["units"], mean, A, off, partial,
                      counters, y, h_out=h, group=group, slot_rows=slot_rows, skip_empty=c["skip_empty"])
        torch.cuda.synchronize()
        assert not counters.any()                                # the last arriver leaves the ticket counter at zero
    return y.cpu().numpy(), None if h is None else h.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _tail_ref(name):
    c = P.TAIL_CASES[name]
    d = P.tail_data(c)
    return d, P.tail_reference(c, d)


def check_tail(c, d, r, y, h, tag):
    live = np.array([not c["skip_empty"] or n > 0 for n in (d["lens"] or [1] * c["B"])])
    integer = c["regime"] == "int"
    ratios = {}
    if h is not None:
        assert (h[~live] == SENT).all()
        if integer:
            assert _same_bits(h[live], r["h"][live].astype(F32))
        else:
            ratios["h"] = P.ratio(h[live], r["h"][live], r["e_h"][live])
    assert (y[~live] == SENT).all()
    ratios["y"] = P.ratio(y[live], r["y"][live], (P.EXACT_Y * np.abs(r["y"]) if integer else r["e_y"])[live])
    _note("xvec_tail_" + c["regime"], tag, **ratios)
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("name", sorted(P.TAIL_CASES))
def test_xvec_tail(name):
    c = P.TAIL_CASES[name]
    d, r = _tail_ref(name)
    # the ticket form twice on the same counters: the second launch finds them reset
    y, h = run_tail(c, d, launches=1 if c["two_phase"] else 2)
    check_tail(c, d, r, y, h, f"{name} two_phase={c['two_phase']}")
    if not c["skip_empty"] and d["lens"] and 0 in d["lens"] and d["e_pooled"] is not None:
        empty = np.array(d["lens"]) == 0
        assert np.isnan(y[empty]).all() and np.isnan(h[empty]).all() and not np.isnan(y[~empty]).any()


@pytest.mark.parametrize("name", ["t301_u130_o256_ld5_g32", "t70_u65_o33_sums_g32", "t70_u65_o33_slots64"])
def test_xvec_tail_bits_do_not_depend_on_group_or_batch(name):
    c = P.TAIL_CASES[name]
    d, _ = _tail_ref(name)
    y, h = run_tail(c, d)
    for group in (1, 2, 32, 1024):
        yg, hg = run_tail(c, d, group=group)
        assert _same_bits(yg, y) and _same_bits(hg, h), group
    for b in (0, c["B"] // 2, c["B"] - 1):
        y1, h1 = run_tail(c, d, group=1, rows=[b])
        assert _same_bits(y1[0], y[b]) and _same_bits(h1[0], h[b]), b


@pytest.mark.parametrize("name", ["t70_u65_o33_slots64", "t70_u64_o150_slots128_g2", "t2_u7_o33_sums", "t70_u65_o33_slots128_empty_nan"])
def test_xvec_tail_from_sums_is_finalize_then_the_pooled_source(name):
    c = P.TAIL_CASES[name]
    d, _ = _tail_ref(name)
    y, h = run_tail(c, d)
    pooled = _filled((c["B"], c["in_dim"]), NAN)
    ops.stats_finalize(_dev(d["sums"]), _i32(d["lens"]), P.TAIL_T, c["D"], c["include_std"], d["eps"], pooled,
                       slots=d["slots"], slot_rows=d["slot_rows"])
    torch.cuda.synchronize()
    c2, d2 = dict(c, source="pooled"), dict(d, pooled=pooled.cpu().numpy())
    y2, h2 = run_tail(c2, d2)
    assert _same_bits(y2, y) and _same_bits(h2, h)


def test_xvec_tail_refusals():
    def call(**kw):
        a = dict(pooled=_filled((2, 8), 0.0), sums=None, slots=0, lens=None, T=5, D=4, include_std=True, eps=EPS, W=_filled((6, 8), 0.0), bias=None, units=6,
                 mean=None, A=_filled((6, 3), 0.0), off=None, partial=_filled((2, 64, 3), NAN), counters=torch.zeros(2, dtype=torch.int32, device=DEV),
                 out=_filled((2, 3), SENT), group=1)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.xvec_tail(**a)
        torch.cuda.synchronize()
        assert (a["out"].cpu().numpy() == SENT).all()

    call(units=513, W=_filled((513, 8), 0.0), A=_filled((513, 3), 0.0))
    call(D=1537, pooled=_filled((2, 3074), 0.0), W=_filled((6, 3076), 0.0))                # in_dim 3074 (3073 is odd: include_std=False)
    call(D=3073, include_std=False, pooled=_filled((2, 3073), 0.0), W=_filled((6, 3076), 0.0))
    call(A=_filled((6, 257), 0.0), partial=_filled((2, 64, 257), NAN), out=_filled((2, 257), SENT))
    call(group=0)
    call(group=1025)
    call(sums=torch.zeros((2, 2, 4), dtype=torch.float64, device=DEV))                      # both sources
    call(pooled=None)                                                                       # neither
    call(D=3, pooled=_filled((2, 6), 0.0), W=_filled((6, 10), 0.0))                         # ldw not a multiple of 4
    call(D=3, pooled=_filled((2, 6), 0.0), W=_filled((6, 6), 0.0))                          # ... and below in_dim rounded up to one
    call(skip_empty=True)                                                                   # without lens
    call(pooled=None, sums=torch.zeros((2, 1, 2, 4), dtype=torch.float64, device=DEV), slots=1, slot_rows=4, lens=_i32([5, 5]))   # too few slots


def test_worst_ratios():
    """The summary line of this file's run (nothing to assert: every test above asserted its own)."""
    families = sorted({f for f, _ in WORST})
    for f in families:
        print(f"WORST {f}: " + ", ".join(f"{k} {v:.4f}" for (g, k), v in sorted(WORST.items()) if g == f))
    assert all(v <= 1.0 for v in WORST.values())
