"""tests/_tdnn16_ref.py checks itself, without a GPU: a numpy emulation of the 16-bit TDNN kernels' arithmetic (bf16 operands -- or the
hi / lo split of fp32 ones and the three products of KTF_GEMM_BF16X3 --, fp32 accumulation in two different K orders, the fp32 epilogue,
round-to-nearest-even packs, the hi / lo output planes, the pivot-relative pooled sums and the finalize) stands in for the kernels on the
smallest SHORT and LONG shapes of tests/test_gpu_tdnn16_bits.py. Both emulations must pass every comparison (else a bound is too tight),
and each plausible kernel mistake, applied to an emulated output, must fail one (else the comparison is too loose)."""

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

import _tdnn16_ref as R  # noqa: E402
import test_gpu_tdnn16_bits as bits  # noqa: E402
from test_gpu_tdnn16_bits import BF16, F32, LONG, SHORT, case  # noqa: E402

EPS = 1e-10
X3 = dict(gemm=R.GEMM_BF16X3, xdt=F32)
SHAPES = {"short": dict(K=SHORT, T=130), "long": dict(K=LONG, T=258)}


def forms(K, T):
    """One case per output form (the kernel names are not used here); ldy > units so that there are pad columns."""
    return {
        "f32": case("f32", "", K, T, 260, ldy=264, ydt=F32),
        "bf16": case("bf16", "", K, T, 260, ldy=264),
        "bf16_view": case("bf16_view", "", K, T, 260, ldy=272, y_view=4, act=None),
        "f32_view": case("f32_view", "", K, T, 260, ldy=264, y_view=2, ydt=F32, affine=False),
        "bf16_sigmoid": case("bf16_sigmoid", "", K, T, 260, ldy=264, act="sigmoid"),
        "f32_tanh_plain": case("f32_tanh_plain", "", K, T, 260, ldy=264, act="tanh", ydt=F32, affine=False),
        "x3_f32": case("x3_f32", "", K, T, 260, ldy=264, ydt=F32, **X3),
        "x3_f32_valid_sub": case("x3_f32_valid_sub", "", K, T, 260, ldy=264, ydt=F32, padding="VALID", sub=3, act=None, **X3),
        "planes": case("planes", "", K, T, 260, ldy=264, mode="split"),
        "pooled": case("pooled", "", K, T, 260, mode="pooled"),
        "pooled_atomic": case("pooled_atomic", "", K, T, 260, mode="pooled", atomic=True, act=None),
        "pooled_ragged": case("pooled_ragged", "", K, T, 260, mode="split_pooled", lens=(T, 127, 65)),
        "flat_pooled": case("flat_pooled", "", K, T, 260, mode="flat_pooled", lens=(T, 129, 17)),
    }


# ----------------------------------------------------------------------------- the emulation
def f32(a):
    return np.asarray(a, np.float32)


def rows_idx(c, n, T, extra=0, clip_T_last=False):
    """Input rows (Tout + extra, K) of an utterance of n frames: tdnn_common.h's row(t, k), the clamp applied in every padding mode as
    the kernels do. clip_T_last: the last valid row clamps against the buffer's T instead."""
    ctx = np.asarray(c["ctx"])
    start = -ctx[0] if c["padding"] == "VALID" and ctx[0] < 0 else 0
    nout = R.out_rows(c, n)
    t = start + np.arange(nout + extra)[:, None] * c["sub"] + ctx[None, :]
    idx = np.clip(t, 0, n - 1)
    if clip_T_last and nout:
        idx[nout - 1] = np.clip(t[nout - 1], 0, T - 1)
    return idx, nout


def accumulate(terms, bias, order):
    """fp32 sum of the exact products of `terms` = [(g (rows, K), w (U, K))] and the bias, in one of two orders."""
    rows, K = terms[0][0].shape
    U = terms[0][1].shape[0]
    if order == 0:                                  # accumulators preloaded with the bias, K ascending, one product at a time
        acc = np.broadcast_to(f32(bias), (rows, U)).copy()
        for k in range(K):
            for g, w in terms:
                acc += g[:, k:k + 1] * w[None, :, k]
        return acc
    acc = np.zeros((rows, U), np.float32)           # 32-deep K-steps, K descending, each step summed on its own; bias last
    for k in range(K - 32, -1, -32):
        for g, w in reversed(terms):
            acc += g[:, k:k + 32] @ w[:, k:k + 32].T
    return acc + f32(bias)


def activate(z, act):
    if act == "relu":
        return np.maximum(z, np.float32(0))
    if act in ("sigmoid", "tanh"):
        return f32(R.act64(z.astype(np.float64), act))          # a correctly rounded device function
    return z


def values(c, order, corrupt=None, extra=0):
    """Per utterance the fp32 epilogue values (out_len + extra rows) and the activation's values before the affine."""
    x, W, bias, sc, sh = bits.inputs(c)
    x3 = R.is_x3(c)
    xh, wh = R.bf16_rne(x), R.bf16_rne(W)
    xs, ws = [xh], [wh]
    if x3 and corrupt != "drop_lo":
        xs, ws = [xh, R.bf16_rne(x - xh), xh], [wh, wh, R.bf16_rne(W - wh)]
    if corrupt == "group_shift":
        sc, sh = sc.copy(), sh.copy()
        sc[16:32], sh[16:32] = sc[32:48], sh[32:48]
    B, T, D = x.shape
    out = []
    for b, n in enumerate(int(v) for v in R.lens_of(c, B)):
        if n <= 0:
            out.append((np.zeros((0, c["units"]), np.float32),) * 2)
            continue
        idx, _ = rows_idx(c, n, T, extra, clip_T_last=corrupt == "clip_T" and n < T)
        if idx.shape[0] == 0:
            out.append((np.zeros((0, c["units"]), np.float32),) * 2)
            continue
        terms = [(xo[b][idx].reshape(idx.shape[0], -1), wo) for xo, wo in zip(xs, ws)]
        late = corrupt == "bias_after"
        acc = accumulate(terms, np.zeros_like(bias) if late else bias, order)
        a = activate(acc, c["act"])
        if late:
            a = a + bias
        out.append((f32(a * sc) + sh if sc is not None else a, a))
    return out


def pooled_slot(v, blk_row0, order):
    """S, Q of the rows v (n, U) of one slot whose first row is row blk_row0 of its 128-row block: fp64 sums (order 1: the 32x32
    kernels), or per lane -- rows with the same (row of the block >> 2) & 3 -- in fp32 relative to the slot's first row (order 0)."""
    if order == 1 or v.shape[0] == 0:
        v64 = v.astype(np.float64)
        return v64.sum(0), (v64 * v64).sum(0)
    pv = v[0]
    S, Q = np.zeros(v.shape[1]), np.zeros(v.shape[1])
    for g in range(4):
        s = np.zeros(v.shape[1], np.float32)
        q = np.zeros(v.shape[1], np.float32)
        cnt = 0
        for r in range(v.shape[0]):
            if ((blk_row0 + r) >> 2) & 3 != g:
                continue
            u = v[r] - pv
            s = s + u
            q = f32(u.astype(np.float64) * u.astype(np.float64) + q.astype(np.float64))       # fmaf
            cnt += 1
        pd, sd = pv.astype(np.float64), s.astype(np.float64)
        S += sd + cnt * pd
        Q += q.astype(np.float64) + 2.0 * pd * sd + cnt * pd * pd
    return S, Q


def emulate(c, order, corrupt=None):
    """(raw output buffer, finalized mean | std or None) of case c, as R.check takes them."""
    U, ld, col0 = c["units"], c["ldy"], c["y_view"] or 0
    vals = values(c, order, corrupt, extra=1 if corrupt == "slot_extra_row" else 0)
    B = len(vals)
    out_len = [R.out_rows(c, int(n)) for n in R.lens_of(c, B)]
    Tout = R.out_rows(c, c["T"])
    if c["mode"] in R.POOLED_MODES:
        slots = R.slot_rows(c, out_len)
        nslots = max(k for _, k, _, _ in slots) + 1
        raw = np.full((B, nslots + 1, 2, U), R.SENTINEL)
        flat0 = np.concatenate([[0], np.cumsum(out_len)]) if c["mode"] in R.FLAT_MODES else np.zeros(B + 1, np.int64)
        for b, k, lo, hi in slots:
            last = hi == out_len[b]
            if corrupt == "slot_missing_last" and last:
                hi -= 1
            if corrupt == "slot_extra_row" and last:
                hi += 1
            v, a = vals[b][0][lo:hi], vals[b][1][lo:hi]
            S, Q = pooled_slot(v, (int(flat0[b]) + lo) & 127, order)
            if corrupt == "q_before_affine":
                Q = pooled_slot(a, (int(flat0[b]) + lo) & 127, order)[1]
            raw[b, k] = (S, Q)
        tot = np.zeros((B, 2, U))
        for b, k, _, _ in slots:
            tot[b] += raw[b, k]
        fin = np.full((B, 2 * U), np.nan, np.float32)
        for b, n in enumerate(out_len):
            if n:
                fin[b, :U], fin[b, U:] = R.finalize64(tot[b, 0], tot[b, 1], n, EPS)
        return (tot if c["atomic"] else raw), fin
    planes = c["mode"] in ("split", "flat") and c["ydt"] == BF16
    f32_rows = c["ydt"] == F32
    buf = np.full(((2,) if planes else ()) + (B, Tout, ld), R.SENTINEL, np.float32)
    for b, n in enumerate(out_len):
        v = vals[b][0]
        if f32_rows:
            buf[b, :n, col0:col0 + U] = v
            continue
        hi = R.bf16_trunc(v) if corrupt == "truncate" else R.bf16_rne(v)
        if planes:
            buf[0, b, :n, col0:col0 + U] = hi
            buf[1, b, :n, col0:col0 + U] = 0.0 if corrupt == "lo_zero" else R.bf16_rne(v - hi)
        else:
            buf[b, :n, col0:col0 + U] = hi
    tgt = buf[0] if planes else buf
    if corrupt == "row_beyond":
        tgt[1, out_len[1], col0:col0 + U] = vals[1][0][out_len[1] - 1] if out_len[1] else 0.5
    if corrupt == "pad_col":
        tgt[0, 0, col0 + U] = 0.0
    return (buf if f32_rows else R.bf16_bits(buf)), None


@functools.lru_cache(maxsize=None)
def ref_of(shape, form):
    c = forms(**SHAPES[shape])[form]
    return c, R.reference(c, *bits.inputs(c))


# ----------------------------------------------------------------------------- the bounds are not too tight
@pytest.mark.parametrize("order", (0, 1))
@pytest.mark.parametrize("form", sorted(forms(**SHAPES["short"])))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_emulated_kernels_pass(shape, form, order):
    c, ref = ref_of(shape, form)
    raw, fin = emulate(c, order)
    res = R.check(c, ref, raw, fin, EPS)
    print(f"{shape} {form} order {order}: largest |got - want| / allowed = {res.ratio:.3f}")
    assert res.ok, res.failures
    assert 0 < res.ratio <= 1


# ----------------------------------------------------------------------------- the comparisons are not too loose
CORRUPTIONS = [("group_shift", "f32"), ("group_shift", "bf16"), ("group_shift", "pooled"),
               ("bias_after", "f32"), ("bias_after", "bf16_sigmoid"), ("bias_after", "pooled"),
               ("truncate", "bf16"), ("truncate", "planes"),
               ("lo_zero", "planes"),
               ("drop_lo", "x3_f32"), ("drop_lo", "planes"), ("drop_lo", "flat_pooled"),
               ("clip_T", "f32"), ("clip_T", "bf16"), ("clip_T", "pooled_ragged"), ("clip_T", "flat_pooled"),
               ("row_beyond", "f32"), ("row_beyond", "bf16"), ("row_beyond", "planes"),
               ("pad_col", "bf16_view"), ("pad_col", "f32_view"), ("row_beyond", "bf16_view"), ("truncate", "bf16_view"),
               ("pad_col", "f32"), ("pad_col", "bf16"), ("pad_col", "planes"),
               ("slot_missing_last", "pooled"), ("slot_missing_last", "pooled_atomic"), ("slot_missing_last", "flat_pooled"),
               ("slot_extra_row", "pooled"), ("slot_extra_row", "pooled_ragged"), ("slot_extra_row", "flat_pooled"),
               ("q_before_affine", "pooled"), ("q_before_affine", "flat_pooled")]


@pytest.mark.parametrize("corrupt,form", CORRUPTIONS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_corrupted_outputs_fail(shape, corrupt, form):
    c, ref = ref_of(shape, form)
    raw, fin = emulate(c, 0, corrupt)
    res = R.check(c, ref, raw, fin, EPS)
    assert not res.ok, (shape, corrupt, form, res.ratio)
    if corrupt in ("q_before_affine",):              # the sums themselves are right: it is the squares that must be caught
        assert not any(f.startswith("sum,") or f.startswith("mean") for f in res.failures), res.failures


def test_finalized_values_alone_catch_a_wrong_slot():
    """The mean | std comparison is a check of its own: right slots, finalize of a slot too few."""
    c, ref = ref_of("short", "pooled")
    raw, _ = emulate(c, 0)
    _, fin = emulate(c, 0, "slot_missing_last")
    assert not R.check(c, ref, raw, fin, EPS).ok


# ----------------------------------------------------------------------------- the pieces
def test_bf16_rounding_helpers():
    v = np.array([1.0, 1.00390625, 1.01171875, -3.0e-3, 0.0, 7.0], np.float32)        # 1 + 2^-8 ties to even (down), 1 + 3 * 2^-8 ties up
    assert R.bf16_rne(v).tolist() == [1.0, 1.0, 1.015625, R.bf16_rne(np.float32(-3.0e-3)).item(), 0.0, 7.0]
    t = torch.tensor(np.random.default_rng(0).standard_normal(4096).astype(np.float32))
    assert np.array_equal(R.bf16_rne(t.numpy()), t.to(torch.bfloat16).to(torch.float32).numpy())
    assert np.array_equal(R.bf16_from_bits(R.bf16_bits(R.bf16_rne(t.numpy()))), R.bf16_rne(t.numpy()))
    assert R.half_ulp_bf16([1.0, 1.5, 2.0, 0.0, -0.75]).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 0.0, 2.0 ** -9]


def test_slot_partitions():
    per_utt = dict(mode="pooled")
    assert R.slot_rows(per_utt, [130, 1, 0]) == [(0, 0, 0, 128), (0, 1, 128, 130), (1, 0, 0, 1)]
    assert R.slot_rows(per_utt, [258, 129, 17]) == [(0, 0, 0, 128), (0, 1, 128, 256), (0, 2, 256, 258), (1, 0, 0, 128), (1, 1, 128, 129),
                                                    (2, 0, 0, 17)]
    flat = dict(mode="flat_pooled")           # utterances start at flat rows 0, 130, 257: 128-row blocks of the flat row space
    assert R.slot_rows(flat, [130, 127, 65]) == [(0, 0, 0, 128), (0, 1, 128, 130), (1, 0, 0, 126), (1, 1, 126, 127), (2, 0, 0, 65)]


def test_reference_rows_follow_the_oracle():
    c = forms(**SHAPES["short"])["x3_f32_valid_sub"]
    ref = R.reference(c, *bits.inputs(c))
    assert ref.out_len.tolist() == [42, 0, 0] and ref.Tout == 42          # VALID: 130 - 4 rows, every third; one frame: none
    assert np.isfinite(ref.want[0]).all() and np.isnan(ref.want[1:]).all()


# ----------------------------------------------------------------------------- the y alignment the launchers ask for
def _desc(units, K, act, gemm, xdt, ydt):
    t = bits.ktf.layers.TDNN(units, context=list(K[0]), activation=act, name="refusal")
    t.build((bits.B, 130, K[1]))
    return t.desc(gemm, xdt, ydt)


@pytest.mark.parametrize("who,units,K,act,gemm,xdt,ydt,off", [
    ("tdnn_bf16r16_kernel", 260, LONG, "relu", R.GEMM_BF16, BF16, F32, 8),
    ("tdnn_bf16r_kernel", 260, SHORT, "tanh", R.GEMM_BF16, BF16, F32, 8),
    ("tdnn_bf16r_kernel", 260, SHORT, "sigmoid", R.GEMM_BF16, BF16, BF16, 4),
    ("tdnn_x3r_kernel", 260, SHORT, "relu", R.GEMM_BF16X3, F32, F32, 8),
    ("tdnn_x3r_kernel", 260, SHORT, None, R.GEMM_BF16X3, F32, BF16, 2),
    ("tdnn_bf16g_kernel", 100, ([-2, 0, 2], 64), "relu", R.GEMM_BF16, BF16, F32, 4),
    ("tdnn_bf16g_kernel", 100, ([-2, 0, 2], 64), "relu", R.GEMM_BF16, BF16, BF16, 4),
])
def test_a_misaligned_y_is_refused_before_any_launch(who, units, K, act, gemm, xdt, ydt, off):
    """include/ktf_hip.h, next to ktf_tdnn: the families whose epilogues store 16 / 8 bytes without a test of their own. The pointers stand
    for device memory and are never followed: the refusal comes from the host-side checks (no GPU here)."""
    import ctypes as C
    from kaldi_tflite_amd import _lib as L
    lib, P = L.load(), C.c_void_p
    d = _desc(units, K, act, gemm, xdt, ydt)
    buf, y = 0x7000000, 0x7800000
    w_lo = P(buf) if gemm == R.GEMM_BF16X3 else None
    rc = lib.ktf_tdnn(P(buf), bits.B, 130, K[1], None, C.byref(d), P(buf), w_lo, P(buf), None, None, P(y + off), 264, None, None)
    assert rc == -1 and "aligned" in L.last_error(), (who, rc, L.last_error())
    with pytest.raises(ValueError):
        L.check(rc, "ktf_tdnn")


def test_misaligned_planes_are_refused_before_any_launch():
    import ctypes as C
    from kaldi_tflite_amd import _lib as L
    lib, P = L.load(), C.c_void_p
    buf, y = 0x7000000, 0x7800000
    for ydt, off_y, off_lo in ((BF16, 4, 0), (BF16, 0, 4), (F32, 8, None)):
        d = _desc(260, SHORT, "relu", R.GEMM_BF16X3, BF16, ydt)
        y_lo = None if off_lo is None else P(y + 0x100000 + off_lo)
        rc = lib.ktf_tdnn_split(P(buf), P(buf), bits.B, 130, 32, None, C.byref(d), P(buf), P(buf), P(buf), None, None, P(y + off_y), y_lo, 264,
                                None, None)
        assert rc == -1 and "aligned" in L.last_error(), (ydt, off_y, off_lo, rc, L.last_error())
        rs = (C.c_int32 * 4)(0, 130, 131, 131)
        if ydt == BF16:                            # the flat entry point shares the launcher (row_starts is not read on the host)
            rc = lib.ktf_tdnn_split_flat(P(buf), P(buf), bits.B, 130, 32, rs, None, C.byref(d), P(buf), P(buf), P(buf), None, None, P(y + off_y),
                                         y_lo, 264, None)
            assert rc == -1 and "aligned" in L.last_error(), (ydt, off_y, off_lo, rc, L.last_error())
