"""tests/_tdnn_mx_ref.py checks itself, without a GPU: a numpy emulation of the f16mx TDNN kernels' arithmetic (the three products on the
decoded operands, fp32 accumulation in two different orders, the fp32 epilogue, mx.encode_activations for plane outputs, the pivot-relative
pooled sums of 128- and 96-row slots and the finalize) stands in for the kernels. Both emulations must pass every comparison (else a bound
is too tight), and each plausible kernel mistake, applied to an emulated output, must fail one (else the comparison is too loose). The
reference itself rests on oracle/ktf_oracle.py, the host-side plane packer round-trips, and the exact-arithmetic cases are certified exact
from their decoded operands."""

import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "kaldi-tflite_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _tdnn16_ref as R  # noqa: E402
import _tdnn_mx_ref as M  # noqa: E402
from kaldi_tflite_amd import mx  # noqa: E402
from oracle import ktf_oracle as O  # noqa: E402

K3 = ([-2, 0, 2], 30)            # nk 3
K8 = ([-3, -1, 0, 2], 64)        # nk 8
FORMS = {
    "f32": M.case("f32", "tile", "f32", K3, 130, ldy=264, affine=True),
    "f32_plain": M.case("f32_plain", "loader", "f32", K8, 130, ldy=263, act=None),
    "f32_valid_sub": M.case("f32_valid_sub", "tile", "f32", K3, 130, ldy=264, act=None, affine=True, padding="VALID", sub=3),
    "planes": M.case("planes", "tile", "planes", K3, 130, affine=True),
    "planes_none": M.case("planes_none", "loader", "planes", K8, 130, act=None),
    "planes_wide": M.case("planes_wide", "flat", "planes", K3, 130, act=None, inputs="wide"),
    "pooled": M.case("pooled", "tile", "pooled", K3, 130, affine=True),
    "pooled_atomic": M.case("pooled_atomic", "flat", "pooled", K8, 130, act=None, affine=True, atomic=True),
    "pooled_loader": M.case("pooled_loader", "loader", "pooled", K3, 200),
    "flat_pooled": M.case("flat_pooled", "flat", "pooled", K3, 130, affine=True),
    "exact_f32": M.case("exact_f32", "tile", "f32", K3, 130, ldy=264, affine=True, inputs="exact"),
    "exact_planes": M.case("exact_planes", "loader", "planes", K8, 130, act=None, inputs="exact"),
}


# ----------------------------------------------------------------------------- the emulation
def f32(a):
    return np.asarray(a, np.float32)


def rows_idx(c, ctx, n, T, unclamped=False):
    """Input rows (out_len, K) of an utterance of n frames, clamped in every padding mode as the kernels do. unclamped: the last output row
    clamps against the buffer's T instead (reads row `len`)."""
    ctx = np.asarray(ctx)
    start = -min(c["ctx"]) if c["padding"] == "VALID" and min(c["ctx"]) < 0 else 0
    nout = R.out_rows(c, n)
    t = start + np.arange(nout)[:, None] * c["sub"] + ctx[None, :]
    idx = np.clip(t, 0, n - 1)
    if unclamped and nout:
        idx[nout - 1] = np.clip(t[nout - 1], 0, T - 1)
    return idx


def accumulate(g, w, bias, order):
    """fp32 sum of the exact products g (rows, K) x w (U, K) and the bias, in one of two orders."""
    rows, K = g.shape
    if order == 0:                                  # accumulators start at the bias, K ascending, one product at a time
        acc = np.broadcast_to(f32(bias), (rows, w.shape[0])).copy()
        for k in range(K):
            acc += g[:, k:k + 1] * w[None, :, k]
        return acc
    acc = np.zeros((rows, w.shape[0]), np.float32)  # 32-deep steps, K descending, each step summed on its own; bias last
    for k in range(K - 32, -1, -32):
        acc += g[:, k:k + 32] @ w[:, k:k + 32].T
    return acc + f32(bias)


def values(c, order, corrupt=None):
    """Per utterance the fp32 epilogue values (out_len rows)."""
    x, W, bias, sc, sh = M.inputs(c)
    xq, Wq = M.operands(c, x, W)
    assert np.array_equal(f32(xq), xq) and np.array_equal(f32(Wq), Wq)           # the operands are fp32 numbers
    xq, Wq = f32(xq), f32(Wq)
    nb, T, D3 = xq.shape
    ctx = list(c["ctx"])
    if corrupt == "ctx_off":
        ctx[-1] += 1
    if corrupt == "drop_product":                   # x_4 w_l6 of K-step (chunk 0, context 0)
        Wq = Wq.copy()
        Wq.reshape(Wq.shape[0], len(ctx), 3, D3 // 3)[:, 0, 2, :32] = 0
    out = []
    for b, n in enumerate(int(v) for v in R.lens_of(c, nb)):
        if R.out_rows(c, n) == 0:
            out.append(np.zeros((0, c["units"]), np.float32))
            continue
        idx = rows_idx(c, ctx, n, T, unclamped=corrupt == "unclamped" and n < T)
        acc = accumulate(xq[b][idx].reshape(idx.shape[0], -1), Wq, 2 * bias if corrupt == "bias_twice" else bias, order)
        if corrupt == "relu_after":
            y = np.maximum(f32(acc * sc) + sh, np.float32(0))
        else:
            a = np.maximum(acc, np.float32(0)) if c["act"] == "relu" else acc
            y = f32(a * sc) + sh if sc is not None else a
        if corrupt == "unit_swap":
            y[:, [40, 41]] = y[:, [41, 40]]
        out.append(y)
    return out


def pooled_slot(v, blk_row0, order):
    """S, Q of the rows v (n, U) of one slot whose first row is row blk_row0 of its block: per lane -- rows with the same
    (row of the block >> 2) & 3 -- in fp32 relative to the slot's first row, rows ascending (order 0) or descending (order 1), then fp64."""
    pv = v[0]
    S, Q = np.zeros(v.shape[1]), np.zeros(v.shape[1])
    for g in range(4):
        s = np.zeros(v.shape[1], np.float32)
        q = np.zeros(v.shape[1], np.float32)
        cnt = 0
        for r in (range(v.shape[0]) if order == 0 else reversed(range(v.shape[0]))):
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
    """(raw output as M.check takes it, finalized mean | std or None) of case c."""
    U = c["units"]
    vals = values(c, order, corrupt)
    nb = len(vals)
    out_len = [R.out_rows(c, int(n)) for n in R.lens_of(c, nb)]
    Tout = R.out_rows(c, c["T"])
    if c["out"] == "pooled":
        rows = c["slot_rows"]
        slots = R.slot_rows(c, out_len)
        nslots = max(k for _, k, _, _ in slots) + 1
        raw = np.full((nb, nslots + 1, 2, U), R.SENTINEL)
        flat0 = np.concatenate([[0], np.cumsum(out_len)]) if c["mode"] in R.FLAT_MODES else np.zeros(nb + 1, np.int64)
        for b, k, lo, hi in slots:
            raw[b, k] = pooled_slot(vals[b][lo:hi], (int(flat0[b]) + lo) % rows, order)
            if corrupt == "cnt_off" and b == 0 and hi == out_len[0]:             # the partly valid last block counts a row too many
                raw[b, k, 0] += vals[b][lo].astype(np.float64)
                raw[b, k, 1] += vals[b][lo].astype(np.float64) ** 2
        if corrupt == "slot_swap":
            raw[0, [0, 1]] = raw[0, [1, 0]]
        tot = np.zeros((nb, 2, U))
        for b, k, _, _ in slots:
            tot[b] += raw[b, k]
        fin = np.full((nb, 2 * U), np.nan, np.float32)
        for b, n in enumerate(out_len):
            if n:
                fin[b, :U], fin[b, U:] = R.finalize64(tot[b, 0], tot[b, 1], n, M.EPS)
        return (tot if c["atomic"] else raw), fin
    if c["out"] == "f32":
        buf = np.full((nb, Tout, c["ldy"]), R.SENTINEL, np.float32)
        for b, n in enumerate(out_len):
            buf[b, :n, :U] = vals[b]
        if corrupt == "row_beyond":
            buf[4, out_len[4], :U] = vals[4][out_len[4] - 1]
        if corrupt == "pad_col":
            buf[0, 0, U] = 0.0
        return buf, None
    Y = np.zeros((nb, Tout, M.cdiv(U, 32) * 32), np.float32)
    for b, n in enumerate(out_len):
        Y[b, :n, :U] = vals[b]
    xh, cl, ch, sl, sh = mx.encode_activations(Y)
    blk = (nb, Tout, Y.shape[-1] // 32, 32)
    if corrupt == "x4_sign":
        i = np.argwhere((ch[0] & 7) != 0)[0]
        ch[0, i[0], i[1]] ^= 8
    if corrupt == "scale_high":
        sl = (sl + 1).astype(np.uint8)
        lo = np.clip(Y, -M.HALF_MAX, M.HALF_MAX) - xh.astype(np.float32)
        cl = mx.encode_e2m1(lo.reshape(blk), sl).reshape(Y.shape)
    if corrupt == "pad_unit":
        xh[0, 0, U + 3] = 1.0
    if corrupt == "no_clamp":
        assert (np.abs(Y) > M.HALF_MAX).any()
        with np.errstate(over="ignore"):
            xh = np.where(np.abs(Y) > M.HALF_MAX, Y.astype(np.float16), xh)
    planes = M.pack_planes(xh, cl, ch, sl, sh, lens=out_len, fill=M.FILL)
    if corrupt == "row_beyond":
        planes[3][4, 0, out_len[4]] = planes[3][4, 0, out_len[4] - 1]
    return planes, None


@functools.lru_cache(maxsize=None)
def ref_of(form):
    c = FORMS[form]
    return c, M.reference(c, *M.inputs(c))


# ----------------------------------------------------------------------------- the bounds are not too tight
@pytest.mark.parametrize("order", (0, 1))
@pytest.mark.parametrize("form", sorted(FORMS))
def test_emulated_kernels_pass(form, order):
    c, ref = ref_of(form)
    raw, fin = emulate(c, order)
    res = M.check(c, ref, raw, fin)
    print(f"{form} order {order}: largest |got - want| / allowed = {res.ratio:.3f}")
    assert res.ok, res.failures
    if c["inputs"] == "exact" and c["out"] == "f32":
        assert res.ratio == 0
    else:
        assert 0 < res.ratio <= 1


# ----------------------------------------------------------------------------- the comparisons are not too loose
CORRUPTIONS = [("unit_swap", "f32"), ("unit_swap", "planes"), ("unit_swap", "pooled"), ("unit_swap", "exact_f32"),
               ("unclamped", "f32"), ("unclamped", "planes_none"), ("unclamped", "flat_pooled"), ("unclamped", "exact_planes"),
               ("ctx_off", "f32"), ("ctx_off", "planes"), ("ctx_off", "pooled_loader"), ("ctx_off", "exact_f32"),
               ("drop_product", "f32"), ("drop_product", "planes"), ("drop_product", "exact_f32"), ("drop_product", "exact_planes"),
               ("bias_twice", "f32"), ("bias_twice", "planes_none"), ("bias_twice", "pooled_atomic"), ("bias_twice", "exact_f32"),
               ("relu_after", "f32"), ("relu_after", "planes"), ("relu_after", "pooled"), ("relu_after", "exact_f32"),
               ("pad_col", "f32"), ("pad_col", "f32_plain"), ("pad_col", "exact_f32"),
               ("row_beyond", "f32"), ("row_beyond", "f32_valid_sub"), ("row_beyond", "planes"), ("row_beyond", "planes_none"),
               ("x4_sign", "planes"), ("x4_sign", "planes_none"),
               ("scale_high", "planes"), ("scale_high", "planes_none"), ("scale_high", "planes_wide"),
               ("pad_unit", "planes"), ("pad_unit", "planes_none"),
               ("no_clamp", "planes_wide"),
               ("slot_swap", "pooled"), ("slot_swap", "pooled_loader"), ("slot_swap", "flat_pooled"),
               ("cnt_off", "pooled"), ("cnt_off", "pooled_atomic"), ("cnt_off", "pooled_loader"), ("cnt_off", "flat_pooled")]


@pytest.mark.parametrize("corrupt,form", CORRUPTIONS)
def test_corrupted_outputs_fail(corrupt, form):
    c, ref = ref_of(form)
    raw, fin = emulate(c, 0, corrupt)
    res = M.check(c, ref, raw, fin)
    assert not res.ok, (corrupt, form, res.ratio)
    tag = {"x4_sign": "(b)", "scale_high": "(c) residual scale", "pad_unit": "(d)", "no_clamp": "(a)"}.get(corrupt)
    if tag:
        assert any(f.startswith(tag) for f in res.failures), res.failures
    if corrupt == "row_beyond" and c["out"] == "planes":
        assert all(f.startswith("(e)") for f in res.failures), res.failures


def test_finalized_values_alone_catch_a_wrong_slot():
    c, ref = ref_of("pooled")
    raw, _ = emulate(c, 0)
    _, fin = emulate(c, 0, "cnt_off")
    assert not M.check(c, ref, raw, fin).ok


def test_a_constant_unit_that_is_not_summed_relative_to_the_pivot_fails():
    """The dead and the constant unit: S = n v and Q = n v^2 to fp64 rounding; a slot whose fp32 sums picked up one fp32 ulp does not pass."""
    c, ref = ref_of("pooled")
    raw, fin = emulate(c, 0)
    raw = raw.copy()
    raw[0, 0, 1, M.CONST_UNIT] *= 1 + 2.0 ** -24
    res = M.check(c, ref, raw, fin)
    assert any(f.startswith("constant unit") for f in res.failures), res.failures


# ----------------------------------------------------------------------------- the reference rests on code it does not share
@pytest.mark.parametrize("form", ["f32", "f32_plain", "f32_valid_sub"])
def test_the_reference_on_undecoded_operands_is_the_oracles_layer(form):
    """[x | 0 | 0] against [w | 0 | 0] through the K-step layout, the operand concatenation and reference_on == oracle.tdnn on the fp32
    x and W per utterance, to fp64 summation order."""
    c = FORMS[form]
    x, W, bias, sc, sh = M.inputs(c)
    ref = M.reference(c, x, W, bias, sc, sh, decoded=False)
    Wk = W.reshape(c["units"], -1).astype(np.float64)
    for b, n in enumerate(int(v) for v in R.lens_of(c, x.shape[0])):
        nout = O.tdnn_eval_indices(n, c["ctx"], c["sub"], c["padding"]).shape[0] if n else 0
        assert ref.out_len[b] == nout
        if not nout:
            continue
        y = O.tdnn(x[b:b + 1, :n], Wk, bias.astype(np.float64), context=c["ctx"], subsampling_factor=c["sub"], padding=c["padding"],
                   activation=c["act"], dtype=np.float64)[0]
        if sc is not None:
            y = y * sc.astype(np.float64) + sh.astype(np.float64)
        assert np.abs(ref.want[b, :nout] - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
        assert np.isnan(ref.want[b, nout:]).all()


def test_decoded_operands_are_the_three_products_of_test_gpu_mx():
    """The long GEMM's operands, multiplied out K-step by K-step as tests/test_gpu_mx.py::_emulate does, give the reference's z."""
    c = FORMS["f32_plain"]
    x, W, bias, _, _ = M.inputs(c)
    ref = M.reference(c, x, W, bias)
    xp = M.pad_features(x)
    nb, T, Dp = xp.shape
    xh, cl, ch, sl, sh = mx.encode_activations(xp)
    blk = (nb, T, Dp // 32, 32)
    X = [xh.astype(np.float64), mx.decode_e2m1(cl.reshape(blk), sl).reshape(nb, T, Dp), mx.decode_e2m1(ch.reshape(blk), sh).reshape(nb, T, Dp)]
    Wd = mx.weight_images_loader(M.kstep_weights(W))[2]
    K, ctx = len(c["ctx"]), c["ctx"]
    b, n = 3, T - 1
    acc = np.zeros((n, Wd[0].shape[0]))
    for ks in range((Dp // 32) * K):
        ch_, k = divmod(ks, K)
        rows = np.clip(np.arange(n) + ctx[k], 0, n - 1)
        for Xj, Wj in zip(X, Wd):
            acc += Xj[b, rows, ch_ * 32:ch_ * 32 + 32] @ Wj[:, ks].T
    z = acc[:, :c["units"]] + bias
    assert np.abs(z - ref.z[b, :n]).max() <= 1e-12 * np.abs(z).max()


# ----------------------------------------------------------------------------- the pieces
def test_the_packer_round_trips():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((3, 37, 70)) * np.exp2(rng.integers(-20, 20, (3, 37, 70)))).astype(np.float32)
    enc = mx.encode_activations(M.pad_features(x))
    lens = [37, 5, 0]
    planes = M.pack_planes(*enc, lens=lens)
    assert [a.shape for a in planes] == [(3, 3, 37, 32), (3, 3, 37, 16), (3, 3, 37, 16), (3, 3, 37)]
    assert [a.dtype for a in planes] == [np.uint16, np.uint8, np.uint8, np.uint32]
    back = M.unpack_planes(*planes)
    for b, n in enumerate(lens):
        for got, want in zip(back, enc):
            assert np.array_equal(got[b, :n].view(np.uint8), np.ascontiguousarray(want[b, :n]).view(np.uint8))
        # the poison: NaN halves, codes -6 on a NaN scale
        assert np.isnan(back[0][b, n:].astype(np.float32)).all()
        assert (planes[1][b, :, n:] == 0xFF).all() and (planes[2][b, :, n:] == 0xFF).all() and (planes[3][b, :, n:] == 0xFFFF).all()
    filled = M.pack_planes(*enc, lens=lens, fill=M.FILL)
    for a in filled:
        assert (np.ascontiguousarray(a[1, :, 5:]).view(np.uint8) == M.FILL).all()
    # ... and the layout is mx.Planes': decoded through the module's own reader
    import torch
    P = mx.Planes(*(torch.as_tensor(a.view(d)) for a, d in zip(M.pack_planes(*enc), (np.float16, np.uint8, np.uint8, np.int32))), 70)
    blk = (3, 37, 3, 32)
    for got, want in zip(P.decode(), (enc[0].astype(np.float64), mx.decode_e2m1(enc[1].reshape(blk), enc[3]).reshape(3, 37, 96),
                                      mx.decode_e2m1(enc[2].reshape(blk), enc[4]).reshape(3, 37, 96))):
        assert np.array_equal(got, want)


def _gpu_cases():
    import test_gpu_tdnn_mx_values as G
    return G


EXACT = {**{k: c for k, c in FORMS.items() if c["inputs"] == "exact"}, **{k: c for k, c in _gpu_cases().CASES.items() if c["inputs"] == "exact"}}


@pytest.mark.parametrize("form", sorted(EXACT))
def test_the_exact_cases_are_exact_by_construction(form):
    """From the decoded operands alone, for the exact cases here and the ones tests/test_gpu_tdnn_mx_values.py launches: every term of every
    output element is a multiple of one power of two q, all three products are non-zero, and sum |terms| + |bias| (and |a s| + |h| behind
    the affine) < 2^24 q: the bound is zero."""
    c = EXACT[form]
    args = M.inputs(c)
    q, top, ok = M.exact_condition(c, *args)
    print(f"{form}: q = 2^{q}, largest sum of magnitudes {top}")
    assert ok and q == -13 and top < 2.0 ** (24 + q)
    ref = M.reference(c, *args)
    assert np.nanmax(ref.bound) == 0
    assert pow_grid_ok(ref.want, q if args[3] is None else q + M.pow2_grid(args[3]))


def pow_grid_ok(a, q):
    a = a[np.isfinite(a)]
    return bool((np.round(a / 2.0 ** q) * 2.0 ** q == a).all())


def test_subnormal_halves_count_at_their_exponent_field():
    """Item 2a of the reference's docstring: A3 takes a non-zero subnormal half at 2^-14 and every other operand as it is -- the bound of a
    case without subnormal halves is the plain (3 Ktot + 2) u (A3 + |bias|) + 3 Ktot 2^-126 of its own products."""
    assert M.nominal_halves(np.array([0.0, 2.0 ** -24, 2.0 ** -15, 2.0 ** -14, 1.0])).tolist() == [0.0, 2.0 ** -14, 2.0 ** -14, 2.0 ** -14, 1.0]
    c = FORMS["f32_plain"]
    x, W, bias, _, _ = M.inputs(c)
    x[np.abs(x) < 2.0 ** -13], W[np.abs(W) < 2.0 ** -13] = 0.0, 0.0          # no subnormal half among the operands
    xq, Wq = M.operands(c, x, W)
    plain = R.reference_on(c, xq, Wq, bias, None, None, M.dz_mx)
    ref = M.reference(c, x, W, bias)
    assert np.array_equal(ref.bound, plain.bound, equal_nan=True) and np.array_equal(ref.want, plain.want, equal_nan=True)
    cw = FORMS["planes_wide"]
    xw, Ww, bw, _, _ = M.inputs(cw)
    xq, Wq = M.operands(cw, xw, Ww)
    plain, ref = R.reference_on(cw, xq, Wq, bw, None, None, M.dz_mx), M.reference(cw, xw, Ww, bw)
    e = (np.arange(cw["units"]) * 7) % 44 - 28
    grew = np.nanmax(ref.bound / plain.bound, axis=(0, 1))
    assert (grew[e >= -4] < 1.01).all() and (grew[(e >= -22) & (e <= -16)] > 4).all() and (grew >= 1).all()
    assert (grew[e <= -24] == 1).all()                      # (weights below half the smallest subnormal: w_h = 0)


def test_pow2_grid():
    assert M.pow2_grid([0.0]) is None
    assert M.pow2_grid([1.0, 0.0, 6.0]) == 0 and M.pow2_grid([0.75, 3.0]) == -2 and M.pow2_grid([2.0 ** -14 * 6, 4.0]) == -13
    assert M.pow2_grid([2.0 ** 40]) == 40 and M.pow2_grid([1 + 2.0 ** -52]) == -52


def test_half_ulp_and_slots():
    assert M.half_ulp_f16([1.0, 1.5, 2.0, 65504.0, 2.0 ** -14, 2.0 ** -15, 0.0]).tolist() == [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 16.0, 2.0 ** -25,
                                                                                          2.0 ** -25, 2.0 ** -25]
    loader = dict(mode="pooled", slot_rows=96)
    assert R.slot_rows(loader, [200, 1, 0, 97]) == [(0, 0, 0, 96), (0, 1, 96, 192), (0, 2, 192, 200), (1, 0, 0, 1), (3, 0, 0, 96), (3, 1, 96, 97)]


def test_the_gpu_cases_reach_every_instantiation():
    """The coverage statement of tests/test_gpu_tdnn_mx_values.py needs no GPU: it is checked here too."""
    G = _gpu_cases()
    G.test_the_cases_reach_every_instantiation()
    assert all(c["kernel"] == M.FAMILY[c["family"]] for c in G.CASES.values())


def test_instances():
    assert len(M.all_instances()) == 26
    assert M.instance_of(FORMS["f32"]) == ("tdnn_mx_kernel", "RELU", "F32", True, False)
    assert M.instance_of(FORMS["pooled_atomic"]) == ("tdnn_mx_kernel", "NONE", "STATS", False, True)
    assert M.instance_of(FORMS["planes_none"]) == ("tdnn_mxl_kernel", "NONE", "PLANES", None, False)
    assert {M.instance_of(c) for c in FORMS.values()} <= M.all_instances()
