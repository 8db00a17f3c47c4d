"""The KTF_GEMM_F16MX TDNN kernels compute the RIGHT values (run with `-m gpu` on an MI355X): every one of the 26 instantiations the
launchers choose among (tdnn_mx_kernel<ACT, OUT, PADK>, tdnn_mx_kernel<ACT, OUT, PADK, FLAT>, tdnn_mxl_kernel<ACT, OUT>) and every output
form is compared with the fp64 reference of tests/_tdnn_mx_ref.py -- the kernels' own three products on the operands the MFMAs see -- inside
its derived bounds, element by element: fp32 rows (vector and scalar stores, pad columns, rows beyond the lengths keep the sentinel), the
four output planes (half plane to half an fp16 ulp, value image bit for bit from the observed half plane, residual image and its scale,
pad units, records beyond the lengths keep the fill byte), the slots of the reproducible pooling with their finalized mean | std and the
totals of the atomic pooling. The input planes are packed on the host with every row beyond an utterance's length poisoned (NaN halves,
0xFF codes and scales): a read of such a row turns the output NaN. Each case asserts the kernel family it ran on, and
test_the_cases_reach_every_instantiation proves the coverage from the launchers' rules (_tdnn_mx_ref.instance_of).

The grid: signed and ReLU-like inputs; {none, ReLU} x {no affine, affine} on every output form that takes it; nk = 1, 3, 4, 8, 25 (PADK and
not, one to seven super-steps) and context offsets beyond the utterance; ragged batches with a one-row and an empty utterance, no lens,
dense batches and T = 1 on flat tiles; units 260 and 258, ldy 260 / 263 / 288; VALID padding and subsampling on the 256-row kernel; outputs
from subnormal halves to beyond 65504; and exact-arithmetic cases whose bound is zero (every fp32 element must EQUAL the reference).

Room the bounds leave (largest |got - want| / allowed per family on the MI355X, as each case prints it; fp32 rows and pooled sums, where
the allowance is the derived bound alone | planes, where it includes the rounding under test):
tdnn_mx_kernel 0.045 (fp32 rows 0.026, pooled 0.045) | 0.9997, tdnn_mx_kernel<flat> 0.049 (pooled) | 0.9999, tdnn_mxl_kernel 0.027 (fp32 rows
0.021, pooled 0.027) | 0.9996; the exact cases: fp32 rows 0 (every element equal), planes 1.0 (a tie sits exactly half an ulp away and the
bound is zero). The worst-case accumulation term (3 Ktot + 2) 2^-24 A3 dominates the derived bound, and rounding errors add like a random
walk. One finding went into the reference instead of a kernel: with half-subnormal weights ("tile_f32_wide") the fp32 rows left the
one-rounding-per-term bound by up to 2.32 x -- v_mfma_f32_16x16x32_f16 itself, see item 2a of tests/_tdnn_mx_ref.py; with subnormal
halves taken at the magnitude of their exponent field that case sits at 0.011."""

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
import _tdnn_mx_ref as M  # noqa: E402
import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import _lib as L, mx, ops  # noqa: E402

pytestmark = pytest.mark.gpu

K1 = ([0], 32)                          # nk 1: a single context at offset 0 (always the interior loop on flat tiles); PADK
K3 = ([-2, 0, 2], 30)                   # nk 3: PADK, din not a multiple of 32
K4 = ([-2, 0], 64)                      # nk 4: one whole super-step
K8 = ([-3, -1, 0, 2], 64)               # nk 8: two
K25 = ([-2, -1, 0, 1, 2], 160)          # nk 25: PADK, seven super-steps
KW = ([-100, 0, 100], 32)               # nearly every row clamped, offsets beyond the one-row utterance
OUTS = {"tile": ("f32", "planes", "pooled", "atomic"), "flat": ("planes", "pooled", "atomic"), "loader": ("f32", "planes", "pooled", "atomic")}


def rows_of(family, out):
    """T: 600 = an edge tile, an interior tile and an 88-row partial tile of the 256-row kernel; 130 = flat 192-row loader tiles that span
    utterances and contain the empty one; 200 = 192 + 8 rows of the loader kernel's per-utterance pooled tiles."""
    if family != "loader":
        return 600
    return 200 if out in ("pooled", "atomic") else 130


def mk(name, family, out, K, T=None, **kw):
    return M.case(name, family, "pooled" if out == "atomic" else out, K, rows_of(family, out) if T is None else T, atomic=out == "atomic", **kw)


def cases():
    c = []
    for family, outs in OUTS.items():
        i = 0
        for out in outs:
            # the epilogue grid on a ragged batch, PADK (nk 3) and not (nk 8)
            for act in (None, "relu"):
                for affine in (False, True):
                    if family == "loader" and out == "planes" and affine:
                        continue                                         # refused: test_the_launchers_refuse_what_they_do_not_take
                    for K in (K3, K8):
                        c.append(mk(f"{family}_{out}_{act or 'none'}_{'affine' if affine else 'plain'}_nk{M.cdiv(K[1], 32) * len(K[0])}", family, out, K,
                                    act=act, affine=affine, zeros=i % 2 == 1))
                        i += 1
            # no lens argument
            c.append(mk(f"{family}_{out}_nolens", family, out, K4, T=300 if family != "loader" else None, lens=None, batch=3,
                        affine=not (family == "loader" and out == "planes")))
    # flat tiles: every utterance complete (rows by division), and T = 1 (t_div_m == 0)
    for out in OUTS["flat"]:
        c.append(mk(f"flat_{out}_dense", "flat", out, K4, T=300, lens=(300,) * 3, act=None, affine=True))
    c.append(mk("flat_planes_T1", "flat", "planes", K3, T=1, lens=(1,) * 300, affine=True))
    c.append(mk("flat_pooled_T1", "flat", "pooled", K3, T=1, lens=(1,) * 300, act=None))
    # K: nk 1, 4, 25 and context offsets larger than the utterances
    c += [mk("tile_f32_nk1", "tile", "f32", K1, act=None, affine=True), mk("tile_planes_nk4", "tile", "planes", K4, affine=True),
          mk("tile_pooled_nk25", "tile", "pooled", K25, zeros=True), mk("tile_f32_nk25", "tile", "f32", K25, act=None),
          mk("tile_f32_wide_ctx", "tile", "f32", KW, T=130), mk("tile_pooled_wide_ctx", "tile", "pooled", KW, T=130, act=None, affine=True),
          mk("flat_planes_nk1", "flat", "planes", K1, act=None, affine=True), mk("flat_pooled_nk4", "flat", "pooled", K4, act=None, affine=True),
          mk("flat_planes_nk25", "flat", "planes", K25, zeros=True), mk("flat_pooled_nk1", "flat", "pooled", K1),
          mk("flat_planes_wide_ctx", "flat", "planes", KW, T=130, act=None), mk("flat_pooled_wide_ctx", "flat", "pooled", KW, T=130, affine=True),
          mk("loader_f32_nk1", "loader", "f32", K1, affine=True), mk("loader_planes_nk4", "loader", "planes", K4, act=None),
          mk("loader_f32_nk25", "loader", "f32", K25, act=None, affine=True), mk("loader_pooled_nk25", "loader", "pooled", K25, zeros=True),
          mk("loader_f32_wide_ctx", "loader", "f32", KW, act=None), mk("loader_planes_wide_ctx", "loader", "planes", KW),
          mk("loader_pooled_wide_ctx", "loader", "pooled", KW, T=130, act=None)]
    # columns: ldy 260 (vector stores) is the grid above; 263 (scalar stores), 288 (pad columns); units 258 (the last four straddle units)
    for family in ("tile", "loader"):
        c += [mk(f"{family}_f32_ldy263", family, "f32", K3, ldy=263, affine=True), mk(f"{family}_f32_ldy288", family, "f32", K8, ldy=288, act=None),
              mk(f"{family}_f32_units258", family, "f32", K4, units=258, ldy=260, act=None, affine=True),
              mk(f"{family}_planes_units258", family, "planes", K4, units=258)]
    c += [mk("flat_planes_units258", "flat", "planes", K4, units=258, affine=True), mk("flat_pooled_units258", "flat", "pooled", K4, units=258)]
    # VALID padding and subsampling (256-row kernel only): two M-tiles of outputs
    for i, (padding, sub) in enumerate((("VALID", 1), ("SAME", 3), ("VALID", 3))):
        T = 600 if sub == 1 else 800
        c.append(mk(f"tile_f32_{padding}_sub{sub}", "tile", "f32", K3, T=T, padding=padding, sub=sub, act=None if i % 2 else "relu", affine=i != 1, ldy=264))
        c.append(mk(f"tile_planes_{padding}_sub{sub}", "tile", "planes", K8, T=T, padding=padding, sub=sub, act="relu" if i % 2 else None, affine=i == 1))
    # outputs from subnormal halves to beyond 65504
    c += [mk("tile_planes_wide", "tile", "planes", K3, act=None, affine=True, inputs="wide"), mk("tile_f32_wide", "tile", "f32", K3, act=None, inputs="wide"),
          mk("flat_planes_wide", "flat", "planes", K8, act=None, inputs="wide"), mk("flat_planes_wide_relu", "flat", "planes", K3, inputs="wide"),
          mk("loader_planes_wide", "loader", "planes", K8, act=None, inputs="wide"), mk("loader_planes_wide_relu", "loader", "planes", K3, inputs="wide")]
    # exact arithmetic: the bound is zero (tests/test_tdnn_mx_ref_cpu.py certifies these very cases)
    c += [mk("tile_f32_exact_nk3", "tile", "f32", K3, affine=True, inputs="exact"), mk("tile_planes_exact_nk8", "tile", "planes", K8, act=None, affine=True, inputs="exact"),
          mk("flat_planes_exact_nk3", "flat", "planes", K3, act=None, affine=True, inputs="exact"), mk("flat_planes_exact_nk8", "flat", "planes", K8, inputs="exact"),
          mk("loader_f32_exact_nk8", "loader", "f32", K8, act=None, affine=True, inputs="exact"), mk("loader_planes_exact_nk3", "loader", "planes", K3, inputs="exact")]
    return c


CASES = {c["name"]: c for c in cases()}
assert len(CASES) == len(cases())


@functools.lru_cache(maxsize=None)
def _reference(key):
    c = dict(key)
    c["ctx"] = list(c["ctx"])
    return M.reference(c, *M.inputs(c))


def reference(c):
    """The case's fp64 reference, computed once per (shape, inputs, layer options, lens); it does not depend on the kernel or the output form."""
    keys = ("T", "din", "units", "sub", "padding", "act", "affine", "lens", "B", "inputs", "zeros", "seed")
    return _reference(tuple((k, c[k]) for k in keys) + (("ctx", tuple(c["ctx"])), ("mode", "store"), ("slot_rows", 128), ("y_view", None)))


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    return t if dtype is None else t.to(dtype)


def launch(c):
    """One launch of the case's entry point on host-built planes -> (raw, finalized) as M.check takes them."""
    x, W, bias, sc, sh = M.inputs(c)
    nb, T, D = x.shape
    U, K = c["units"], len(c["ctx"])
    layer = ktf.layers.TDNN(U, context=list(c["ctx"]), padding=c["padding"], subsampling_factor=c["sub"], name="t")
    layer.build((None, None, D))
    layer.set_weights([W.reshape(U, K * D), bias])
    ph, pl, p4, ps = M.input_planes(c, x)
    p = mx.Planes(dev(ph.view(np.float16)), dev(pl), dev(p4), dev(ps.view(np.int32)), D)
    lens = R.lens_of(c, nb)
    dl = dev(lens, torch.int32) if c["lens"] is not None else None
    loader, flat, pooled = c["family"] == "loader", c["family"] == "flat", c["out"] == "pooled"
    det = pooled and not c["atomic"]
    flags = (L.TDNN_MX_LOADER if loader else 0) | (L.TDNN_DET_STATS if det else 0)
    wh, wq, bd = layer.device_weights_mx(torch.device("cuda"), kernel="loader" if loader else "tile")
    d = layer.desc(L.GEMM_F16MX, torch.float32, torch.float32, act="relu" if c["act"] == "relu" else None, flags=flags)
    Tout = ops.tdnn_out_len(T, d)
    assert Tout == R.out_rows(c, T)
    scale, shift = (dev(sc), dev(sh)) if sc is not None else (None, None)
    rows = ops.flat_rows(dl, nb, T, lambda role, shape, dt: torch.zeros(shape, dtype=dt, device="cuda")) if flat else None
    if c["out"] == "f32":
        y = torch.full((nb, Tout, c["ldy"]), M.SENTINEL, device="cuda")
        ops.tdnn_mx(p, dl, d, wh, wq, bd, scale, shift, y)
        assert ops.last_kernel() == c["kernel"]
        return y.cpu().numpy(), None
    if c["out"] == "planes":
        o = mx.Planes.empty(nb, Tout, U, "cuda")
        for t in (o.xh, o.xl4, o.x4, o.xs):
            t.view(torch.uint8).fill_(M.FILL)
        if flat:
            ops.tdnn_mx_flat(p, rows, d, wh, wq, bd, scale, shift, o)
        else:
            ops.tdnn_mx(p, dl, d, wh, wq, bd, scale, shift, o)
        assert ops.last_kernel() == c["kernel"]
        return (o.xh.view(torch.int16).cpu().numpy().view(np.uint16), o.xl4.cpu().numpy(), o.x4.cpu().numpy(), o.xs.cpu().numpy().view(np.uint32)), None
    slots = (ops.flat_stats_slots(T) if flat else ops.stats_slots(T, mx_flags=flags)) if det else 0
    sums = torch.full((nb, slots, 2, U) if det else (nb, 2, U), 3.0, dtype=torch.float64, device="cuda")
    if flat:
        ops.tdnn_mx_flat_stats(p, rows, d, wh, wq, bd, scale, shift, sums, zero=not det)
    else:
        ops.tdnn_mx_stats(p, dl, d, wh, wq, bd, scale, shift, sums, zero=not det)
    assert ops.last_kernel() == c["kernel"]
    fin = torch.full((nb, 2 * U), float("nan"), device="cuda")
    if det and flat:
        ops.stats_finalize_flat(sums, rows, T, U, True, M.EPS, fin, slots)
    else:
        ops.stats_finalize(sums, dev(lens, torch.int32), T, U, True, M.EPS, fin, slots=slots, slot_rows=ops.mx_slot_rows(flags))
    torch.cuda.synchronize()
    return sums.cpu().numpy(), fin.cpu().numpy()


def form(c):
    return "atomic" if c["atomic"] else c["out"]


def test_the_cases_reach_every_instantiation():
    """{instance_of(case)} is the full set of 26 kernels, and every (family, output form) has a ragged, a no-lens, an affine and a
    no-affine case; both activations meet both affine settings wherever the launcher takes the affine."""
    cs = list(CASES.values())
    assert {M.instance_of(c) for c in cs} == M.all_instances() and len(M.all_instances()) == 26
    for family, outs in OUTS.items():
        for out in outs:
            mine = [c for c in cs if c["family"] == family and form(c) == out]
            assert any(c["lens"] is None for c in mine), (family, out)
            assert any(c["lens"] is not None and 0 in c["lens"] and 1 in c["lens"] for c in mine), (family, out)
            want = {(a, f) for a in (None, "relu") for f in (False, True)}
            if family == "loader" and out == "planes":
                want = {(a, False) for a in (None, "relu")}
            assert {(c["act"], c["affine"]) for c in mine} == want, (family, out)
            assert {(M.nk_of(c) & 3) != 0 for c in mine} == {True, False}, (family, out)
    for family in OUTS:
        mine = [c for c in cs if c["family"] == family]
        assert {M.nk_of(c) for c in mine} >= {1, 3, 4, 8, 25}
        assert sum(c["inputs"] == "exact" for c in mine) == 2 and {M.nk_of(c) for c in mine if c["inputs"] == "exact"} == {3, 8}
        assert any(c["inputs"] == "wide" for c in mine) and any(c["ctx"] == KW[0] for c in mine)
    assert {c["ldy"] for c in cs if c["out"] == "f32" and c["units"] == 260} >= {260, 263, 288}
    assert {(c["padding"], c["sub"], c["out"]) for c in cs if (c["padding"], c["sub"]) != ("SAME", 1)} == {
        (p_, s, o) for p_, s in (("VALID", 1), ("SAME", 3), ("VALID", 3)) for o in ("f32", "planes")}


@pytest.mark.parametrize("name", sorted(CASES))
def test_output_values(name):
    c = CASES[name]
    ref = reference(c)
    raw, fin = launch(c)
    res = M.check(c, ref, raw, fin)
    print(f"RATIO {c['kernel']} {name} {res.ratio:.4f}")
    assert res.ok, (name, M.instance_of(c), res.failures)
    if c["inputs"] == "exact" and c["out"] == "f32":
        assert res.ratio == 0


def _refused(c, match, scale=False):
    x, W, bias, _, _ = M.inputs(c)
    nb, T, D = x.shape
    U, K = c["units"], len(c["ctx"])
    layer = ktf.layers.TDNN(U, context=list(c["ctx"]), padding=c["padding"], subsampling_factor=c["sub"], name="t")
    layer.build((None, None, D))
    layer.set_weights([W.reshape(U, K * D), bias])
    ph, pl, p4, ps = M.input_planes(c, x)
    p = mx.Planes(dev(ph.view(np.float16)), dev(pl), dev(p4), dev(ps.view(np.int32)), D)
    dl = dev(R.lens_of(c, nb), torch.int32)
    loader, flat = c["family"] == "loader", c["family"] == "flat"
    flags = (L.TDNN_MX_LOADER if loader else 0) | (L.TDNN_DET_STATS if c["out"] == "pooled" else 0)
    wh, wq, bd = layer.device_weights_mx(torch.device("cuda"), kernel="loader" if loader else "tile")
    d = layer.desc(L.GEMM_F16MX, torch.float32, torch.float32, act="relu", flags=flags)
    Tout = max(ops.tdnn_out_len(T, d), 1)
    one = torch.ones(U, device="cuda") if scale else None
    with pytest.raises(ValueError, match=match):
        if c["out"] == "pooled":
            sums = torch.zeros((nb, 8, 2, U), dtype=torch.float64, device="cuda")
            if flat:
                rows = ops.flat_rows(dl, nb, T, lambda role, shape, dt: torch.zeros(shape, dtype=dt, device="cuda"))
                ops.tdnn_mx_flat_stats(p, rows, d, wh, wq, bd, one, one, sums)
            else:
                ops.tdnn_mx_stats(p, dl, d, wh, wq, bd, one, one, sums, zero=False)
        elif c["out"] == "planes":
            o = mx.Planes.empty(nb, Tout, U, "cuda")
            if flat:
                rows = ops.flat_rows(dl, nb, T, lambda role, shape, dt: torch.zeros(shape, dtype=dt, device="cuda"))
                ops.tdnn_mx_flat(p, rows, d, wh, wq, bd, one, one, o)
            else:
                ops.tdnn_mx(p, dl, d, wh, wq, bd, one, one, o)
        else:
            ops.tdnn_mx(p, dl, d, wh, wq, bd, one, one, torch.zeros((nb, Tout, U), device="cuda"))


def test_the_launchers_refuse_what_they_do_not_take():
    """The loader kernel writes planes without scale / shift; VALID padding and subsampling exist on the per-utterance tiles of the 256-row
    kernel only, for fp32 rows and planes: flat tiles, the fused pooling and the loader kernel say so instead of launching."""
    _refused(M.case("r", "loader", "planes", K3, 130), "without scale / shift", scale=True)
    for padding, sub in (("VALID", 1), ("SAME", 3)):
        kw = dict(padding=padding, sub=sub)
        _refused(M.case("r", "flat", "planes", K3, 130, **kw), "flat row tiles take")
        _refused(M.case("r", "flat", "pooled", K3, 130, **kw), "SAME padding without subsampling")
        _refused(M.case("r", "tile", "pooled", K3, 130, **kw), "SAME padding without subsampling")
        _refused(M.case("r", "loader", "pooled", K3, 130, **kw), "SAME padding without subsampling")
        _refused(M.case("r", "loader", "f32", K3, 130, **kw), "SAME padding without subsampling")
        _refused(M.case("r", "loader", "planes", K3, 130, **kw), "SAME padding without subsampling")
