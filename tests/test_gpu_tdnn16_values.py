"""The 16-bit TDNN GEMM kernels compute the RIGHT values (run with `-m gpu`): every case of tests/test_gpu_tdnn16_bits.py -- whose golden
file only says "the same bits as before" -- and 59 value-only cases are compared with the fp64 reference of tests/_tdnn16_ref.py
inside its derived bounds, in the manner of the case's output form: fp32 rows, bf16 rows to half an ulp, hi / lo planes, the slots of the
reproducible pooling and its finalized mean | std, the totals of the atomic pooling; rows beyond an utterance's length and pad columns
keep the sentinel. The value-only cases: ldy > units, ragged batches whose last wave block is partly valid, the atomic pooled form, and
-- tdnn_bf16h_kernel only, the one kernel that tests for it -- a y that is 8-byte but not 16-byte aligned (the scalar paths of
r16_store_staged and ring_epilogue16_direct<..., true>). Each case asserts the kernel family it ran on (bits.launch).

Room the bounds leave (largest |got - want| / allowed per family on the MI355X, as each case prints it; fp32 rows and pooled sums, where
the allowance is the derived bound alone | bf16 rows and planes, where it includes the half ulp of the rounding under test):
tdnn_bf16h_kernel 0.046 | 0.999, tdnn_bf16r16_kernel 0.0024 | 0.941, tdnn_bf16r_kernel 0.016 | 0.998, tdnn_x3r_kernel 0.063 | 0.979,
tdnn_x3s_kernel 0.050 | 0.979, its flat forms 0.035 | 0.979, tdnn_bf16g_kernel 0.0061 | 0.990, tdnn_bf16_kernel<...> 0.025 | 0.994. The
worst-case accumulation term (Ktot + 1) 2^-24 sum|x w| dominates the derived bound, and rounding errors add like a random walk."""

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
from kaldi_tflite_amd import _lib as L, ops  # noqa: E402
from test_gpu_tdnn16_bits import BF16, F32, LONG, SHORT, case  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 1e-10                 # layers.StatsPooling's default, as the models pass it to the finalize
X3 = dict(gemm=L.GEMM_BF16X3, xdt=F32)
# family tag -> (kernel, K shape, T, activations, further case() arguments)
FAMILIES = {
    "h": ("tdnn_bf16h_kernel", SHORT, 130, ("relu", None), {}),
    "r16": ("tdnn_bf16r16_kernel", LONG, 258, ("relu", None), {}),
    "r": ("tdnn_bf16r_kernel", SHORT, 258, ("sigmoid", "tanh"), {}),
    "x3r": ("tdnn_x3r_kernel", SHORT, 258, (None, "relu", "sigmoid", "tanh"), X3),
}
PARTIAL = ((127, 65), (129, 17))          # lengths of utterances 1 and 2: the last wave block (128 rows) is partly valid


def extra_cases():
    c = []
    for tag, (kernel, K, T, acts, kw) in FAMILIES.items():
        for ldy in (264, 272):                                                                # ldy > units: pad columns are not written
            for ydt in (BF16, F32):
                c.append(case(f"{tag}_ldy{ldy}_{'bf16' if ydt == BF16 else 'f32'}", kernel, K, T, 260, ldy=ldy, act=acts[0], ydt=ydt, **kw))
        for l1, l2 in PARTIAL:
            c.append(case(f"{tag}_lens_{l1}_{l2}", kernel, K, T, 260, act=acts[0], lens=(T, l1, l2), ydt=F32, **kw))
            c.append(case(f"{tag}_lens_{l1}_{l2}_pooled", kernel, K, T, 260, act=acts[-1], lens=(T, l1, l2), mode="pooled", **kw))
        for act in acts:                                                                      # fp64 atomics into (B, 2, units)
            c.append(case(f"{tag}_{act}_atomic", kernel, K, T, 260, act=act, affine=act != "relu", mode="pooled", atomic=True, **kw))
    c.append(case("g_ldy104", "tdnn_bf16g_kernel", ([-2, 0, 2], 64), 130, 100, ldy=104))
    for ldy in (264, 272):
        c.append(case(f"x3s_planes_ldy{ldy}", "tdnn_x3s_kernel", SHORT, 130, ldy=ldy, mode="split"))
    for l1, l2 in PARTIAL:
        c.append(case(f"x3s_lens_{l1}_{l2}", "tdnn_x3s_kernel", SHORT, 258, lens=(258, l1, l2), mode="split"))
        c.append(case(f"x3s_lens_{l1}_{l2}_pooled", "tdnn_x3s_kernel", SHORT, 258, lens=(258, l1, l2), mode="split_pooled"))
        c.append(case(f"x3s_flat_lens_{l1}_{l2}", "tdnn_x3s_kernel<flat>", SHORT, 258, lens=(258, l1, l2), mode="flat"))
        c.append(case(f"x3s_flat_lens_{l1}_{l2}_pooled", "tdnn_x3s_kernel<flat, pooled>", SHORT, 258, lens=(258, l1, l2), mode="flat_pooled"))
    # ... and tiles full enough for the instantiation without the row-group test (SKIP, csrc/tdnn_split.hip)
    c.append(case("x3s_noskip_planes", "tdnn_x3s_kernel", SHORT, 250, lens=(250, 127, 65), mode="split"))
    c.append(case("x3s_noskip_pooled", "tdnn_x3s_kernel", SHORT, 250, lens=(250, 129, 17), mode="split_pooled"))
    c.append(case("x3s_atomic", "tdnn_x3s_kernel", SHORT, 130, mode="split_pooled", atomic=True))
    c.append(case("x3s_flat_atomic", "tdnn_x3s_kernel<flat, pooled>", SHORT, 130, mode="flat_pooled", atomic=True, act=None))
    # tdnn_bf16h_kernel alone: y 8 bytes past a 16-byte boundary (element 4 of a bf16 buffer, element 2 of an fp32 one), ldy % 8 == 0
    c.append(case("h_unaligned_bf16", "tdnn_bf16h_kernel", SHORT, 130, 260, ldy=272, y_view=4))
    c.append(case("h_unaligned_f32", "tdnn_bf16h_kernel", SHORT, 130, 260, ldy=264, y_view=2, ydt=F32, act=None))
    return c


EXTRA = {c["name"]: c for c in extra_cases()}
assert not set(EXTRA) & set(bits.CASES)
ALL = dict(bits.CASES, **EXTRA)


@functools.lru_cache(maxsize=None)
def _reference(key):
    c = dict(key)
    c["ctx"] = list(c["ctx"])
    return R.reference(c, *bits.inputs(c))


def reference(c):
    """The case's fp64 reference, computed once per (shape, operands' format, layer options, lens)."""
    keys = ("T", "din", "units", "sub", "padding", "act", "affine", "lens")
    key = tuple((k, c[k]) for k in keys) + (("ctx", tuple(c["ctx"])), ("gemm", R.GEMM_BF16X3 if R.is_x3(c) else R.GEMM_BF16), ("mode", "store"))
    return _reference(key)


def family(c):
    return c["kernel"].split("<")[0] + ("<flat>" if "flat" in c["kernel"] else "")


def raw_and_finalized(c, r):
    out = r["out"]
    if c["mode"] not in R.POOLED_MODES:
        return (out.view(torch.int16).cpu().numpy().view(np.uint16) if out.dtype == BF16 else out.cpu().numpy()), None
    U, T = c["units"], c["T"]
    fin = torch.full((bits.B, 2 * U), float("nan"), dtype=torch.float32, device=out.device)
    if r["slots"] and c["mode"] == "flat_pooled":
        ops.stats_finalize_flat(out, r["starts"], T, U, True, EPS, fin, r["slots"])
    else:
        ops.stats_finalize(out, r["lens_dev"], T, U, True, EPS, fin, slots=r["slots"], slot_rows=128)
    torch.cuda.synchronize()
    return out.cpu().numpy(), fin.cpu().numpy()


def test_the_value_only_cases_cover_what_the_golden_cases_leave_out():
    e = EXTRA.values()
    for tag in ("h", "r16", "r", "x3r"):
        mine = [c for c in e if c["name"].startswith(tag + "_")]
        assert {(c["ldy"], c["ydt"]) for c in mine if c["ldy"] > 260 and c["y_view"] is None} == {(l, d) for l in (264, 272) for d in (BF16, F32)}
        assert {c["lens"][1:] for c in mine if c["mode"] == "store" and c["lens"][1] > 1} == set(PARTIAL)
        assert {c["lens"][1:] for c in mine if c["mode"] == "pooled" and not c["atomic"]} == set(PARTIAL)
        assert {c["act"] for c in mine if c["atomic"]} == set(FAMILIES[tag][3])
    assert all(c["kernel"] == "tdnn_bf16h_kernel" for c in e if c["y_view"] is not None)


@pytest.mark.parametrize("name", sorted(ALL))
def test_output_values(name):
    c = ALL[name]
    ref = reference(c)
    raw, fin = raw_and_finalized(c, bits.launch(c))          # (launch asserts ops.last_kernel() == c["kernel"])
    res = R.check(c, ref, raw, fin, EPS)
    print(f"RATIO {family(c)} {name} {res.ratio:.4f}")
    assert res.ok, (name, res.failures)


@pytest.mark.parametrize("act", sorted(R.ACT_ULPS))
def test_device_activation_ulps(act):
    """The one term of the bound that is measured, not derived: the deviation of the device's sigmoid / tanh (apply_act, through
    ops.activation_) from fp64, in fp32 ulps of the result, over the pre-activation values of this file's cases of that activation.
    _tdnn16_ref.ACT_ULPS allows twice the figure its docstring records."""
    zs = [reference(c).z for c in ALL.values() if c["act"] == act]
    z = np.unique(np.concatenate([v[np.isfinite(v)] for v in zs]).astype(np.float32))
    z = np.concatenate([z, np.nextafter(z, np.float32(-np.inf)), np.nextafter(z, np.float32(np.inf))])      # a kernel's own z is a neighbour
    z = np.concatenate([z, np.zeros(-z.size % 256, np.float32)])
    y = torch.as_tensor(z, device="cuda").reshape(1, -1, 256).clone()
    ops.activation_(y, None, {"sigmoid": L.ACT_SIGMOID, "tanh": L.ACT_TANH}[act])
    want = R.act64(z.astype(np.float64), act)
    ulps = np.abs(y.cpu().numpy().reshape(-1).astype(np.float64) - want) / R.ulp32(want)
    print(f"ULPS {act} {ulps.max():.4f} over {z.size} values (allowed in the bounds: {R.ACT_ULPS[act]})")
    assert ulps.max() <= R.ACT_ULPS[act]
