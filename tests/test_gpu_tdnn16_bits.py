"""The 16-bit TDNN GEMM kernels (csrc/tdnn_bf16.hip, csrc/tdnn_split.hip, csrc/tdnn_ring.h) write the same bits as the library the
golden file was recorded with (run with `-m gpu`): tests/golden/tdnn16_bits.txt holds one line per case, its name and the sha256 of
the WHOLE output buffer -- pre-filled with a sentinel, so a row or pad column that is written where none was before shows as well.
The cases are the smallest shapes that reach every path of the tile header, the ring feed and the epilogues of each kernel: B = 3
with lens = [T, 1, 0] (and once without lens), a full M-tile plus a two-row one, a partial N-tile, wide and narrow row tails, one /
three / twenty-five K-steps, VALID padding, subsampling, bf16 and fp32 rows, with and without the BatchNorm affine, and the fused
pooling in its reproducible layout (KTF_TDNN_DET_STATS; the atomic form is not bit-reproducible and has its parity tests).
"The same bits" is not "the right values": tests/test_gpu_tdnn16_values.py compares every case here (through `launch`) with an fp64
reference, so a regenerated golden file is checked against something other than the library that wrote it.

    python tests/test_gpu_tdnn16_bits.py --write      # regenerate the golden file (only for a deliberate change of the arithmetic)
"""

import hashlib
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
from kaldi_tflite_amd import _lib as L, ops  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "tdnn16_bits.txt")
SENTINEL = 7.0
B = 3
SHORT, LONG = ([-2, 0, 2], 32), ([-2, -1, 0, 1, 2], 160)       # (context, input width): 3 K-steps (ktot 96) and 25 (ktot 800 > 768)
BF16, F32 = torch.bfloat16, torch.float32


def case(name, kernel, K=SHORT, T=130, units=260, ldy=None, act="relu", ydt=BF16, affine=True, lens=True, padding="SAME", sub=1,
         gemm=L.GEMM_BF16, xdt=BF16, mode="store", y_view=None, atomic=False):
    """lens: True = (T, 1, 0), False / None = no lens, or the B lengths as a tuple. y_view: y is the column slice [y_view, y_view + units)
    of the (B, Tout, ldy) buffer instead of the buffer itself. atomic: the pooled modes without KTF_TDNN_DET_STATS ((B, 2, units), zeroed
    by the call). (y_view and atomic: the value-only cases of test_gpu_tdnn16_values.py; no golden case sets them.)"""
    lens = (T, 1, 0) if lens is True else (tuple(int(n) for n in lens) if lens else None)
    assert lens is None or len(lens) == B
    return dict(name=name, kernel=kernel, ctx=K[0], din=K[1], T=T, units=units, ldy=units if ldy is None else ldy, act=act, ydt=ydt,
                affine=affine, lens=lens, padding=padding, sub=sub, gemm=gemm, xdt=xdt, mode=mode, y_view=y_view, atomic=atomic)


def ring16(tag, kernel, K, T):
    """tdnn_bf16h_kernel / tdnn_bf16r16_kernel: ReLU and none; stores (wide: units = ldy = 264; narrow tail and partial N-tile: 260),
    bf16 and fp32 rows, with and without the affine; VALID padding; subsampling; no lens; pooled at T and at whole 128-row blocks."""
    out = []
    for act in ("relu", None):
        for units in (264, 260):
            for ydt in (BF16, F32):
                for affine in (True, False):
                    out.append(case(f"{tag}_{act}_{units}_{'bf16' if ydt == BF16 else 'f32'}_{'bn' if affine else 'plain'}", kernel, K, T,
                                    units, act=act, ydt=ydt, affine=affine))
        for Tp in (T, T - 2):
            out.append(case(f"{tag}_{act}_pooled_T{Tp}", kernel, K, Tp, 260, act=act, affine=act == "relu", mode="pooled"))
    out.append(case(f"{tag}_valid", kernel, K, T, 264, padding="VALID"))
    out.append(case(f"{tag}_sub3", kernel, K, T, 260, sub=3, ydt=F32))
    out.append(case(f"{tag}_nolens", kernel, K, T, 260, lens=False))
    return out


def all_cases():
    c = ring16("h", "tdnn_bf16h_kernel", SHORT, 130)
    c.append(case("h_onestep", "tdnn_bf16h_kernel", ([0], 32), 130, 264))                     # nk = 1: prologue only
    c += ring16("r16", "tdnn_bf16r16_kernel", LONG, 258)
    for act in ("sigmoid", "tanh"):                                                           # tdnn_bf16r_kernel: both K shapes
        for tag, K in (("k3", SHORT), ("k25", LONG)):
            c.append(case(f"r_{act}_{tag}_bf16_bn", "tdnn_bf16r_kernel", K, 258, act=act))
            c.append(case(f"r_{act}_{tag}_f32_plain", "tdnn_bf16r_kernel", K, 258, act=act, ydt=F32, affine=False))
            c.append(case(f"r_{act}_{tag}_pooled", "tdnn_bf16r_kernel", K, 258, act=act, affine=tag == "k3", mode="pooled"))
    c.append(case("r_tanh_nolens", "tdnn_bf16r_kernel", SHORT, 258, act="tanh", lens=False))
    for act in (None, "relu", "sigmoid", "tanh"):                                             # tdnn_x3r_kernel: fp32 rows in
        x3 = dict(gemm=L.GEMM_BF16X3, xdt=F32)
        c.append(case(f"x3r_{act}_f32_bn", "tdnn_x3r_kernel", SHORT, 258, act=act, ydt=F32, **x3))
        c.append(case(f"x3r_{act}_bf16_plain", "tdnn_x3r_kernel", SHORT, 258, act=act, affine=False, **x3))
        c.append(case(f"x3r_{act}_pooled", "tdnn_x3r_kernel", SHORT, 258, act=act, affine=act in (None, "tanh"), mode="pooled", **x3))
    c.append(case("x3r_nolens", "tdnn_x3r_kernel", SHORT, 258, ydt=F32, lens=False, gemm=L.GEMM_BF16X3, xdt=F32))
    # the 128 x 128 kernels
    c.append(case("g_bf16_bn", "tdnn_bf16g_kernel", ([-2, 0, 2], 64), 130, 100))
    c.append(case("g_f32_plain_nolens", "tdnn_bf16g_kernel", ([-2, 0, 2], 64), 130, 100, ydt=F32, affine=False, lens=False))
    c.append(case("p_f32x_bf16", "tdnn_bf16_kernel<64, true, false>", ([-2, 0, 2], 64), 130, 100, xdt=F32, ydt=F32))
    c.append(case("p_f32x_bf16x3", "tdnn_bf16_kernel<64, true, true>", ([-2, 0, 2], 64), 130, 100, xdt=F32, ydt=F32, gemm=L.GEMM_BF16X3,
                  affine=False))
    c.append(case("p_bf16x_k32", "tdnn_bf16_kernel<32, false, false>", SHORT, 130, 100))
    # tdnn_x3s_kernel shares the 16x16 epilogue: per-utterance tiles and flat row tiles, planes and pooled
    c.append(case("x3s_planes", "tdnn_x3s_kernel", SHORT, 130, mode="split"))
    c.append(case("x3s_f32_plain", "tdnn_x3s_kernel", SHORT, 130, ydt=F32, affine=False, act=None, mode="split"))
    c.append(case("x3s_pooled", "tdnn_x3s_kernel", SHORT, 130, mode="split_pooled"))
    c.append(case("x3s_flat_planes", "tdnn_x3s_kernel<flat>", SHORT, 130, mode="flat"))
    c.append(case("x3s_flat_pooled", "tdnn_x3s_kernel<flat, pooled>", SHORT, 130, mode="flat_pooled"))
    return c


CASES = {c["name"]: c for c in all_cases()}


def inputs(c):
    """The case's x, W, bias, scale, shift as numpy fp32 (scale / shift None without the affine), from a generator seeded with the
    case's shape, not its name. No GPU."""
    T, D, U, nctx = c["T"], c["din"], c["units"], len(c["ctx"])
    rng = np.random.default_rng([T, D, U, nctx, c["sub"]])
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    W = (rng.standard_normal((U, nctx * D)) / np.sqrt(nctx * D)).astype(np.float32)
    bias = rng.standard_normal(U).astype(np.float32)
    sc = rng.uniform(0.5, 2.0, U).astype(np.float32) if c["affine"] else None
    sh = rng.uniform(-1.0, 1.0, U).astype(np.float32) if c["affine"] else None
    return x, W, bias, sc, sh


def launch(c):
    """Runs case c: a dict of the inputs as numpy (x, W, bias, scale, shift, lens; None where absent), the WHOLE output buffer `out`
    (a CUDA tensor pre-filled with the sentinel) and, for the pooled modes, what the finalize needs (lens_dev / starts, slots)."""
    dev = torch.device("cuda")
    T, D, U = c["T"], c["din"], c["units"]
    x, W, bias, sc_np, sh_np = inputs(c)
    sc = torch.as_tensor(sc_np, device=dev) if c["affine"] else None
    sh = torch.as_tensor(sh_np, device=dev) if c["affine"] else None
    t = ktf.layers.TDNN(U, context=list(c["ctx"]), subsampling_factor=c["sub"], padding=c["padding"], activation=c["act"], name="bits")
    t.build(x.shape)
    t.set_weights([W, bias])
    lens = torch.as_tensor(np.array(c["lens"], np.int32), device=dev) if c["lens"] else None
    Tout = t.outputTimesteps(T)
    mode = c["mode"]
    split = mode in ("split", "split_pooled", "flat", "flat_pooled")
    pooled = mode in ("pooled", "split_pooled", "flat_pooled")
    det = pooled and not c["atomic"]
    flags = L.TDNN_DET_STATS if det else 0
    if split:
        flags |= L.TDNN_K_INTERLEAVED | L.TDNN_W_TILED
        xin = torch.zeros((2, B, T, D), dtype=BF16, device=dev)
        ops.split_bf16(torch.as_tensor(x, device=dev), D, xin)
        w, w_lo, b = t.device_weights(dev, L.GEMM_BF16X3, k_interleaved=True, w_tiled=True)
        d = t.desc(L.GEMM_BF16X3, BF16, c["ydt"], flags=flags)
    else:
        xin = torch.as_tensor(x).to(c["xdt"]).to(dev)
        w, w_lo, b = t.device_weights(dev, c["gemm"])
        d = t.desc(c["gemm"], c["xdt"], c["ydt"], flags=flags)
    slots = 0
    if det:
        slots = ops.flat_stats_slots(T) if mode == "flat_pooled" else ops.stats_slots(Tout)
        out = torch.full((B, slots, 2, U), SENTINEL, dtype=torch.float64, device=dev)
    elif pooled:
        out = torch.full((B, 2, U), SENTINEL, dtype=torch.float64, device=dev)
    elif split and c["ydt"] == BF16:
        out = torch.full((2, B, Tout, c["ldy"]), SENTINEL, dtype=BF16, device=dev)          # hi and lo planes
    else:
        out = torch.full((B, Tout, c["ldy"]), SENTINEL, dtype=c["ydt"], device=dev)
    y = out if c["y_view"] is None else out[..., c["y_view"]:c["y_view"] + U]
    starts = None
    if mode in ("flat", "flat_pooled"):
        starts = ops.row_starts(lens, B, T, torch.zeros(B + 1, dtype=torch.int32, device=dev))
    if mode == "store":
        ops.tdnn(xin, lens, d, w, w_lo, b, sc, sh, y)
    elif mode == "pooled":
        ops.tdnn_stats(xin, lens, d, w, w_lo, b, sc, sh, out, zero=not det)
    elif mode == "split":
        planes = c["ydt"] == BF16
        ops.tdnn_split(xin, lens, d, w, w_lo, b, sc, sh, y[0] if planes else y, y[1] if planes else None)
    elif mode == "split_pooled":
        ops.tdnn_split_stats(xin, lens, d, w, w_lo, b, sc, sh, out, zero=not det)
    elif mode == "flat":
        ops.tdnn_split_flat(xin, starts, d, w, w_lo, b, sc, sh, y[0], y[1])
    else:
        ops.tdnn_split_flat_stats(xin, starts, d, w, w_lo, b, sc, sh, out, zero=not det)
    assert ops.last_kernel() == c["kernel"], (c["name"], ops.last_kernel())
    torch.cuda.synchronize()
    return dict(x=x, W=W, bias=bias, scale=sc_np, shift=sh_np, lens=None if lens is None else np.array(c["lens"], np.int32), out=out,
                lens_dev=lens, starts=starts, slots=slots)


def run(c):
    """sha256 of the output buffer of case c."""
    out = launch(c)["out"]
    raw = out.view(torch.int16) if out.dtype == BF16 else out
    return hashlib.sha256(raw.cpu().numpy().tobytes()).hexdigest()


def golden():
    with open(GOLDEN) as f:
        return dict(line.split() for line in f if line.strip())


def test_the_golden_file_names_every_case():
    assert sorted(golden()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_output_bits(name):
    assert run(CASES[name]) == golden()[name], name


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit(__doc__)
    lines, failed = [], []
    for name in sorted(CASES):
        try:
            lines.append(f"{name} {run(CASES[name])}\n")
        except Exception as e:      # report every case that does not run, not only the first
            failed.append(f"{name}: {type(e).__name__}: {e}")
    if failed:
        sys.exit("\n".join(failed))
    with open(GOLDEN, "w") as f:
        f.writelines(lines)
    print(f"wrote {len(lines)} cases to {GOLDEN} with library {ops.build_id()}")
