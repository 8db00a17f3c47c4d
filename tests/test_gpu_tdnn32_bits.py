"""The fp32, bf16-pair and gradient TDNN kernels (csrc/tdnn_f32.hip, csrc/tdnn_pair.hip, csrc/tdnn_grad.hip) write the same bits as the
library the golden file was recorded with (run with `-m gpu`): tests/golden/tdnn32_bits.txt holds one line per case, its name and the
sha256 of the WHOLE output buffer -- pre-filled with a sentinel, so a row or pad column that is written where none was before shows as
well. Inputs are Gaussian, from a generator seeded with the case's shape. The cases are the smallest shapes that reach every
instantiation the launchers choose (each forward case asserts ops.last_kernel()) and every branch of what the kernels share -- the tile
header, the small-tile K-loop, the register-staged 32x32x2 loop, the epilogue value and store: B = 3 with lens = (T, 1, 0) unless the
kernel needs more tiles (then the pattern of `lens_for`), once per family without lens; a partial N-tile and a two-row last M-tile; one,
three, five and twenty-five K-steps; VALID padding and subsampling 3; none / ReLU / sigmoid / tanh, with and without the BatchNorm
affine; fp32, bf16 and KTF_BF16P rows where the kernel has them; ldy > units, both a multiple of 4 and not; the pooled form of
tdnn_x4s_kernel in its reproducible layout (KTF_TDNN_DET_STATS; the atomic form is not bit-reproducible).
"The same bits" is not "the right values": test_output_values compares every forward case with the fp64 reference of
tests/_tdnn32_ref.py inside its derived bound; the gradient kernels have theirs in tests/test_gpu_tdnn_grad.py. Room the bounds leave
(largest |got - want| / allowed per family on the MI355X, as each case prints it; fp32 rows and pooled sums, where the allowance is the
derived bound alone | bf16 and pair rows, where it includes the half ulp of the rounding under test): tdnn_f32t_kernel and
tdnn_f32_kernel 0.125 | 0.999, tdnn_f32s_kernel 0.101 | 0.998, tdnn_f32_rowvec_kernel 0.068 | 0.989, tdnn_x4s_kernel 0.078 | 0.994.

    python tests/test_gpu_tdnn32_bits.py --write      # regenerate the golden file (only for a deliberate change of the arithmetic)
"""

import functools
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

import _tdnn16_ref as R16  # noqa: E402
import _tdnn32_ref as R  # noqa: E402
import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import _lib as L, autograd as A, ops  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "tdnn32_bits.txt")
SENTINEL = R16.SENTINEL
EPS = 1e-10
BF16, F32, PAIR = torch.bfloat16, torch.float32, R.PAIR
C3, C5 = [-2, 0, 2], [-2, -1, 0, 1, 2]
F32G, X4 = "f32", R.X4


def lens_for(B, T):
    """(T, 1, 0) and, for larger batches, T - 1, T // 2 + 1 and the same again."""
    return tuple((T, 1, 0, T - 1, T // 2 + 1)[i % 5] for i in range(B))


def case(name, kernel, ctx=C3, din=32, T=130, units=260, B=3, ldy=None, act="relu", ydt=F32, affine=True, lens=True, padding="SAME", sub=1,
         gemm=F32G, mode="store", ref_tiles=False):
    return dict(name=name, kernel=kernel, ctx=list(ctx), din=din, T=T, units=units, B=B, ldy=units if ldy is None else ldy, act=act, ydt=ydt,
                affine=affine, lens=lens_for(B, T) if lens else None, padding=padding, sub=sub, gemm=gemm, mode=mode, ref_tiles=ref_tiles,
                y_view=None, atomic=False, slot_rows=64)


def variants(tag, kernel, k1, k3, k25, rows=(F32, BF16, PAIR), Tv=None, Bs=None, **kw):
    """The options every forward family is run through: (activation, affine, rows) dealt round, ldy > units, VALID padding (at T = Tv
    where the family's T is too short for it) and subsampling (in a batch of Bs where the family needs the tiles), no lens, and the K
    shapes (context, input width) of one, three and twenty-five K-steps."""
    kw3 = dict(kw, ctx=k3[0], din=k3[1])
    kwv = dict(kw3, T=Tv) if Tv else kw3
    sub3 = dict(sub=3, B=Bs) if Bs else dict(sub=3)
    out = []
    for i, (act, affine) in enumerate(((None, False), ("relu", True), ("sigmoid", True), ("tanh", False))):
        ydt = rows[i % len(rows)]
        out.append(case(f"{tag}_{act}_{'bn' if affine else 'plain'}_{ydt if ydt == PAIR else str(ydt)[6:]}", kernel, act=act, affine=affine,
                        ydt=ydt, **kw3))
    out.append(case(f"{tag}_ldy263", kernel, ldy=263, **kw3))
    out.append(case(f"{tag}_ldy264_{'bf16' if BF16 in rows else 'pair'}", kernel, ldy=264, ydt=BF16 if BF16 in rows else PAIR, **kw3))
    out.append(case(f"{tag}_valid", kernel, padding="VALID", act=None, **kwv))
    out.append(case(f"{tag}_sub3", kernel, affine=False, **dict(kw3, **sub3)))
    out.append(case(f"{tag}_valid_sub3", kernel, padding="VALID", **dict(kwv, **sub3)))
    out.append(case(f"{tag}_nolens", kernel, lens=False, **kw3))
    out.append(case(f"{tag}_k1", kernel, **dict(kw, ctx=k1[0], din=k1[1])))
    out.append(case(f"{tag}_k25", kernel, act="tanh", **dict(kw, ctx=k25[0], din=k25[1])))
    return out


def all_cases():
    c = []
    # 128 x 128 tiles: cdiv(260, 128) * cdiv(130, 128) * 43 = 258 >= 256 workgroups; DMA-staged and (KTF_TDNN_REF_TILES) register-staged
    K32 = dict(k1=([0], 32), k3=(C3, 32), k25=(C5, 160))
    # (VALID: T = 134 keeps two row tiles; subsampling leaves one, so twice the batch)
    c += variants("t", "tdnn_f32t_kernel", B=43, Tv=134, Bs=86, **K32)
    c += variants("r2", "tdnn_f32_kernel<2, 16>", B=43, Tv=134, Bs=86, ref_tiles=True, **K32)
    c += variants("r1", "tdnn_f32_kernel<1, 32>", ref_tiles=True, **K32)
    # the 64-row small tiles: K-step 32 (din_pad % 64 != 0), K-step 64 at widths 32 / 64 / 96 (small_tile_width), fp32 and pair operands
    K30 = dict(k1=([0], 30), k3=(C3, 30), k25=(C5, 160))
    K64 = dict(k1=([0], 64), k3=(C3, 64), k25=(C5, 320))
    for tag, fam, gemm, rows in (("s", "tdnn_f32s_kernel", F32G, (F32, BF16, PAIR)), ("x", "tdnn_x4s_kernel", X4, (F32, PAIR))):
        c += variants(f"{tag}32", f"{fam}<32, 64>", gemm=gemm, rows=rows, **K30)
        c += variants(f"{tag}64x32", f"{fam}<64, 32>", gemm=gemm, rows=rows, **K64)
        c.append(case(f"{tag}64x32_k5", f"{fam}<64, 32>", ctx=C5, din=64, gemm=gemm, ydt=PAIR))          # the first refill of the ring
        for bn, units, B in ((64, 500, 20), (96, 280, 80)):                                             # 20 / 80 row tiles of 50 rows
            kw = dict(ctx=C3, din=64, T=50, units=units, B=B, gemm=gemm)
            c.append(case(f"{tag}64x{bn}_relu_bn_f32", f"{fam}<64, {bn}>", **kw))
            c.append(case(f"{tag}64x{bn}_none_plain_pair", f"{fam}<64, {bn}>", act=None, affine=False, ydt=PAIR, **kw))
            c.append(case(f"{tag}64x{bn}_tanh_nolens_ldy", f"{fam}<64, {bn}>", act="tanh", lens=False, ldy=units + 3, **kw))
    c.append(case("s64x64_full_bf16", "tdnn_f32s_kernel<64, 64>", ctx=C3, din=64, T=50, units=512, B=20, ydt=BF16))
    c.append(case("s64x96_full_bf16", "tdnn_f32s_kernel<64, 96>", ctx=C3, din=64, T=50, units=288, B=80, ydt=BF16))
    # tdnn_x4s_kernel, pooled (KTF_TDNN_DET_STATS: one slot per 64-row tile)
    P = dict(gemm=X4, mode="pooled")
    for act, affine in ((None, True), ("relu", False), ("sigmoid", False), ("tanh", True)):
        c.append(case(f"x32_{act}_pooled", "tdnn_x4s_kernel<32, 64>", ctx=C3, din=30, act=act, affine=affine, **P))
        c.append(case(f"x64x32_{act}_pooled", "tdnn_x4s_kernel<64, 32>", ctx=C3, din=64, act=act, affine=not affine, **P))
    c.append(case("x32_valid_sub3_pooled", "tdnn_x4s_kernel<32, 64>", ctx=C3, din=30, padding="VALID", sub=3, **P))
    c.append(case("x32_k25_nolens_pooled", "tdnn_x4s_kernel<32, 64>", ctx=C5, din=160, lens=False, **P))
    c.append(case("x64x32_k1_pooled", "tdnn_x4s_kernel<64, 32>", ctx=[0], din=64, **P))
    c.append(case("x64x32_k25_pooled", "tdnn_x4s_kernel<64, 32>", ctx=C5, din=320, **P))
    c.append(case("x64x64_pooled", "tdnn_x4s_kernel<64, 64>", ctx=C3, din=64, T=50, units=500, B=20, **P))
    c.append(case("x64x96_pooled", "tdnn_x4s_kernel<64, 96>", ctx=C3, din=64, T=50, units=280, B=80, **P))
    # the row-vector kernel: B * Tout <= 8
    c += variants("rv", "tdnn_f32_rowvec_kernel", T=2, Tv=6, **K32)
    return c


CASES = {c["name"]: c for c in all_cases()}

# The gradient GEMMs (grad_dx_kernel<1, 2>, grad_dw_kernel<2, 2>): dx, dW and dbias are hashed together. B * Tout just above the 512 rows
# of a weight-gradient slot, clamped first / last rows (SAME) and VALID padding, subsampling, units and din that are no multiples of 64,
# a one-frame and a zero-length utterance.
GRAD_CASES = {
    "grad_same": dict(ctx=C3, padding="SAME", sub=1, din=30, units=130, B=5, T=104),                     # 520 rows
    "grad_valid_sub3": dict(ctx=[-3, 0, 3], padding="VALID", sub=3, din=30, units=130, B=16, T=104),    # 16 x 33 = 528 rows
    "grad_k5_full": dict(ctx=C5, padding="SAME", sub=1, din=64, units=256, B=5, T=104),
    "grad_sub3_same": dict(ctx=[-1, 2], padding="SAME", sub=3, din=23, units=70, B=15, T=104),          # 15 x 35 = 525 rows
}


def inputs(c):
    """The case's x, W, bias, scale, shift as numpy fp32 (scale / shift None without the affine). No GPU."""
    B, T, D, U, nctx = c["B"], c["T"], c["din"], c["units"], len(c["ctx"])
    rng = np.random.default_rng([B, T, D, U, nctx, c["sub"]])
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    W = (rng.standard_normal((U, nctx * D)) / np.sqrt(nctx * D)).astype(np.float32)
    bias = rng.standard_normal(U).astype(np.float32)
    sc = rng.uniform(0.5, 2.0, U).astype(np.float32) if c["affine"] else None
    sh = rng.uniform(-1.0, 1.0, U).astype(np.float32) if c["affine"] else None
    return x, W, bias, sc, sh


def launch(c):
    """Runs forward case c: the WHOLE output buffer (a CUDA tensor pre-filled with the sentinel) and what the pooled finalize needs."""
    dev = torch.device("cuda")
    B, T, D, U = c["B"], c["T"], c["din"], c["units"]
    x, W, bias, sc_np, sh_np = inputs(c)
    sc = torch.as_tensor(sc_np, device=dev) if c["affine"] else None
    sh = torch.as_tensor(sh_np, device=dev) if c["affine"] else None
    t = ktf.layers.TDNN(U, context=list(c["ctx"]), subsampling_factor=c["sub"], padding=c["padding"], activation=c["act"], name="bits32")
    t.build(x.shape)
    t.set_weights([W, bias])
    lens = torch.as_tensor(np.array(c["lens"], np.int32), device=dev) if c["lens"] else None
    Tout = t.outputTimesteps(T)
    xin = torch.zeros((B, T, ops.round_up(D, 32)), device=dev)
    xin[:, :, :D] = torch.as_tensor(x, device=dev)
    x4, pooled = c["gemm"] == X4, c["mode"] == "pooled"
    gemm = L.GEMM_BF16X4 if x4 else L.GEMM_F32
    if x4:
        xin = ops.pair_encode(xin)
    w, w_lo, b = t.device_weights(dev, gemm)
    flags = (L.TDNN_REF_TILES if c["ref_tiles"] else 0) | (L.TDNN_DET_STATS if pooled else 0)
    d = t.desc(gemm, L.PAIR if x4 else F32, L.PAIR if c["ydt"] == PAIR else c["ydt"], flags=flags)
    slots = 0
    if pooled:
        slots = ops.tdnn_stats_slots(Tout, gemm)
        out = torch.full((B, slots, 2, U), SENTINEL, dtype=torch.float64, device=dev)
        ops.tdnn_stats(xin, lens, d, w, w_lo, b, sc, sh, out, zero=False)
    else:
        out = torch.full((B, Tout, c["ldy"]), SENTINEL, dtype=BF16 if c["ydt"] == BF16 else F32, device=dev)
        ops.tdnn(xin, lens, d, w, w_lo, b, sc, sh, out)
    assert ops.last_kernel() == c["kernel"], (c["name"], ops.last_kernel())
    torch.cuda.synchronize()
    return dict(out=out, slots=slots, Tout=Tout)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update((t.view(torch.int16) if t.dtype == BF16 else t).cpu().numpy().tobytes())
    return h.hexdigest()


def run_grad(g):
    """dx (B, T, ldx), dW (units_pad, nctx * din_pad) and dbias of gradient case g, each pre-filled with the sentinel."""
    dev = torch.device("cuda")
    B, T, D, U, nctx = g["B"], g["T"], g["din"], g["units"], len(g["ctx"])
    d = A._desc(U, D, g["ctx"], g["sub"], g["padding"])
    Dp, Up, Tout = d.din_pad, ops.round_up(U, 256), ops.tdnn_out_len(T, d)
    assert (B - 1) * Tout < ops.grad_tdnn_slot_rows() < B * Tout, "the last utterance crosses the slot boundary"
    rng = np.random.default_rng([B, T, D, U, nctx, g["sub"]])
    x = torch.zeros((B, T, Dp + 4), device=dev)
    x[:, :, :D] = torch.as_tensor(rng.standard_normal((B, T, D)).astype(np.float32), device=dev)
    w = torch.zeros((Up, nctx, Dp), device=dev)
    w[:U, :, :D] = torch.as_tensor(rng.standard_normal((U, nctx, D)).astype(np.float32), device=dev)
    w = w.view(Up, nctx * Dp)
    gr = torch.as_tensor(rng.standard_normal((B, Tout, U + 3)).astype(np.float32), device=dev)
    lens = torch.as_tensor(np.array(lens_for(B, T), np.int32), device=dev)
    ws = ops.grad_tdnn_workspace(B, T, d, dev)
    ws.fill_(0xFF)
    dx = torch.full((B, T, Dp + 4), SENTINEL, device=dev)
    dw = torch.full((Up, nctx * Dp), SENTINEL, device=dev)
    db = torch.full((U,), SENTINEL, device=dev)
    ops.grad_tdnn_data(gr, lens, d, w, dx, ws)
    ops.grad_tdnn_weights(x, lens, d, gr, dw, db, ws)
    torch.cuda.synchronize()
    return sha(dx, dw, db)


def run(name):
    """sha256 of the output buffer(s) of the case."""
    return run_grad(GRAD_CASES[name]) if name in GRAD_CASES else sha(launch(CASES[name])["out"])


def golden():
    with open(GOLDEN) as f:
        return dict(line.split() for line in f if line.strip())


@functools.lru_cache(maxsize=None)
def _reference(key):
    c = dict(key)
    c["ctx"] = list(c["ctx"])
    return R.reference(c, *inputs(c))


def reference(c):
    """The case's fp64 reference, computed once per (shape, operands' format, layer options, lens)."""
    keys = ("B", "T", "din", "units", "sub", "padding", "act", "affine", "lens", "gemm")
    return _reference(tuple((k, c[k]) for k in keys) + (("ctx", tuple(c["ctx"])),))


def test_the_golden_file_names_every_case():
    assert not set(CASES) & set(GRAD_CASES)
    assert sorted(golden()) == sorted(list(CASES) + list(GRAD_CASES))


def test_the_cases_reach_every_instantiation():
    """(each launch asserts the kernel it names: naming them all is reaching them all)"""
    small = [f"<{bk}, {bn}>" for bk, bn in ((32, 64), (64, 32), (64, 64), (64, 96))]
    want = {"tdnn_f32t_kernel", "tdnn_f32_kernel<2, 16>", "tdnn_f32_kernel<1, 32>", "tdnn_f32_rowvec_kernel"}
    want |= {"tdnn_f32s_kernel" + s for s in small} | {"tdnn_x4s_kernel" + s for s in small}
    assert {c["kernel"] for c in CASES.values()} == want
    for s in small:
        mine = [c for c in CASES.values() if c["kernel"] == "tdnn_x4s_kernel" + s]
        assert {(c["mode"], c["ydt"]) for c in mine} >= {("store", F32), ("store", PAIR), ("pooled", F32)}


@pytest.mark.parametrize("name", sorted(list(CASES) + list(GRAD_CASES)))
def test_output_bits(name):
    assert run(name) == golden()[name], name


@pytest.mark.parametrize("name", sorted(CASES))
def test_output_values(name):
    c = CASES[name]
    ref = reference(c)
    r = launch(c)
    out, fin = r["out"], None
    if c["mode"] == "pooled":
        fin = torch.full((c["B"], 2 * c["units"]), float("nan"), device=out.device)
        rows = torch.as_tensor(ref.out_len.astype(np.int32), device=out.device)       # (the finalize divides by the rows pooled)
        ops.stats_finalize(out, rows, r["Tout"], c["units"], True, EPS, fin, slots=r["slots"], slot_rows=64)
        torch.cuda.synchronize()
        fin = fin.cpu().numpy()
    raw = out.view(torch.int16).cpu().numpy().view(np.uint16) if out.dtype == BF16 else out.cpu().numpy()
    res = R.check(c, ref, raw, fin, EPS)
    print(f"RATIO {c['kernel']} {name} {res.ratio:.4f}")
    assert res.ok, (name, res.failures)


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit(__doc__)
    lines, failed = [], []
    for name in sorted(list(CASES) + list(GRAD_CASES)):
        try:
            lines.append(f"{name} {run(name)}\n")
        except Exception as e:      # report every case that does not run, not only the first
            failed.append(f"{name}: {type(e).__name__}: {e}")
    if failed:
        sys.exit("\n".join(failed))
    with open(GOLDEN, "w") as f:
        f.writelines(lines)
    print(f"wrote {len(lines)} cases to {GOLDEN} with library {ops.build_id()}")
