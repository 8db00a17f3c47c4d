"""GPU tests of the single-context form of the f16mx flat-tile kernel (csrc/tdnn_mx.hip, mx_single_kernel; run with `-m gpu` on an MI355X).

A flat-tile layer with ONE context at offset 0 (tdnn4, tdnn5 + pooling) runs an instantiation of its own: interior K-loop only, chunk
bases from a running scalar instead of the K-step table, the M-phase's first fragments read under the last MFMA groups of F3. It feeds
the same operands into the same MFMAs in the same order as the general kernel, so

* its planes equal the per-utterance tiles' (ktf_tdnn_mx: the general kernel, edge K-loop) bit for bit -- one super-step with padded
  K-steps (32 features), a padded second super-step (160), four full ones (512); 32, 256 and 288 units (a second N-tile with one valid
  chunk); ReLU or none, BatchNorm affine or none; a ragged batch whose utterance boundaries fall inside tiles and whose last tile is
  partial, and a dense one (row -> utterance by division) whose last tile holds one row;
* its pooled sums match the fp64 emulation of the kernel's three products to the bound the flat pooled form is held to elsewhere
  (1e-5 of the largest pooled value), with reproducible slots and with fp64 atomics, bit-identical between two runs of the slot form;
* a one-context layer at another offset ([2], [-1]: rows ARE clamped) and a three-context layer keep the general kernel's results.

Both forms report the family "tdnn_mx_kernel<flat>" (ktf_tdnn_last_kernel names families, not instantiations): which one ran is not
observable from Python, the bit comparisons are the test."""

import numpy as np
import pytest
import torch

import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import mx, ops
from kaldi_tflite_amd import _lib as L

pytestmark = pytest.mark.gpu

BATCHES = {"ragged": (4, 300, (1, 255, 257, 300)),        # 813 flat rows: boundaries at rows 1, 256 (a tile edge), 513; 45 rows in the last tile
           "dense": (3, 171, (171, 171, 171))}            # 513 flat rows, every utterance complete: one row in the last tile


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype)


def _layer(rng, D, ctx, units):
    K = len(ctx)
    W = (rng.standard_normal((units, K * D)) / np.sqrt(K * D)).astype(np.float32)
    bias = (rng.standard_normal(units) * 0.1).astype(np.float32)
    layer = ktf.layers.TDNN(units, context=list(ctx), name="t")
    layer.build((None, None, D))
    layer.set_weights([W, bias])
    return layer


def _input(rng, B, T, D):
    return np.maximum(rng.standard_normal((B, T, D)) * np.exp2(rng.integers(-3, 3, (1, 1, D))), 0.0).astype(np.float32)     # ReLU-like


def _planes(x, lens):
    B, T, D = x.shape
    p = mx.Planes.empty(B, T, D, "cuda")
    dl = dev(lens, torch.int32)
    ops.mx_planes(dev(x), D, dl, p)
    rows = ops.flat_rows(dl, B, T, lambda role, shape, dt: torch.zeros(shape, dtype=dt, device="cuda"))
    return p, dl, rows


def _flat_equals_tiles(layer, x, lens, relu, affine, seed):
    """All four output planes of ktf_tdnn_mx_flat against ktf_tdnn_mx's: every byte, written or not (both start from the same fill)."""
    B, T, _ = x.shape
    units = layer.units
    p, dl, rows = _planes(x, lens)
    wh, wq, bd = layer.device_weights_mx(torch.device("cuda"), kernel="tile")
    d = layer.desc(L.GEMM_F16MX, torch.float32, torch.float32, act="relu" if relu else None)
    g = torch.Generator(device="cuda").manual_seed(seed)
    scale = torch.rand(units, device="cuda", generator=g) + 0.5 if affine else None
    shift = torch.randn(units, device="cuda", generator=g) if affine else None
    outs = []
    for flat in (False, True):
        o = mx.Planes.empty(B, T, units, "cuda")
        for t in (o.xh, o.xl4, o.x4, o.xs):
            t.view(torch.uint8).fill_(0x5a)
        if flat:
            ops.tdnn_mx_flat(p, rows, d, wh, wq, bd, scale, shift, o)
            assert ops.last_kernel() == "tdnn_mx_kernel<flat>"
        else:
            ops.tdnn_mx(p, dl, d, wh, wq, bd, scale, shift, o)
            assert ops.last_kernel() == "tdnn_mx_kernel"
        outs.append([t.view(torch.uint8).cpu().numpy() for t in (o.xh, o.xl4, o.x4, o.xs)])
    for name, a, b_ in zip(("xh", "xl4", "x4", "xs"), *outs):
        assert a.shape == b_.shape and np.array_equal(a, b_), name
    for bi in range(B):                                      # rows beyond the length keep the fill
        for a in outs[1]:
            assert (a.reshape(B, a.shape[1], T, -1)[bi, :, lens[bi]:] == 0x5a).all()
    written = outs[1][0].reshape(B, -1, T, 64)
    assert any((written[bi, :, :lens[bi]] != 0x5a).any() for bi in range(B)), "the flat kernel wrote nothing"


@pytest.mark.parametrize("relu,affine", [(True, False), (True, True), (False, False), (False, True)], ids=["relu", "relu_bn", "none", "none_bn"])
@pytest.mark.parametrize("units", [32, 256, 288])
@pytest.mark.parametrize("din", [32, 160, 512])
def test_single_context_planes_equal_the_per_utterance_tiles_bit_for_bit(din, units, relu, affine):
    rng = np.random.default_rng(1000 * din + units)
    layer = _layer(rng, din, [0], units)
    for B, T, lens in BATCHES.values():
        _flat_equals_tiles(layer, _input(rng, B, T, din), np.asarray(lens, np.int32), relu, affine, seed=din + units)


@pytest.mark.parametrize("ctx", [[2], [-1], [-2, 0, 2]], ids=["offset_2", "offset_m1", "three_contexts"])
def test_other_layers_keep_the_general_kernel(ctx):
    """One context at an offset other than 0 clamps rows at both ends of every utterance, so it must NOT take the single-context form
    (which never clamps); three contexts are the general kernel's ordinary case."""
    rng = np.random.default_rng(77 + len(ctx) + ctx[0])
    layer = _layer(rng, 64, ctx, 256)
    for B, T, lens in BATCHES.values():
        _flat_equals_tiles(layer, _input(rng, B, T, 64), np.asarray(lens, np.int32), True, False, seed=5)


def _emulate_pooled(layer, x, lens, scale, shift, eps=1e-10):
    """fp64: the kernel's three products on the DECODED operands (context [0]), + bias, ReLU, affine, then mean | std over each utterance."""
    B, T, D = x.shape
    units = layer.units
    Dp, Up = ops.round_up(D, 32), ops.round_up(units, 256)
    xp = np.zeros((B, T, Dp), np.float32)
    xp[:, :, :D] = x
    xh, cl, ch, sl, sh = mx.encode_activations(xp)
    blk = (B, T, Dp // 32, 32)
    Xh = xh.astype(np.float64)
    Xl = mx.decode_e2m1(cl.reshape(blk), sl).reshape(B, T, Dp)
    X4 = mx.decode_e2m1(ch.reshape(blk), sh).reshape(B, T, Dp)
    Wp = np.zeros((Up, Dp))
    Wp[:units, :D] = np.transpose(layer.kernel[0], (2, 0, 1)).astype(np.float64).reshape(units, D)
    _, _, (Wh, W4, W6) = mx.weight_images(Wp.reshape(Up, Dp // 32, 32))
    Wh, W4, W6 = (w[:units, :Dp // 32].reshape(units, Dp) for w in (Wh, W4, W6))      # (the images pad the K-steps to whole super-steps)
    out = np.zeros((B, 2 * units))
    for b in range(B):
        n = int(lens[b])
        y = Xh[b, :n] @ Wh.T + Xl[b, :n] @ W4.T + X4[b, :n] @ W6.T + layer.bias.astype(np.float64)
        y = np.maximum(y, 0.0) * scale + shift
        m = y.mean(0)
        out[b, :units] = m
        out[b, units:] = np.sqrt(np.maximum((y * y).mean(0) - m * m, 0.0) + eps)
    return out


POOLED = [(32, 32, "ragged"), (160, 288, "ragged"), (512, 256, "ragged"), (160, 256, "dense"), (512, 288, "dense"),
          (512, 1500, (7, 300, (300, 1, 129, 300, 77, 256, 213)))]      # tdnn5's widths: six N-tiles, the last with 220 units; runs of 1 .. 300 rows


@pytest.mark.parametrize("deterministic", [True, False], ids=["slots", "atomic"])
@pytest.mark.parametrize("din,units,batch", POOLED, ids=[f"{c[0]}x{c[1]}_{c[2] if isinstance(c[2], str) else 'B7'}" for c in POOLED])
def test_single_context_pooled_sums_vs_fp64_emulation(din, units, batch, deterministic):
    B, T, lens = BATCHES[batch] if isinstance(batch, str) else batch
    lens = np.asarray(lens, np.int32)
    rng = np.random.default_rng(din + units + B)
    layer = _layer(rng, din, [0], units)
    x = _input(rng, B, T, din)
    scale = rng.uniform(0.5, 1.5, units).astype(np.float32)
    shift = rng.standard_normal(units).astype(np.float32)
    p, dl, rows = _planes(x, lens)
    wh, wq, bd = layer.device_weights_mx(torch.device("cuda"), kernel="tile")
    d = layer.desc(L.GEMM_F16MX, torch.float32, torch.float32, act="relu", flags=L.TDNN_DET_STATS if deterministic else 0)
    slots = ops.flat_stats_slots(T) if deterministic else 0
    res, raw = [], []
    for _ in range(2):
        sums = torch.full((B, max(slots, 1), 2, units), 123.0, dtype=torch.float64, device="cuda")
        pooled = torch.zeros((B, 2 * units), device="cuda")
        ops.tdnn_mx_flat_stats(p, rows, d, wh, wq, bd, dev(scale), dev(shift), sums, zero=not slots)
        assert ops.last_kernel() == "tdnn_mx_kernel<flat>"
        if slots:
            ops.stats_finalize_flat(sums, rows, T, units, True, 1e-10, pooled, slots)
        else:
            ops.stats_finalize(sums, dl, T, units, True, 1e-10, pooled)
        res.append(pooled.cpu().numpy())
        raw.append(sums.cpu().numpy())
    if deterministic:
        assert np.array_equal(raw[0], raw[1]) and np.array_equal(res[0], res[1])
    want = _emulate_pooled(layer, x, lens, scale.astype(np.float64), shift.astype(np.float64))
    sc = max(1.0, float(np.abs(want).max()))
    err = float(np.abs(res[0] - want).max())
    print(f"{din}x{units} {'slots' if deterministic else 'atomic'}: max |pooled - fp64 emulation| = {err:.3e}, bound {1e-5 * sc:.3e}")
    assert err <= 1e-5 * sc, err
