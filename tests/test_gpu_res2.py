"""The Res2Net dilated convolution on the GPU (include/ktf_res2.h): bit for bit against tests/_res2_ref.py on exactly representable
inputs, the bit-level invariances of rules 1 - 5, every mode against the slice composition on the TDNN kernels (the limit is measured
on those kernels: e_new <= 2 e_comp + 2^-20 max|ref|, both round at the same points and differ in accumulation order only), and the
layer inside the fused runner in every gemm mode. Every comparison prints its figures."""

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

import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import _lib as L, ops  # noqa: E402
from oracle import ktf_oracle as O  # noqa: E402
import _res2_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77.0
MODES = {"f32": L.GEMM_F32, "bf16": L.GEMM_BF16, "bf16x3": L.GEMM_BF16X3}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows(a, ld, off, fill):
    """a (B, T, C) fp32 as a device tensor (B, T, ld) whose base lies `off` floats behind a 256-byte boundary; pad columns = fill."""
    B, T, C = a.shape
    buf = torch.full((B * T * ld + 64 + off,), fill, dtype=torch.float32, device=DEV)
    at = (-buf.data_ptr() // 4) % 64 + off
    v = buf[at:at + B * T * ld].view(B, T, ld)
    v[:, :, :C] = torch.as_tensor(a, device=DEV)
    return v


def run(c, lens, s, d, gemm=L.GEMM_F32, relu=True, bn=True, ldx=None, ldy=None, off=0, only=None):
    """One call on a copy of c["x"] with NaN in every row from the utterance's length on and in every pad column, into a y full of
    SENTINEL -> y (B, T, ldy) as numpy. `only`: that utterance alone."""
    x = np.array(c["x"] if only is None else c["x"][only:only + 1], np.float32)
    lens = lens if only is None or lens is None else lens[only:only + 1]
    B, T, C = x.shape
    for b in range(B if lens is not None else 0):
        x[b, R.clamp_len(lens[b], T):] = np.nan
    tx, ty = _rows(x, ldx or C, off, np.nan), _rows(np.full_like(x, SENTINEL), ldy or C, off, SENTINEL)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)      # noqa: E731
    ops.res2_conv(tx[:, :, :C], None if lens is None else dev(np.asarray(lens, np.int32)), s, d, dev(c["W"].reshape(s - 1, -1, C // s)), dev(c["bias"]),
                  dev(c["nscale"]) if bn else None, dev(c["nshift"]) if bn else None, L.ACT_RELU if relu else L.ACT_NONE, gemm, ty[:, :, :C])
    torch.cuda.synchronize()
    return ty.cpu().numpy()


@pytest.mark.parametrize("w,s,d", [(16, 2, 1), (16, 3, 8), (64, 8, 2), (64, 8, 4), (128, 4, 3), (128, 8, 4)])
def test_exact_inputs_give_the_reference_bit_for_bit(w, s, d):
    C = s * w
    lens = R.exact_lens(s, d, ops.res2_row_tile(w, s, d))
    c = R.exact_case(w, s, d, lens)
    for ls in (lens, None):
        ref = R.batch(c["x"], ls, s, d, c["W"], bias=c["bias"], nscale=c["nscale"], nshift=c["nshift"])
        y = run(c, ls, s, d, ldy=C + 8)
        assert (y[:, :, C:] == SENTINEL).all()
        for b, r in enumerate(ref):
            assert np.array_equal(_bits(y[b, :len(r), :C]), _bits(r)), (w, s, d, b, len(r))
            assert (y[b, len(r):] == SENTINEL).all(), (b, len(r))


@pytest.mark.parametrize("w,s,d,mode", [(16, 3, 8, "f32"), (64, 8, 2, "f32"), (64, 8, 2, "bf16x3"), (128, 4, 3, "bf16")])
def test_strides_alignment_batch_and_options_do_not_change_a_bit(w, s, d, mode):
    C, Rt = s * w, ops.res2_row_tile(w, s, d)
    lens = [Rt + 3, 0, 5, 2 * Rt + 1, (s - 1) * d + 1]
    c = R.exact_case(w, s, d, lens)
    rng = np.random.default_rng(5)
    c.update(x=rng.standard_normal(c["x"].shape).astype(np.float32), W=(rng.standard_normal(c["W"].shape) / np.sqrt(3 * w)).astype(np.float32))
    for relu, bn in ((True, True), (False, False)):
        plain = run(c, lens, s, d, MODES[mode], relu, bn)
        assert np.isfinite(plain[0, :lens[0]]).all() and np.array_equal(_bits(plain), _bits(run(c, lens, s, d, MODES[mode], relu, bn)))
        moved = run(c, lens, s, d, MODES[mode], relu, bn, ldx=C + 4, ldy=C + 8, off=4)
        assert np.array_equal(_bits(moved[:, :, :C]), _bits(plain)) and (moved[:, :, C:] == SENTINEL).all()
        for b in (0, 3):
            assert np.array_equal(_bits(run(c, lens, s, d, MODES[mode], relu, bn, only=b)[0]), _bits(plain[b])), b


def _composition(x, lens, layer, mode):
    """The layer as slices, adds and one TDNN.forward per group on the library's TDNN kernels: x (B, T, C) fp32 on the device."""
    s, w, d = layer.scale, layer.width, layer.dilation
    kernel, bias, nsc, nsh = layer.get_weights()
    ys = [x[:, :, :w]]
    for i in range(1, s):
        t = ktf.layers.TDNN(w, [-d, 0, d], name=f"group{i}")
        t.set_weights([kernel[i - 1][None], bias[i - 1]], fmt="tensorflow")
        u = (x[:, :, i * w:(i + 1) * w] + ys[-1] if i >= 2 else x[:, :, w:2 * w]).contiguous()
        bn = (torch.as_tensor(nsc[i - 1], device=DEV), torch.as_tensor(nsh[i - 1], device=DEV))
        ys.append(t.forward(t.prepare_input(u, mode), lens=lens, relu=True, bn=bn, gemm=mode)[:, :, :w].float())
    return torch.cat(ys, 2)


def _random_layer(w, s, d, seed):
    rng = np.random.default_rng(seed)
    layer = ktf.layers.Res2Conv(s, dilation=d, name="res")
    layer.set_weights([rng.standard_normal((s - 1, 3, w, w)) / np.sqrt(3 * w), 0.1 * rng.standard_normal((s - 1, w)), rng.uniform(0.5, 2.0, (s - 1, w)),
                       0.1 * rng.standard_normal((s - 1, w))])
    return layer


def _errors(got, comp, ref, lens, what):
    e_new, e_comp = (max(float(np.abs(a[b, :n] - ref[b]).max()) for b, n in enumerate(lens)) for a in (got, comp))
    top = max(float(np.abs(r).max()) for r in ref)
    print(f"{what}: e_new {e_new:.3e} e_comp {e_comp:.3e} max|ref| {top:.3e}")
    assert e_new <= 2 * e_comp + 2.0 ** -20 * top, what


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("w,s,d", [(64, 8, 3), (128, 4, 2)])
def test_random_inputs_against_the_slice_composition(w, s, d, mode):
    lens = [37, ops.res2_row_tile(w, s, d, MODES[mode]) + 5]
    layer = _random_layer(w, s, d, 9)
    x = np.random.default_rng(10).standard_normal((2, max(lens), s * w)).astype(np.float32)
    kernel, bias, nsc, nsh = layer.get_weights()
    ref = R.batch(x, lens, s, d, kernel, bias=bias, nscale=nsc, nshift=nsh)
    tx, tl = torch.as_tensor(x, device=DEV), torch.as_tensor(np.asarray(lens, np.int32), device=DEV)
    got = layer.forward(tx, tl, mode).cpu().numpy()
    _errors(got, _composition(tx, tl, layer, MODES[mode]).cpu().numpy(), ref, lens, f"w {w} s {s} d {d} {mode}")


FEAT, WIDE, EMB, LENS = 24, 64, 32, (9, 150, 61)
CHAIN = [{"name": "input", "type": "input", "shape": [None, None, FEAT]},
         {"name": "tdnn1", "type": ["tdnn", "relu", "batchnorm"], "cfg": {"units": WIDE, "context": [-2, -1, 0, 1, 2]}},
         {"name": "tdnn2", "type": "tdnn", "cfg": {"units": WIDE, "context": [0]}},
         {"name": "res", "type": "res2_conv", "cfg": {"scale": 4, "dilation": 2}},
         {"name": "tdnn3", "type": "tdnn", "cfg": {"units": WIDE, "context": [0]}},
         {"name": "pool", "type": "stats_pooling", "cfg": {"left_context": 0, "right_context": 10000, "reduce_time_axis": True}},
         {"name": "embed", "type": "tdnn", "cfg": {"units": EMB, "context": [0]}}]


@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16x3", "f16mx"])
def test_layer_in_the_fused_runner_in_every_mode(mode):
    import warnings
    import yaml
    mdl = ktf.models.SequentialFromConfig(yaml.safe_load(yaml.safe_dump({"type": "sequential", "layers": CHAIN})), None, "res2net", gemm=mode)
    mdl.min_tiles, mdl.min_frames = {}, {}               # every batch on the mode's own kernels
    res = mdl.get_layer("res")
    res.set_weights(_random_layer(16, 4, 2, 21).get_weights())
    x = np.random.default_rng(22).standard_normal((len(LENS), max(LENS), FEAT)).astype(np.float32)
    tl = torch.as_tensor(np.asarray(LENS, np.int32), device=DEV)
    seq = lambda layers: ktf.models.Sequential([ktf.models.Input(shape=(None, None))] + layers, gemm=mode)      # noqa: E731
    padded = lambda t: ktf.models._padded_copy(t, torch.float32)      # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = [mdl.run_ragged(padded(torch.as_tensor(x, device=DEV)), tl).float().cpu().numpy().reshape(len(LENS), -1) for _ in range(2)]
        front, back = seq(mdl.layers[:4]), seq(mdl.layers[5:])
        front.min_tiles = front.min_frames = back.min_tiles = back.min_frames = {}
        h = front.run_ragged(padded(torch.as_tensor(x, device=DEV)), tl).float()
        mid = _composition(h.contiguous(), tl, res, res.MODES[mode])
        comp = back.run_ragged(padded(mid), tl).float().cpu().numpy().reshape(len(LENS), -1)
    assert np.array_equal(_bits(got[0]), _bits(got[1]))
    t1, bn1, t2, _, t3, _, t4 = mdl.layers[0], mdl.layers[2], *mdl.layers[3:]
    ref = []
    for b, n in enumerate(LENS):
        f = O.batchnorm(O.relu(O.tdnn(x[b:b + 1, :n], t1.kaldi_matrix(), t1.bias, t1.context, dtype=np.float64)), 1.0, bn1.moving_mean, bn1.moving_variance,
                        bn1.epsilon, dtype=np.float64)
        f = R.conv(O.tdnn(f, t2.kaldi_matrix(), t2.bias, dtype=np.float64)[0], 4, 2, *res.get_weights())
        f = O.stats_pooling(O.tdnn(f[None], t3.kaldi_matrix(), t3.bias, dtype=np.float64), 0, 10000, reduce_time_axis=True, dtype=np.float64)
        ref.append(O.tdnn(f, t4.kaldi_matrix(), t4.bias, dtype=np.float64)[0])
    _errors(got[0][:, None], comp[:, None], ref, [1] * len(LENS), f"runner {mode}")
