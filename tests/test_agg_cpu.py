"""Multi-layer feature aggregation without a GPU: tests/_agg_ref.py against torch's conv1d on torch.cat in fp64, the C-ABI of
include/ktf_agg.h (symbols, every refusal of rule 7 through ops), the layer's weight formats, its YAML kind and the plan-time refusals,
the exactness of the inputs that tests/test_gpu_agg.py compares bit for bit, and the margin of its training model's ReLU inputs."""

import contextlib
import ctypes as C
import os
import re
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
import _agg_ref as R  # noqa: E402


@pytest.mark.parametrize("widths,units,n,relu", [((32, 64), 17, 9, True), ((64, 32, 32), 5, 1, False), ((32, 32, 32, 32), 40, 3, True)])
def test_reference_is_torch_conv1d_on_the_concatenation(widths, units, n, relu):
    rng = np.random.default_rng(units)
    xs, w = [rng.standard_normal((n, c)) for c in widths], rng.standard_normal((units, sum(widths)))
    bias, nsc, nsh = (rng.standard_normal(units) for _ in range(3))
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)      # noqa: E731
    z = torch.nn.functional.conv1d(torch.cat([t(x) for x in xs], 1).T[None], t(w)[:, :, None], t(bias))[0].T
    want = (z.clamp(min=0) if relu else z) * t(nsc) + t(nsh)
    assert np.abs(R.conv(xs, w, bias, nsc, nsh, relu=relu) - want.numpy()).max() <= 1e-12


def test_header_symbols_are_the_agg_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_agg.h")).read()
    code = hdr[hdr.index("#ifndef KTF_AGG_H_"):]
    protos = re.findall(r"^(?:int|int32_t) (ktf_[a-z0-9_]+)\(([^;]*)\);", code, flags=re.M)
    assert {n for n, _ in protos} == set(L.AGG_PROTOTYPES) == {"ktf_agg_conv", "ktf_agg_row_tile"}
    ctype = {"const float* const*": L._P, "const float*": L._P, "float*": L._P, "const int32_t*": L._P, "const int64_t*": L._P, "void*": L._P,
             "int64_t": L._i64, "int32_t": L._i32}
    for name, args in protos:
        assert L.AGG_PROTOTYPES[name][1] == [ctype[" ".join(a.split()[:-1])] for a in args.replace("\n", " ").split(",")], name
    assert L.AGG_PROTOTYPES["ktf_agg_conv"][0] is C.c_int and L.AGG_PROTOTYPES["ktf_agg_row_tile"][0] is L._i32
    lib = L.load()
    assert all(hasattr(lib, n) for n in L.AGG_PROTOTYPES) and not set(L.AGG_PROTOTYPES) & (set(L.PROTOTYPES) | set(L.RES2_PROTOTYPES) | set(L.SE_PROTOTYPES))
    assert (L.AGG_MAX_SOURCES, L.AGG_MAX_WIDTH, L.AGG_MAX_UNITS) == tuple(int(re.search(rf"#define KTF_AGG_MAX_{n} (\d+)", hdr).group(1))
                                                                          for n in ("SOURCES", "WIDTH", "UNITS"))
    assert len(L.PROTOTYPES) == 120 and lib.ktf_version() == 117          # (the families that were there stay as they are)


def test_every_refusal_of_rule_7_through_ops(monkeypatch):
    monkeypatch.setattr(L, "stream_ptr", lambda: None)       # host pointers and a null stream: every refusal comes before any launch
    monkeypatch.setattr(L, "on_device", lambda device: contextlib.nullcontext())
    B, T, U = 2, 5, 8
    z = lambda *s: torch.zeros(*s)      # noqa: E731

    def call(widths=(32, 64), lds=None, units=U, ldw=None, ldy=None, w="w", nscale="n", nshift="n", act=L.ACT_RELU, gemm=L.GEMM_F32, y=None):
        K = sum(widths)
        xs = [z(B, T, ld)[:, :, :c] for c, ld in zip(widths, lds or widths)]
        par = lambda v: z(units) if isinstance(v, str) else v      # noqa: E731
        y = z(B, T, ldy or units)[:, :, :units] if y is None else y
        return ops.agg_conv(xs, None, z(units, ldw or K)[:, :K] if isinstance(w, str) else w, par("b"), par(nscale), par(nshift), act, gemm, y)

    for kw, what in ((dict(widths=(32,)), "sources"), (dict(widths=(32,) * 5), "sources"), (dict(widths=(32, 48)), "multiple of 32"),
                     (dict(widths=(32, 4128)), "multiple of 32"), (dict(units=8193), "units"), (dict(lds=(32, 66)), "ldx"), (dict(ldw=98), "ldw"),
                     (dict(ldy=10), "ldy"), (dict(nscale=None), "go together"), (dict(nshift=None), "go together"), (dict(act=L.ACT_TANH), "act"),
                     (dict(act=-1), "act"), (dict(gemm=L.GEMM_F16MX), "gemm"), (dict(gemm=L.GEMM_BF16X4), "gemm"), (dict(gemm=7), "gemm"), (dict(w=None), "null")):
        with pytest.raises(ValueError, match=what):
            call(**kw)
    flat = z(2 * B * T * 64)
    with pytest.raises(ValueError, match="overlaps source 1"):
        ops.agg_conv([z(B, T, 32), flat[:B * T * 64].view(B, T, 64)], None, z(U, 96), None, None, None, 0, 0, flat[64:64 + B * T * U].view(B, T, U))
    lib, P = L.load(), C.c_void_p(8)
    tab = lambda ld: ((C.c_void_p * 2)(8, 8), (C.c_int32 * 2)(32, 32), (C.c_int64 * 2)(ld, ld))      # noqa: E731
    for B_, T_, ld, units in ((-1, 5, 32, U), (2, -5, 32, U), (65536, 5, 32, U), (2, (1 << 30) + 1, 32, U), (2, 5, 1 << 31, U), (2, 5, 32, 0), (2, 5, 30, U)):
        assert lib.ktf_agg_conv(*tab(ld), 2, B_, T_, None, P, 64, None, None, None, units, 0, 0, P, 8192, None) == -1
    assert lib.ktf_agg_conv((C.c_void_p * 2)(8, None), (C.c_int32 * 2)(32, 32), (C.c_int64 * 2)(32, 32), 2, 2, 5, None, P, 64, None, None, None, U, 0, 0, P, U, None) == -1
    assert lib.ktf_agg_conv(*tab(32), 2, 0, 5, None, None, 64, None, None, None, U, 0, 0, None, U, None) == 0      # (B T = 0: nothing is launched)
    assert ops.agg_row_tile(1, 64) == ops.agg_row_tile(8192, 16384, L.GEMM_BF16X3) == 128
    for bad in ((0, 64, 0), (8193, 64, 0), (8, 32, 0), (8, 80, 0), (8, 16416, 0), (8, 64, 5)):
        with pytest.raises(ValueError):
            ops.agg_row_tile(*bad)


def _chain(sources, units=48, front=(), between=()):
    tdnn = lambda n, u, **kw: {"name": n, "type": "tdnn", "cfg": dict(units=u, **kw)}      # noqa: E731
    return {"layers": [{"type": "input", "shape": [None, None, 24]}, {"name": "t1", "type": ["tdnn", "relu", "bn"], "cfg": {"units": 32, "context": [-2, -1, 0, 1, 2]}},
                       tdnn("t2", 64), *between, tdnn("t3", 32), *front, {"name": "mfa", "type": ["aggregate", "relu", "bn"], "cfg": {"units": units, "sources": sources}},
                       {"name": "pool", "type": "stats_pooling", "cfg": {"left_context": 0, "right_context": 10000, "reduce_time_axis": True}}, tdnn("emb", 16)]}


def test_layer_weight_formats_config_yaml_kind_and_plan():
    conv, rng = torch.nn.Conv1d(128, 48, 1), np.random.default_rng(3)
    nsc, nsh = ktf.layers.Aggregate.fold_batch_norm(rng.standard_normal(48), rng.uniform(0.5, 2, 48), rng.uniform(0.5, 2, 48), rng.standard_normal(48), 1e-5)
    assert ktf.layers.Aggregate.fold_batch_norm is ktf.layers.Res2Conv.fold_batch_norm
    layer = ktf.layers.Aggregate(48, ["a", "b"], batch_norm=True, name="mfa")
    epoch = ktf.layers.WEIGHTS_EPOCH[0]
    layer.set_weights([conv.weight, conv.bias, nsc, nsh], fmt="torch")
    assert layer._version == 1 and ktf.layers.WEIGHTS_EPOCH[0] == epoch + 1 and layer.inputDim == 128 and not layer.built
    kernel = layer.get_weights()[0]
    assert kernel.shape == (128, 48) and kernel[5, 7] == conv.weight[7, 5, 0].item()
    layer.set_weights([conv.weight[:, :, 0]] + layer.get_weights()[1:], fmt="torch")
    assert np.array_equal(layer.get_weights()[0], kernel)
    layer.build((2, 7, 32), [(2, 7, 32), (2, 7, 64)])
    assert layer.built and layer.widths == [32, 64, 32] and layer.compute_output_shape((2, 7, 32)) == (2, 7, 48)
    twin = ktf.layers.Aggregate.from_config(layer.get_config())
    twin.set_weights(layer.get_weights())
    assert twin.get_config() == layer.get_config() and all(np.array_equal(a, b) for a, b in zip(twin.get_weights(), layer.get_weights()))
    for bad in (dict(units=0, sources=["a"]), dict(units=8, sources=[]), dict(units=8, sources=list("abcd")), dict(units=8, sources="a"),
                dict(units=8, sources=["a"], activation="tanh")):
        with pytest.raises(ValueError):
            ktf.layers.Aggregate(**bad)
    with pytest.raises(ValueError, match="multiple of 32"):
        ktf.layers.Aggregate(8, ["a"]).build((2, 7, 48), [(2, 7, 32)])
    mdl = ktf.models.SequentialFromConfig(_chain(["t1.batchnorm", "t2.affine"]))
    mfa = mdl.get_layer("mfa")
    plan = mdl._plan()
    assert [st[0] for st in plan] == ["tdnn", "tdnn", "tdnn", "agg", "stats", "tdnn"] and plan[3][2] is True and plan[3][3] is mdl.layers[-3] and plan[3][4] == [0, 1]
    assert mfa.widths == [32, 64, 32] and (id(mfa), mfa._version) in mdl.weights_signature()
    bare = ktf.models.SequentialFromConfig({"layers": [e for e in _chain(["t2.affine"])["layers"] if e.get("name") != "mfa"]})
    assert [st[:1] + st[2:] for st in bare._plan()] == [("tdnn", True, bare.layers[2]), ("tdnn", False, None), ("tdnn", False, None), ("stats",), ("tdnn", False, None)]


@pytest.mark.parametrize("kw,what", [(dict(sources=["nope"]), "nope"), (dict(sources=["emb.affine"]), "emb.affine"), (dict(sources=["t1.affine"]), "t1.affine"),
                                     (dict(sources=["t1.batchnorm", "t2.affine", "t3.affine", "t2.affine"]), "one to 3"), (dict(sources=["t3.affine"]), "own input"),
                                     (dict(sources=["t2.affine"], between=[{"name": "cut", "type": "tdnn", "cfg": {"units": 64, "context": [-1, 0, 1], "padding": "VALID"}}]), "lengths"),
                                     (dict(sources=["t2.affine"], front=[{"name": "odd", "type": "tdnn", "cfg": {"units": 40}}]), "multiple of 32"),
                                     (dict(sources=["t2.affine"], front=[{"name": "p0", "type": "stats_pooling", "cfg": {"left_context": 0, "right_context": 9, "reduce_time_axis": True}}]), "pooling")])
def test_plan_time_refusals_name_the_layer(kw, what):
    with pytest.raises(ValueError, match=f"(?s)mfa.*{what}"):
        ktf.models.SequentialFromConfig(_chain(**kw))._plan()


@pytest.mark.parametrize("widths,units", R.EXACT_SHAPES)
def test_inputs_of_the_bitwise_gpu_test_are_exact_in_fp32(widths, units):
    lens = R.exact_lens(ops.agg_row_tile(units, sum(widths)))
    c = R.exact_case(widths, units, lens)
    assert all(np.abs(x).max() <= 8 and (x == np.rint(x)).all() for x in c["xs"]) and set(np.unique(c["w"])) <= {-1, 0, 1}
    off = 0
    for C_ in widths:
        assert ((c["w"][:, off:off + C_] != 0).sum(1) == 4).all()
        off += C_
    x = np.abs(np.concatenate(c["xs"], 2)).astype(np.float64)
    assert (x @ np.abs(c["w"]).T.astype(np.float64) + np.abs(c["bias"])).max() < 2.0 ** 24      # every partial sum: an integer below 2^24
    for y in R.batch(c["xs"], lens, c["w"], bias=c["bias"], nscale=c["nscale"], nshift=c["nshift"], relu=True):
        assert (y * 4 == np.rint(y * 4)).all() and np.array_equal(y.astype(np.float32).astype(np.float64), y)


def test_relu_inputs_of_the_training_model_stay_away_from_zero():
    mdl, feats = R.train_model(ktf)
    pre = []
    R.restated(mdl, [torch.as_tensor(p, dtype=torch.float64) for p in R.train_params(mdl)], torch.as_tensor(feats, dtype=torch.float64), R.TRAIN["lens"], pre)
    assert len(pre) == 3 and min(float(p.abs().min()) for p in pre) > 1e-4
