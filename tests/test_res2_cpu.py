"""The Res2Net dilated convolution without a GPU: tests/_res2_ref.py against torch's conv1d in fp64, the C-ABI of include/ktf_res2.h
(symbols, every refusal of rule 6 through ops), the layer's weight formats and its YAML kind, and the exactness of the inputs that
tests/test_gpu_res2.py compares bit for bit."""

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
import _res2_ref as R  # noqa: E402

CASES = [(16, 2, 1), (16, 3, 8), (64, 8, 2), (64, 8, 4), (128, 4, 3), (128, 8, 4)]      # (w, s, d) of the GPU test


@pytest.mark.parametrize("w,s,d,n,relu", [(16, 3, 2, 9, True), (32, 4, 3, 2, False), (16, 8, 8, 40, True), (48, 2, 1, 1, True)])
def test_reference_is_torch_conv1d_on_replicate_padded_slices(w, s, d, n, relu):
    rng = np.random.default_rng(w + s + d)
    x, W = rng.standard_normal((n, s * w)), rng.standard_normal((s - 1, 3, w, w)) / np.sqrt(3 * w)
    bias, nsc, nsh = (rng.standard_normal((s - 1, w)) for _ in range(3))
    t = lambda a: torch.as_tensor(a, dtype=torch.float64)      # noqa: E731
    ys = [t(x[:, :w])]
    for i in range(1, s):
        u = t(x[:, i * w:(i + 1) * w]) + (ys[-1] if i >= 2 else 0.0)
        padded = torch.nn.functional.pad(u.T[None], (d, d), mode="replicate")
        z = torch.nn.functional.conv1d(padded, t(W[i - 1]).permute(2, 1, 0), t(bias[i - 1]), dilation=d)[0].T      # weight (out, in, k)
        ys.append((z.clamp(min=0) if relu else z) * t(nsc[i - 1]) + t(nsh[i - 1]))
    got = R.conv(x, s, d, W, bias, nsc, nsh, relu=relu)
    assert np.abs(got - torch.cat(ys, 1).numpy()).max() <= 1e-12


def test_header_symbols_are_the_res2_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_res2.h")).read()
    code = hdr[hdr.index("#ifndef KTF_RES2_H_"):]
    protos = re.findall(r"^(?:int|int32_t) (ktf_[a-z0-9_]+)\(([^;]*)\);", code, flags=re.M)
    assert {n for n, _ in protos} == set(L.RES2_PROTOTYPES) == set(re.findall(r"\b(ktf_[a-z0-9_]+)\s*\(", code))
    ctype = {"const float*": L._P, "float*": L._P, "const int32_t*": L._P, "void*": L._P, "int64_t": L._i64, "int32_t": L._i32}
    for name, args in protos:
        assert L.RES2_PROTOTYPES[name][1] == [ctype[" ".join(a.split()[:-1])] for a in args.replace("\n", " ").split(",")], name
    assert L.RES2_PROTOTYPES["ktf_res2_conv"][0] is C.c_int and L.RES2_PROTOTYPES["ktf_res2_row_tile"][0] is L._i32
    lib = L.load()
    assert all(n.startswith("ktf_res2_") and hasattr(lib, n) for n in L.RES2_PROTOTYPES)
    families = [L.PROTOTYPES, L.AUGMENT_PROTOTYPES, L.RESAMPLE_PROTOTYPES, L.GRAD_PROTOTYPES, L.NORM_PROTOTYPES, L.LOSS_PROTOTYPES,
                L.EGS_PROTOTYPES, L.OPTIM_PROTOTYPES, L.HEAD_PROTOTYPES, L.ATTN_PROTOTYPES, L.DENSE_PROTOTYPES]
    assert not set(L.RES2_PROTOTYPES) & set().union(*families)
    assert all("ktf_res2_" not in open(os.path.join(ROOT, "include", o)).read() for o in os.listdir(os.path.join(ROOT, "include")) if o != "ktf_res2.h")
    assert (L.RES2_MAX_BATCH, L.RES2_MAX_ROWS) == tuple(int(re.search(rf"#define KTF_RES2_MAX_{n} (\d+)", hdr).group(1)) for n in ("BATCH", "ROWS"))
    assert len(L.PROTOTYPES) == 120 and lib.ktf_version() == 117          # (the families that were there stay as they are)


def test_every_refusal_of_rule_6_through_ops(monkeypatch):
    monkeypatch.setattr(L, "stream_ptr", lambda: None)       # host pointers and a null stream: every refusal comes before any launch
    monkeypatch.setattr(L, "on_device", lambda device: contextlib.nullcontext())
    s, w, B, T = 4, 16, 2, 5
    C_ = s * w

    def call(x=None, y=None, lens=None, scale=s, d=1, W="w", nscale="n", nshift="n", act=L.ACT_RELU, gemm=L.GEMM_F32, C=C_, wd=w):
        g = max(scale - 1, 1)
        x = torch.zeros(B, T, C_) if x is None else x
        y = torch.zeros(B, T, C_) if y is None else y
        par = lambda v: torch.zeros(g, wd) if isinstance(v, str) else v      # noqa: E731
        return ops.res2_conv(x, lens, scale, d, torch.zeros(g, 3 * wd, wd) if isinstance(W, str) else W, par("b"), par(nscale), par(nshift),
                             act, gemm, y, C=C)

    for kw, what in ((dict(scale=1), "scale"), (dict(scale=9), "scale"), (dict(scale=3, C=64, wd=21), "C % scale"),
                     (dict(scale=4, C=32, wd=8), "width"), (dict(scale=2, C=288, wd=144, x=torch.zeros(B, T, 288), y=torch.zeros(B, T, 288)), "width"),
                     (dict(scale=2, C=48, wd=24), "width"), (dict(d=0), "dilation"), (dict(d=9), "dilation"),
                     (dict(x=torch.zeros(B, T, C_ - 4)), "below C"), (dict(y=torch.zeros(B, T, C_ - 4)), "below C"),
                     (dict(x=torch.zeros(B, T, C_ + 2)[:, :, :C_]), "multiples of 4"), (dict(y=torch.zeros(B, T, C_ + 2)[:, :, :C_]), "multiples of 4"),
                     (dict(nscale=None), "go together"), (dict(nshift=None), "go together"), (dict(act=L.ACT_TANH), "act"), (dict(act=-1), "act"),
                     (dict(gemm=L.GEMM_F16MX), "gemm"), (dict(gemm=L.GEMM_BF16X4), "gemm"), (dict(gemm=7), "gemm"), (dict(W=None), "null")):
        with pytest.raises(ValueError, match=what):
            call(**kw)
    xy = torch.zeros(2 * B * T * C_)
    with pytest.raises(ValueError, match="overlaps"):
        call(x=xy[:B * T * C_].view(B, T, C_), y=xy[C_:C_ + B * T * C_].view(B, T, C_))
    lib, P = L.load(), C.c_void_p(8)
    for B_, T_, ld in ((-1, 5, C_), (2, -5, C_), (65536, 5, C_), (2, (1 << 30) + 1, C_), (2, 5, 1 << 31)):
        assert lib.ktf_res2_conv(P, B_, T_, C_, ld, None, s, 1, P, None, None, None, 0, 0, P, ld, None) == -1
    assert ops.res2_row_tile(64, 8, 4) == 128 and ops.res2_row_tile(128, 8, 4, L.GEMM_BF16X3) == 96 and ops.res2_row_tile(128, 8, 8) == 32
    for bad in ((8, 4, 1, 0), (144, 4, 1, 0), (64, 1, 1, 0), (64, 9, 1, 0), (64, 4, 0, 0), (64, 4, 9, 0), (64, 4, 1, 5)):
        with pytest.raises(ValueError):
            ops.res2_row_tile(*bad)


def test_layer_weight_formats_config_and_yaml_kind():
    s, w = 4, 16
    rng = np.random.default_rng(3)
    conv = [torch.nn.Conv1d(w, w, 3, dilation=2, padding=2) for _ in range(s - 1)]
    nsc, nsh = ktf.layers.Res2Conv.fold_batch_norm(rng.standard_normal((s - 1, w)), rng.uniform(0.5, 2, (s - 1, w)), rng.uniform(0.5, 2, (s - 1, w)),
                                                   rng.standard_normal((s - 1, w)), 1e-5)
    layer = ktf.layers.Res2Conv(s, dilation=2, name="block")
    epoch = ktf.layers.WEIGHTS_EPOCH[0]
    layer.set_weights([torch.stack([c.weight for c in conv]), torch.stack([c.bias for c in conv]), nsc, nsh], fmt="torch")
    assert layer._version == 1 and ktf.layers.WEIGHTS_EPOCH[0] == epoch + 1 and layer.inputDim == s * w
    kernel, bias, gs, gh = layer.get_weights()
    assert kernel.shape == (s - 1, 3, w, w) and kernel[1, 2, 5, 7] == conv[1].weight[7, 5, 2].item() and bias[2, 3] == conv[2].bias[3].item()
    u = rng.standard_normal((11, s * w))
    want = torch.nn.functional.conv1d(torch.as_tensor(u[:, w:2 * w].T[None], dtype=torch.float32), conv[0].weight, conv[0].bias, dilation=2, padding=2)
    got = R.conv(u, s, 2, kernel, bias, relu=False)[2:-2, w:2 * w]          # (interior rows: Conv1d pads with zeros, the layer replicates)
    assert np.abs(got - want[0].T[2:-2].detach().numpy()).max() < 1e-5
    twin = ktf.layers.Res2Conv.from_config(layer.get_config())
    twin.set_weights(layer.get_weights())
    assert twin.get_config() == layer.get_config() and all(np.array_equal(a, b) for a, b in zip(twin.get_weights(), layer.get_weights()))
    assert twin.compute_output_shape((2, 7, s * w)) == (2, 7, s * w)
    for bad in (dict(scale=1), dict(scale=4, dilation=9), dict(scale=4, activation="tanh")):
        with pytest.raises(ValueError):
            ktf.layers.Res2Conv(**bad)
    for C_ in (66, 4 * 8, 4 * 144):
        with pytest.raises(ValueError, match="scale|width"):
            ktf.layers.Res2Conv(4).build((None, None, C_))
    (built,) = ktf.models.cfg2layers({"name": "res", "type": "res2_conv", "cfg": {"scale": 4, "dilation": 3, "batch_norm": False}})
    assert isinstance(built, ktf.layers.Res2Conv) and (built.name, built.scale, built.dilation, built.batchNorm) == ("res", 4, 3, False)
    mdl = ktf.models.Sequential([ktf.models.Input(shape=(None, 64)), built, ktf.layers.StatsPooling(0, 10000, reduce_time_axis=True), ktf.layers.TDNN(8)])
    assert [st[0] for st in mdl._plan()] == ["res2", "stats", "tdnn"] and (id(built), built._version) in mdl.weights_signature()
    assert ktf.models.Sequential([ktf.models.Input(shape=(None, 64)), ktf.layers.StatsPooling(0, 10000, reduce_time_axis=True), ktf.layers.Res2Conv(4)])._plan() is None


@pytest.mark.parametrize("w,s,d", CASES)
def test_inputs_of_the_bitwise_gpu_test_are_exact_in_fp32(w, s, d):
    lens = R.exact_lens(s, d, ops.res2_row_tile(w, s, d))
    c = R.exact_case(w, s, d, lens)
    assert np.abs(c["x"]).max() <= 8 and (c["x"] == np.rint(c["x"])).all() and ((c["W"] != 0).sum(axis=(1, 2)) == 4).all() and set(np.unique(c["W"])) <= {-1, 0, 1}
    for b, n in enumerate(lens):
        trace = []
        if n:
            R.conv(c["x"][b, :n], s, d, c["W"], c["bias"], c["nscale"], c["nshift"], trace=trace)
        for st in trace:
            for k, v in st.items():
                assert (v * 2.0 ** 14 == np.rint(v * 2.0 ** 14)).all() and np.abs(v).max() < 2.0 ** 10, (b, k)
