"""The squeeze-excitation gate without a GPU: tests/_se_ref.py against fp64 torch.autograd of the plain composition, the C-ABI of
include/ktf_se.h (symbols, every refusal of rule 9 through ops), the layer's weight formats and YAML kind, the residual_from refusals,
and the distance from zero of every hidden pre-activation of the cases tests/test_gpu_se.py runs."""

import contextlib
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
import _se_ref as R  # noqa: E402


@pytest.mark.parametrize("C,H,lens,bias", [(8, 3, [5, 0, 70], True), (20, 17, [129, 1], False)])
def test_reference_is_fp64_autograd_of_the_plain_composition(C, H, lens, bias):
    c = R.case(C, H, lens, max(lens), 7, bias)
    t = {k: torch.tensor(np.asarray(c[k], np.float64), requires_grad=True) for k in ("w1", "w2", "b1", "b2") if c[k] is not None}
    fs, bs, loss = [], [], 0.0
    for b, n in enumerate(lens):
        x, r, g = (c[k][b, :n] for k in ("x", "r", "g"))
        fs.append(R.forward(x, r, c["w1"], c["b1"], c["w2"], c["b2"], round_gate=False))
        bs.append(R.backward(g, x, c["w1"], c["w2"], fs[-1]))
        if n == 0:
            continue
        xt = torch.tensor(x.astype(np.float64), requires_grad=True)
        h = torch.relu(xt.mean(0) @ t["w1"] + (t["b1"] if bias else 0.0))
        s = torch.sigmoid(h @ t["w2"] + (t["b2"] if bias else 0.0))
        y = xt * s + torch.tensor(r.astype(np.float64))
        part = (y * torch.tensor(g.astype(np.float64))).sum()
        (dx,) = torch.autograd.grad(part, xt, retain_graph=True)
        loss = loss + part
        for name, got, want in (("mean", fs[-1]["mean"], xt.mean(0)), ("hid", fs[-1]["hid"], h), ("gate", fs[-1]["gate"], s), ("y", fs[-1]["y"], y),
                                ("dx", bs[-1]["dx"], dx)):
            assert np.abs(got - want.detach().numpy()).max() <= 1e-12, (name, b)
        # the rounded gate the GPU is compared with is this one rounded once, and nothing else changes
        f32 = R.forward(x, r, c["w1"], c["b1"], c["w2"], c["b2"])
        assert f32["gate"].dtype == np.float32 and np.array_equal(f32["gate"], fs[-1]["gate"].astype(np.float32))
        assert np.array_equal(f32["y"], x.astype(np.float64) * f32["gate"].astype(np.float64) + r.astype(np.float64))
    loss.backward()
    for k, (v, _) in R.param_grads(fs, bs).items():
        if k[1:] in t:
            assert np.abs(v - t[k[1:]].grad.numpy()).max() <= 1e-12, k


def test_header_symbols_are_the_se_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_se.h")).read()
    code = hdr[hdr.index("#ifndef KTF_SE_H_"):]
    protos = re.findall(r"^(?:int|int64_t) (ktf_[a-z0-9_]+)\(([^;]*)\);", code, flags=re.M)
    assert {n for n, _ in protos} == set(L.SE_PROTOTYPES) == {"ktf_se_gate", "ktf_se_gate_train", "ktf_se_gate_backward",
                                                             "ktf_se_gate_backward_workspace_bytes"}
    ctype = {"const float*": L._P, "float*": L._P, "const double*": L._P, "double*": L._P, "const int32_t*": L._P, "void*": L._P,
             "int64_t": L._i64, "int32_t": L._i32, "size_t": __import__("ctypes").c_size_t}
    for name, args in protos:
        assert L.SE_PROTOTYPES[name][1] == [ctype[" ".join(a.split()[:-1])] for a in args.replace("\n", " ").split(",")], name
    lib = L.load()
    assert all(hasattr(lib, n) for n in L.SE_PROTOTYPES) and len(L.PROTOTYPES) == 120 and lib.ktf_version() == 117
    assert ops.se_gate_floats(3, 20) == 64 + 120 and ops._size("ktf_se_gate_backward_workspace_bytes", 0, 8, 3) == 3 * 256 + 256


def _aligned(n, off=0):
    """n zero floats on the host whose base is `off` floats behind a 256-byte boundary."""
    buf = torch.zeros(n + 128)
    k = (-buf.data_ptr() // 4) % 64
    return buf[k + off:k + off + n]


def test_every_refusal_of_rule_9_through_ops(monkeypatch):
    monkeypatch.setattr(L, "stream_ptr", lambda: None)       # host pointers and a null stream: every refusal comes before any launch
    monkeypatch.setattr(L, "on_device", lambda device: contextlib.nullcontext())
    B, T, C_, H = 2, 5, 8, 3
    rows = lambda C=C_: _aligned(B * T * C).view(B, T, C)      # noqa: E731

    def fwd(x=None, r=None, y=None, C=C_, H=H, w1="w", gate=None, C_arg=None):
        w1 = torch.zeros(C, H) if isinstance(w1, str) else w1
        return ops.se_gate(rows(C) if x is None else x, r, None, w1, None, torch.zeros(H, C), None, rows(C) if y is None else y,
                           _aligned(ops.se_gate_floats(B, C)) if gate is None else gate, C=C_arg)

    def bwd(g=None, x=None, dx=None, gate=None, ws=None, H=H):
        ws = _aligned(ops._size("ktf_se_gate_backward_workspace_bytes", B, C_, H) // 4).view(torch.uint8) if ws is None else ws
        return ops.se_gate_backward(rows() if g is None else g, rows() if x is None else x, None, torch.zeros(C_, H), torch.zeros(H, C_),
                                    torch.zeros(B, C_, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64),
                                    _aligned(B * C_).view(B, C_) if gate is None else gate, rows() if dx is None else dx, None, None, None, None, ws)

    wide = _aligned(B * T * (C_ + 2)).view(B, T, C_ + 2)
    big = _aligned(2 * B * T * C_)
    xo, yo = big[:B * T * C_].view(B, T, C_), big[C_:C_ + B * T * C_].view(B, T, C_)
    for call, what in ((lambda: fwd(C=2), "multiple of 4"), (lambda: fwd(C=6), "multiple of 4"), (lambda: fwd(C=4100), "multiple of 4"),
                       (lambda: fwd(H=0), "H 0"), (lambda: fwd(H=1025), "H 1025"), (lambda: fwd(w1=None), "w1"),
                       (lambda: fwd(x=rows(4), C_arg=C_, w1=torch.zeros(C_, H)), "ldx"), (lambda: fwd(y=rows(4), C_arg=C_), "ldy|B, T"),
                       (lambda: fwd(x=wide[:, :, :C_], C_arg=C_), "ldx"), (lambda: fwd(r=wide[:, :, :C_], C_arg=C_), "ldr"),
                       (lambda: fwd(gate=_aligned(ops.se_gate_floats(B, C_) - 1)), "workspace"),
                       (lambda: fwd(gate=_aligned(ops.se_gate_floats(B, C_), 4)), "256-byte"),
                       (lambda: fwd(x=xo, y=yo), "y overlaps x"), (lambda: fwd(r=xo, y=yo), "y overlaps r"),
                       (lambda: bwd(g=xo, dx=yo), "dx overlaps"), (lambda: bwd(x=xo, dx=yo), "dx overlaps"),
                       (lambda: bwd(gate=big[:B * C_].view(B, C_), dx=big[4:4 + B * T * C_].view(B, T, C_)), "dx overlaps"),
                       (lambda: bwd(ws=_aligned(64).view(torch.uint8)), "workspace"),
                       (lambda: bwd(ws=_aligned(4096, 4).view(torch.uint8)), "256-byte")):
        with pytest.raises(ValueError, match=what):
            call()
    lib, P = L.load(), __import__("ctypes").c_void_p(256)
    for B_, T_, ld in ((-1, 5, C_), (2, -5, C_), (65536, 5, C_), (2, (1 << 30) + 1, C_), (2, 5, 1 << 31)):
        assert lib.ktf_se_gate(P, B_, T_, C_, ld, None, 0, None, P, None, P, None, H, P, ld, P, None) == -1
    assert lib.ktf_se_gate(None, 2, 5, C_, C_, None, 0, None, P, None, P, None, H, P, C_, P, None) == -1      # a null x
    assert lib.ktf_se_gate(None, 0, 5, C_, C_, None, 0, None, None, None, None, None, H, None, C_, None, None) == 0      # B = 0: nothing to do
    for bad in ((1, 6, 3), (1, 8, 0), (65536, 8, 3)):
        with pytest.raises(ValueError):
            ops.se_gate_backward_workspace(*bad, device="cpu")


def test_layer_weight_formats_config_yaml_kind_and_residual_refusals():
    C_, H = 16, 4
    fc1, fc2 = torch.nn.Conv1d(C_, H, 1), torch.nn.Linear(H, C_)
    layer = ktf.layers.SqueezeExcite(H, residual_from="first", name="se")
    epoch = ktf.layers.WEIGHTS_EPOCH[0]
    layer.set_weights([fc1.weight, fc1.bias, fc2.weight, fc2.bias], fmt="torch")
    w1, b1, w2, b2 = layer.get_weights()
    assert layer._version == 1 and ktf.layers.WEIGHTS_EPOCH[0] == epoch + 1 and layer.inputDim == C_
    assert w1.shape == (C_, H) and w2.shape == (H, C_) and w1[5, 2] == fc1.weight[2, 5, 0].item() and w2[3, 7] == fc2.weight[7, 3].item()
    twin = ktf.layers.SqueezeExcite.from_config(layer.get_config())
    twin.set_weights(layer.get_weights())
    assert twin.get_config() == layer.get_config() and all(np.array_equal(a, b) for a, b in zip(twin.get_weights(), layer.get_weights()))
    for bad in (lambda: ktf.layers.SqueezeExcite(0), lambda: ktf.layers.SqueezeExcite(1025), lambda: ktf.layers.SqueezeExcite(4).build((None, None, 6)),
                lambda: layer.set_weights([w1, b1, w2], fmt="tensorflow"), lambda: layer.set_weights([w2, b1, w1, b2], fmt="tensorflow")):
        with pytest.raises(ValueError):
            bad()
    (built,) = ktf.models.cfg2layers({"name": "gate", "type": "squeeze_excite", "cfg": {"bottleneck": 8, "residual_from": "first.affine"}})
    assert isinstance(built, ktf.layers.SqueezeExcite) and (built.name, built.bottleneck, built.residualFrom) == ("gate", 8, "first.affine")

    pool = lambda: ktf.layers.StatsPooling(0, 10000, reduce_time_axis=True)      # noqa: E731
    seq = lambda *ls: ktf.models.Sequential([ktf.models.Input(shape=(None, 32))] + list(ls))      # noqa: E731
    tdnn = lambda name, units=32, **kw: ktf.layers.TDNN(units, name=name, **kw)      # noqa: E731
    se = lambda src: ktf.layers.SqueezeExcite(8, residual_from=src, name="se")      # noqa: E731
    mdl = seq(tdnn("first"), tdnn("a"), ktf.layers.Res2Conv(2, name="res"), tdnn("b"), se("first"), pool(), ktf.layers.TDNN(8))
    plan = mdl._plan()
    assert [st[0] for st in plan] == ["tdnn", "tdnn", "res2", "tdnn", "se", "stats", "tdnn"] and plan[4][2] == 0
    assert (id(mdl.layers[4]), mdl.layers[4]._version) in mdl.weights_signature()
    assert [st[0] for st in seq(tdnn("first"), pool(), ktf.layers.TDNN(8))._plan()] == ["tdnn", "stats", "tdnn"]      # (as before)
    assert seq(tdnn("first"), pool(), se(None))._plan() is None
    assert seq(tdnn("first"), tdnn("a", padding="VALID"), se("first"), pool())._plan()[2][2] == 0      # (a VALID 1x1 layer keeps the lengths)
    for bad in (seq(tdnn("first"), se("nobody"), pool()), seq(tdnn("first"), se("later"), tdnn("later"), pool()),
                seq(tdnn("first"), se("tail"), pool(), ktf.layers.TDNN(8, name="tail")), seq(tdnn("first", 64), tdnn("a"), se("first"), pool()),
                seq(tdnn("first"), tdnn("a", context=[-1, 0, 1], padding="VALID"), se("first"), pool()),
                seq(tdnn("first"), tdnn("a", subsampling_factor=2), se("first"), pool()),
                seq(tdnn("first"), ktf.layers.ReLU(name="r"), se("first"), pool())):
        with pytest.raises(ValueError, match="residual|width|lengths"):
            bad._plan()


@pytest.mark.parametrize("i", range(len(R.GRID)))
def test_hidden_pre_activations_of_the_gpu_cases_lie_away_from_zero(i):
    c, _ = R.grid_case(i)
    for b, n in enumerate(c["lens"]):
        if n:
            f = R.forward(c["x"][b, :n], None, c["w1"], c["b1"], c["w2"], c["b2"])
            assert (np.abs(f["a"]) >= 2.0 ** -20 * f["a_abs"]).all(), (i, b)
