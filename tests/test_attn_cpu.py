"""Attentive statistics pooling without a GPU: the fp64 restatement (tests/_attn_ref.py) against fp64 torch.autograd of a plain
softmax composition and against tests/_pool_ref.py, the C-ABI of include/ktf_attn.h (symbols, argument types, every refusal of
rule 13 through ops), what the bounds assume of every input test_gpu_attn.py uses, and the host side of
ktf.layers.AttentiveStatsPooling, cfg2layers, ktf.autograd.attentive_stats_pooling and TrainableSequential / export()."""

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
import _attn_ref as R  # noqa: E402
import _pool_ref as P  # noqa: E402

F64 = torch.float64


# ----------------------------------------------------------------------------- the restatement
def torch_pool(x, e, n, include_std=True, eps=1e-10):
    """One utterance in torch ops, for autograd: x (T, D), e (T, H) fp64 -> (D or 2 D)."""
    D, H = x.shape[1], e.shape[1]
    w = torch.softmax(e[:n], dim=0).repeat_interleave(D // H, dim=1)
    mu = (w * x[:n]).sum(0)
    if not include_std:
        return mu
    var = (w * x[:n] * x[:n]).sum(0) - mu * mu
    return torch.cat([mu, torch.sqrt(torch.clamp(var, min=0.0) + float(np.float32(eps)))])


@pytest.mark.parametrize("D,H", [(1, 1), (6, 1), (6, 3), (6, 6), (130, 2)])
@pytest.mark.parametrize("include_std", [True, False])
def test_reference_gradients_match_fp64_autograd(D, H, include_std):
    rng = np.random.default_rng([D, H])
    T, n = 23, 19
    x = rng.standard_normal((T, D)).astype(np.float32)
    e = (2 * rng.standard_normal((T, H))).astype(np.float32)
    gout = rng.standard_normal(2 * D if include_std else D).astype(np.float32)
    f = R.forward(x, e, n, include_std)
    g = R.backward(x, e, n, gout, f, include_std)
    tx, te = torch.tensor(x, dtype=F64, requires_grad=True), torch.tensor(e, dtype=F64, requires_grad=True)
    out = torch_pool(tx, te, n, include_std)
    (out * torch.tensor(gout, dtype=F64)).sum().backward()
    assert np.abs(f["out"] - out.detach().numpy()).max() <= 1e-12
    assert np.abs(g["dx"] - tx.grad.numpy()).max() <= 1e-12
    assert np.abs(g["de"] - te.grad.numpy()).max() <= 1e-12
    assert not g["dx"][n:].any() and not g["de"][n:].any()
    assert (g["dx_bound"][:n] > 0).all() and (g["de_bound"][:n] > 0).all() and (f["out_bound"] > 0).all()


@pytest.mark.parametrize("H", [1, 3, 6])
def test_constant_logits_reproduce_the_plain_pooling(H):
    rng = np.random.default_rng(H)
    B, T, D = 4, 40, 6
    x = rng.standard_normal((B, T, D)).astype(np.float32)
    e = np.repeat(rng.standard_normal((B, 1, H)).astype(np.float32), T, axis=1)
    lens = [40, 1, 17, 0]
    want, _ = P.pool(x, lens)
    got = R.pool(x, e, lens)["out"]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[3]).all()
    assert np.abs(got[:3] - want[:3]).max() <= 1e-13


def test_empty_utterance_and_unread_rows():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((9, 4)).astype(np.float32)
    e = rng.standard_normal((9, 2)).astype(np.float32)
    f = R.forward(x, e, 5)
    x2, e2 = x.copy(), e.copy()
    x2[5:], e2[5:] = np.nan, np.nan
    f2 = R.forward(x2, e2, 5)
    assert np.array_equal(f["out"], f2["out"])
    g = R.backward(x2, e2, 5, np.ones(8, np.float32), f2)
    assert not np.isnan(g["dx"]).any() and not g["dx"][5:].any() and not g["de"][5:].any()
    z = R.backward(x, e, 0, np.ones(8, np.float32), R.forward(x, e, 0))
    assert not z["dx"].any() and not z["de"].any()


# ----------------------------------------------------------------------------- what the bounds assume of the GPU test's inputs
def test_gpu_inputs_meet_the_bounds_assumptions():
    tags = []
    for tag, x, e, lens, gradients in R.gpu_inputs():
        R.check_inputs(x, e, lens, R.pool(x, e, lens)["fwd"], gradients)
        tags.append(tag)
    assert len(tags) == len(set(tags)) == 2 * len(R.DIMS) + 1 + len(R.STRIDE_DIMS) + len(R.INVARIANCE_CASES) + 2 * len(R.SHIFT_DIMS) \
        + len(R.CONST_LOGIT_DIMS) + len(R.AUTOGRAD_DIMS) + 1


def test_constant_channel_lies_within_the_bound_on_both_branches():
    D, H = 30, 5
    x, e, lens, gout = R.kernel_case(D, H, True, 7)
    r = R.pool(x, e, lens)
    for b, f in enumerate(r["fwd"]):
        n = f["n"]
        if n < 2:
            continue
        assert f["const"][7] and f["const"].sum() == 1
        on = R.backward(x[b], e[b], n, gout[b], f, live=True)
        off = R.backward(x[b], e[b], n, gout[b], f, live=False)
        for k in ("dx", "de"):
            # (half of the smaller bound: whichever branch the restatement took, the other one leaves the kernel the other half)
            assert (np.abs(on[k] - off[k]) <= 0.5 * np.minimum(on[k + "_bound"], off[k + "_bound"])).all(), (b, k)


# ----------------------------------------------------------------------------- the C-ABI
def test_header_symbols_are_the_attn_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_attn.h")).read()
    code = hdr[hdr.index("#ifndef KTF_ATTN_H_"):]
    protos = re.findall(r"^(?:int|int32_t|int64_t) (ktf_[a-z0-9_]+)\(([^;]*)\);", code, flags=re.M)
    assert {n for n, _ in protos} == set(L.ATTN_PROTOTYPES) == set(re.findall(r"\b(ktf_[a-z0-9_]+)\s*\(", code))
    ctype = {"const float*": L._P, "float*": L._P, "const double*": L._P, "double*": L._P, "const int32_t*": L._P, "void*": L._P,
             "int64_t": L._i64, "int32_t": L._i32, "float": L._f32, "size_t": C.c_size_t}
    res = {"int": C.c_int, "int64_t": L._i64}
    for name, args in protos:
        want = [ctype[" ".join(a.split()[:-1])] for a in args.replace("\n", " ").split(",")]
        assert L.ATTN_PROTOTYPES[name][1] == want, name
        assert L.ATTN_PROTOTYPES[name][0] is res[re.search(rf"^(\w+) {name}\(", code, flags=re.M).group(1)], name
    assert all(n.startswith("ktf_attn_") for n in L.ATTN_PROTOTYPES)
    lib = L.load()
    for name in L.ATTN_PROTOTYPES:
        assert hasattr(lib, name), name
    families = [L.PROTOTYPES, L.AUGMENT_PROTOTYPES, L.RESAMPLE_PROTOTYPES, L.GRAD_PROTOTYPES, L.NORM_PROTOTYPES, L.LOSS_PROTOTYPES,
                L.EGS_PROTOTYPES, L.OPTIM_PROTOTYPES, L.HEAD_PROTOTYPES]
    assert not set(L.ATTN_PROTOTYPES) & set().union(*families)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "ktf_attn.h":
            assert "ktf_attn_" not in open(os.path.join(ROOT, "include", other)).read(), other
    for name, val in (("BATCH", L.ATTN_MAX_BATCH), ("ROWS", L.ATTN_MAX_ROWS), ("DIM", L.ATTN_MAX_DIM)):
        assert int(re.search(rf"#define KTF_ATTN_MAX_{name} (\d+)", hdr).group(1)) == val
    assert len(L.PROTOTYPES) == 120 and lib.ktf_version() == 117          # (the families that were there stay as they are)


@pytest.fixture
def host_calls(monkeypatch):
    """ops on CPU tensors: the library gets host pointers and a null stream, which is enough for every refusal (they come before
    any launch). -> the library."""
    monkeypatch.setattr(L, "stream_ptr", lambda: None)
    monkeypatch.setattr(L, "on_device", lambda device: contextlib.nullcontext())
    return L.load()


def _args(B=2, T=5, D=6, H=3, ldx=None, lde=None, ld_out=None, ld_dx=None, ld_de=None, std=True):
    ldx, lde = ldx or D, lde or H
    od = 2 * D if std else D
    f32 = torch.float32
    return dict(x=torch.zeros(B, T, ldx), e=torch.zeros(B, T, lde), lens=torch.full((B,), T, dtype=torch.int32),
                out=torch.zeros(B, ld_out or od), norm=torch.zeros(B, H, 2, dtype=F64), stats=torch.zeros(B, 2, D, dtype=F64),
                gout=torch.zeros(B, ld_out or od), dx=torch.zeros(B, T, ld_dx or D, dtype=f32), de=torch.zeros(B, T, ld_de or H, dtype=f32),
                ws=torch.zeros(max(ops._size("ktf_attn_pool_backward_workspace_bytes", B, D, H), 256) + 512, dtype=torch.uint8))


def _aligned(ws):
    off = (-ws.data_ptr()) % 256
    return ws[off:off + ws.numel() - 256]


def _fwd(a, D=6, H=3, std=True, eps=1e-10, **over):
    a = dict(a, **over)
    return ops.attn_pool(a["x"], a["e"], a["lens"], std, eps, a["out"], a["norm"], a["stats"], D=D, H=H)


def _bwd(a, D=6, H=3, std=True, eps=1e-10, **over):
    a = dict(a, **over)
    ws = a["ws"] if a["ws"] is None or over.get("raw_ws") else _aligned(a["ws"])
    return ops.attn_pool_backward(a["x"], a["e"], a["lens"], std, eps, a["norm"], a["stats"], a["gout"], a["dx"], a["de"], ws, D=D, H=H)


def test_every_refusal_of_rule_13_through_ops(host_calls):
    a = _args()
    with pytest.raises(ValueError, match="null"):
        _fwd(a, norm=None)
    for name in ("norm", "stats", "ws"):
        with pytest.raises(ValueError, match="null"):
            _bwd(a, **{name: None})
    for fn in (_fwd, _bwd):
        for D, H in ((0, 1), (6, 0), (6, 4), (3, 6), (-6, 3)):
            with pytest.raises(ValueError, match="D % H"):
                fn(a, D=D, H=H)
        with pytest.raises(ValueError, match="ldx < D or lde < H"):
            fn(a, D=12, H=3)
        with pytest.raises(ValueError, match="ldx < D or lde < H"):
            fn(_args(D=8, H=8, lde=4), D=8, H=8)
        for eps in (-1e-10, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="eps"):
                fn(a, eps=eps)
    with pytest.raises(ValueError, match="ld_out too small"):
        _fwd(_args(ld_out=11))
    with pytest.raises(ValueError, match="ld_out too small"):
        _fwd(_args(ld_out=5, std=False), std=False)
    with pytest.raises(ValueError, match="ld_gout too small"):
        _bwd(_args(ld_out=11))
    b = _args(ldx=8, lde=4)
    with pytest.raises(ValueError, match="ld_dx < D or ld_de < H"):
        _bwd(b, D=8, H=4, gout=torch.zeros(2, 16))
    with pytest.raises(ValueError, match="ld_dx < D or ld_de < H"):
        _bwd(dict(b, dx=torch.zeros(2, 5, 8)), D=8, H=4, gout=torch.zeros(2, 16))
    with pytest.raises(ValueError, match="workspace"):
        _bwd(a, ws=torch.zeros(256 + 128, dtype=torch.uint8))
    with pytest.raises(ValueError, match="256-byte"):
        _bwd(a, ws=_aligned(a["ws"])[4:], raw_ws=True)
    lib = host_calls
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))

    def raw(B=2, T=5, D=6, H=3):
        return lib.ktf_attn_pool(p, B, T, D, max(D, 1), p, H, max(H, 1), None, 1, 1e-10, p, 2 * max(D, 1), p, p, None)
    for kw, text in ((dict(B=-1), ">= 0"), (dict(T=-1), ">= 0"), (dict(B=L.ATTN_MAX_BATCH + 1), "B 65536 above"),
                     (dict(T=L.ATTN_MAX_ROWS + 1), "T 1073741825 above"), (dict(D=L.ATTN_MAX_DIM * 2, H=1), "D 2097152 above")):
        assert raw(**kw) == -1 and text in L.last_error(), (kw, L.last_error())
    for bad in ((-1, 6, 3), (L.ATTN_MAX_BATCH + 1, 6, 3), (2, 0, 1), (2, 6, 4), (2, L.ATTN_MAX_DIM * 2, 1)):
        assert lib.ktf_attn_pool_backward_workspace_bytes(*bad) == -1
    assert lib.ktf_attn_pool_backward_workspace_bytes(0, 6, 3) == 512
    assert lib.ktf_attn_pool_backward_workspace_bytes(3, 100, 4) == 4864 + 256
    assert lib.ktf_attn_pool(None, 0, 0, 6, 6, None, 3, 3, None, 1, 1e-10, p, 12, p, None, None) == 0      # B = 0: nothing to do
    with pytest.raises(ValueError, match="same B and T"):
        ops.attn_pool(torch.zeros(2, 5, 6), torch.zeros(2, 4, 3), None, True, 1e-10, a["out"], a["norm"])
    with pytest.raises(ValueError, match="fp32"):
        ops.attn_pool(torch.zeros(2, 5, 6, dtype=F64), torch.zeros(2, 5, 3), None, True, 1e-10, a["out"], a["norm"])


# ----------------------------------------------------------------------------- the layer, the YAML kind and the training module
def _weights(rng, D, A, H):
    return [rng.standard_normal((D, A)).astype(np.float32), rng.standard_normal(A).astype(np.float32),
            rng.standard_normal((A, H)).astype(np.float32), rng.standard_normal(H).astype(np.float32)]


@pytest.mark.parametrize("kind", ["attentive_stats", "attentive_stats_pooling", "Attentive_Stats"])
def test_cfg2layers_builds_the_layer_from_both_spellings(kind):
    (layer,) = ktf.models.cfg2layers({"name": "pool", "type": kind, "cfg": {"attention_units": 16, "heads": 4, "include_std": False}})
    assert isinstance(layer, ktf.layers.AttentiveStatsPooling) and layer.name == "pool"
    assert (layer.attentionUnits, layer.heads, layer.includeStd, layer.epsilon, layer.attentionActivation) == (16, 4, False, 1e-10, "tanh")
    assert layer.reduce is True and layer.hidden.context == [0] and layer.logits.context == [0]
    assert layer.hidden.units == 16 and layer.logits.units == 4 and layer.hidden.activation == "tanh"
    with pytest.raises(TypeError):
        ktf.models.cfg2layers({"name": "pool", "type": kind, "cfg": {"heads": 4}})
    with pytest.raises(ValueError, match="unsupported layer type"):
        ktf.models.cfg2layers({"name": "pool", "type": "attentive"})


def test_layer_config_round_trip_shapes_and_weights():
    L0 = ktf.layers.AttentiveStatsPooling
    layer = L0(8, heads=3, include_std=True, epsilon=1e-8, attention_activation="relu", name="asp")
    cfg = layer.get_config()
    twin = L0.from_config(cfg)
    assert twin.get_config() == cfg and cfg["attention_units"] == 8 and cfg["heads"] == 3 and cfg["attention_activation"] == "relu"
    assert layer.compute_output_shape((5, 100, 12)) == (5, 1, 24)
    assert L0(8, include_std=False).compute_output_shape((None, None, 12)) == (None, 1, 12)
    assert layer.get_weights() == []
    layer.build((None, None, 12))
    got = layer.get_weights()
    assert [w.shape for w in got] == [(12, 8), (8,), (8, 3), (3,)]
    rng = np.random.default_rng(0)
    w = _weights(rng, 12, 8, 3)
    v0 = layer._version
    layer.set_weights(w)
    assert layer._version > v0
    for a, b in zip(layer.get_weights(), w):
        assert np.array_equal(a, b)
    layer.set_weights([w[0].T, w[1], w[2].T, w[3]], fmt="kaldi")
    for a, b in zip(layer.get_weights(), w):
        assert np.array_equal(a, b)
    for bad in ([w[0]], [w[0].T, w[1], w[2], w[3]], [w[0], w[1][:-1], w[2], w[3]], [w[0], w[1], w[2][:, :2], w[3]],
                [w[0], w[1], w[2], np.zeros(4, np.float32)]):
        with pytest.raises(ValueError):
            layer.set_weights(bad)
    with pytest.raises(ValueError, match="fmt"):
        layer.set_weights(w, fmt="numpy")
    with pytest.raises(ValueError, match="does not divide"):
        L0(8, heads=5).build((None, None, 12))
    fresh = L0(8, heads=3)
    fresh.set_weights(w)                                         # (unbuilt: the input width comes from W1)
    assert fresh.built and fresh.inputDim == 12
    for bad in (dict(attention_units=0), dict(attention_units=4, heads=0), dict(attention_units=4, epsilon=-1.0),
                dict(attention_units=4, epsilon=float("nan")), dict(attention_units=4, attention_activation="nope")):
        with pytest.raises(ValueError):
            L0(**bad)


def _attentive_model(act="tanh", heads=2):
    M, Y = ktf.models, ktf.layers
    return M.Sequential([M.Input(shape=(None, 6)), Y.TDNN(8, [-1, 0, 1], name="t1"), Y.ReLU(), Y.BatchNorm(name="b1"),
                         Y.AttentiveStatsPooling(5, heads=heads, attention_activation=act, name="asp"), Y.TDNN(4, [0], name="t2")])


def test_plan_and_tail_take_the_layer_as_the_pooling():
    seq = _attentive_model()
    steps = seq._plan()
    assert [s[0] for s in steps] == ["tdnn", "attn", "tdnn"] and seq._tail_step(steps) == 2
    sig = seq.weights_signature()
    seq.get_layer("asp").set_weights(_weights(np.random.default_rng(1), 8, 5, 2))
    assert seq.weights_signature() != sig
    M, Y = ktf.models, ktf.layers
    two = M.Sequential([M.Input(shape=(None, 6)), Y.AttentiveStatsPooling(5, name="p1"), Y.AttentiveStatsPooling(5, name="p2")])
    assert two._plan() is None


def test_trainable_sequential_takes_the_layer_and_exports_it():
    A = ktf.autograd
    seq = _attentive_model()
    mod = A.TrainableSequential(seq, device="cpu")
    kinds = [k for k, _, _ in mod.steps]
    assert kinds == ["tdnn", "relu", "bn", "attn", "tdnn"]
    at = mod.steps[3][2]
    assert [tuple(mod.params[at + k].shape) for k in range(4)] == [(5, 1, 8), (5,), (2, 1, 5), (2,)]
    asp = seq.get_layer("asp")
    w0 = [w.copy() for w in asp.get_weights()]
    assert np.array_equal(mod.params[at].detach().numpy()[:, 0, :].T, w0[0])
    assert np.array_equal(mod.params[at + 2].detach().numpy()[:, 0, :].T, w0[2])
    with torch.no_grad():
        for k in range(4):
            mod.params[at + k].add_(1.0 + k)
    assert mod.export() is seq
    for k, (a, b) in enumerate(zip(asp.get_weights(), w0)):
        assert np.array_equal(a, b + np.float32(1.0 + k)), k
    with pytest.raises(NotImplementedError, match="has no gradient in ktf.autograd"):
        A.TrainableSequential(_attentive_model(act="sigmoid"), device="cpu")
    M, Y = ktf.models, ktf.layers
    twice = M.Sequential([M.Input(shape=(None, 6)), Y.AttentiveStatsPooling(5, name="p1"), Y.AttentiveStatsPooling(5, name="p2")])
    with pytest.raises(NotImplementedError, match="has no gradient in ktf.autograd"):
        A.TrainableSequential(twice, device="cpu")
    with pytest.raises(ValueError, match="divide"):
        A.attentive_stats_pooling(torch.zeros(1, 2, 6), torch.zeros(1, 2, 4))
    with pytest.raises(ValueError, match="epsilon"):
        A.attentive_stats_pooling(torch.zeros(1, 2, 6), torch.zeros(1, 2, 3), epsilon=-1.0)
    with pytest.raises(L.KtfBackendError, match="GPU"):
        A.attentive_stats_pooling(torch.zeros(1, 2, 6), torch.zeros(1, 2, 3))
