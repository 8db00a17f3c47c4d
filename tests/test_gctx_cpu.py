"""Global-context attention without a GPU: tests/_gctx_ref.py against torch.cat([x, mu, sigma]) @ W1 in fp64, the C-ABI of
include/ktf_gctx.h (symbols, every refusal of rule 10), the layer's option, and the conditions tests/test_gpu_gctx.py relies on."""

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
import _gctx_ref as R  # noqa: E402


@pytest.mark.parametrize("D,A,H,n,act", [(5, 3, 1, 70, "tanh"), (33, 17, 11, 1, "relu"), (8, 4, 8, 129, "tanh")])
def test_reference_is_the_attention_on_the_concatenation(D, A, H, n, act):
    rng = np.random.default_rng(D)
    x, w1, b1, w2, b2 = (rng.standard_normal(s).astype(np.float32) for s in ((n + 3, D), (3 * D, A), (A,), (A, H), (H,)))
    r = R.utterance(x, n, w1, b1, w2, b2, act, eps=1e-5)
    tx, (tw1, tb1, tw2, tb2) = torch.as_tensor(x[:n], dtype=torch.float64), (torch.as_tensor(a, dtype=torch.float64) for a in (w1, b1, w2, b2))
    mu = tx.mean(0)
    sigma = ((tx * tx).mean(0) - mu * mu).clamp(min=0).add(float(np.float32(1e-5))).sqrt()
    z = torch.cat([tx, mu.expand(n, D), sigma.expand(n, D)], 1) @ tw1 + tb1
    h = torch.tanh(z) if act == "tanh" else z.clamp(min=0)
    for got, want in ((r["mu"], mu), (r["sigma"], sigma), (r["h"], h), (r["e"], h @ tw2 + tb2), (r["g"], torch.cat([mu, sigma]) @ tw1[D:] + tb1)):
        assert np.abs(got - want.numpy()).max() <= 1e-12
    assert (r["S"] >= np.abs(r["g"])).all()


def test_header_symbols_are_the_gctx_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_gctx.h")).read()
    protos = re.findall(r"^(?:int|int32_t) (ktf_[a-z0-9_]+)\(([^;]*)\);", hdr[hdr.index("#ifndef KTF_GCTX_H_"):], flags=re.M)
    assert {n for n, _ in protos} == set(L.GCTX_PROTOTYPES) == {"ktf_gctx_stats", "ktf_gctx_bias", "ktf_gctx_logits", "ktf_gctx_row_tile"}
    ctype = {"const float*": L._P, "float*": L._P, "const double*": L._P, "double*": L._P, "const int32_t*": L._P, "void*": L._P, "int64_t": L._i64,
             "int32_t": L._i32, "float": L._f32}
    for name, args in protos:
        assert L.GCTX_PROTOTYPES[name][1] == [ctype[" ".join(a.split()[:-1])] for a in args.replace("\n", " ").split(",")], name
    lib = L.load()
    others = [getattr(L, n) for n in dir(L) if n.endswith("PROTOTYPES") and n != "GCTX_PROTOTYPES"]
    assert all(hasattr(lib, n) for n in L.GCTX_PROTOTYPES) and len(others) >= 14 and not any(set(L.GCTX_PROTOTYPES) & set(o) for o in others)
    limits = {n: int(v) for n, v in re.findall(r"#define KTF_GCTX_MAX_(\w+) (\d+)", hdr)}
    assert limits == dict(UNITS=L.GCTX_MAX_UNITS, BATCH=L.ATTN_MAX_BATCH, ROWS=L.ATTN_MAX_ROWS, DIM=L.ATTN_MAX_DIM) and L.GCTX_MAX_UNITS == 256
    assert len(L.PROTOTYPES) == 120 and lib.ktf_version() == 117          # (the families that were there stay as they are)


def test_every_refusal_of_rule_10(monkeypatch):
    monkeypatch.setattr(L, "stream_ptr", lambda: None)       # host pointers and a null stream: every refusal comes before any launch
    monkeypatch.setattr(L, "on_device", lambda device: contextlib.nullcontext())
    B, T, D, A, H = 2, 5, 6, 4, 3
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)      # noqa: E731
    logits = lambda D_=None, A_=A, ldg=A, act=L.ACT_TANH, gemm=L.GEMM_F32: ops.gctx_logits(      # noqa: E731
        z(B, T, D), None, z(D_ or D, A_), z(B, ldg), act, z(A_, H), z(H), gemm, z(B, T, H), D=D_)
    stats = lambda eps=0.0, D_=D: ops.gctx_stats(z(B, T, D), None, eps, z(B, 2, D_, dt=torch.float64), D=D_)      # noqa: E731
    bias = lambda A_=A, ldg=A: ops.gctx_bias(z(B, 2, D, dt=torch.float64), z(2 * D, A_), None, z(B, ldg))      # noqa: E731
    for fn, kw, what in ((logits, dict(D_=7), "ldx"), (logits, dict(A_=257, ldg=257), "A 257"), (logits, dict(ldg=3), "ldg"), (logits, dict(act=L.ACT_NONE), "act"),
                         (logits, dict(act=L.ACT_SIGMOID), "act"), (logits, dict(gemm=L.GEMM_BF16), "gemm"), (logits, dict(gemm=L.GEMM_F16MX), "gemm"),
                         (logits, dict(gemm=L.GEMM_BF16X4), "gemm"), (stats, dict(eps=-1.0), "eps"), (stats, dict(eps=float("inf")), "eps"),
                         (stats, dict(eps=float("nan")), "eps"), (stats, dict(D_=D + 1), "ldx"), (bias, dict(ldg=A - 1), "ldg"), (bias, dict(A_=257, ldg=257), "A 257")):
        with pytest.raises(ValueError, match=what):
            fn(**kw)
    lib, P = L.load(), C.c_void_p(8)                           # what the wrappers cannot be asked: sizes, limits and null pointers
    lg = lambda B_=B, T_=T, D_=D, A_=A, H_=H, ldx=D, ldw1=A, ldw2=H, lde=H, x=P, w1=P, g=P, w2=P, e=P: lib.ktf_gctx_logits(      # noqa: E731
        x, B_, T_, D_, ldx, None, w1, ldw1, g, A, A_, L.ACT_RELU, w2, ldw2, None, H_, L.GEMM_BF16X3, e, lde, None)
    assert [lg(B_=-1), lg(T_=-1), lg(B_=65536), lg(T_=(1 << 30) + 1), lg(D_=0), lg(A_=0), lg(H_=0), lg(H_=(1 << 20) + 1, ldw2=1 << 21, lde=1 << 21), lg(ldx=D - 1),
            lg(ldw1=A - 1), lg(ldw2=H - 1), lg(lde=H - 1), lg(lde=1 << 31), lg(x=None), lg(w1=None), lg(g=None), lg(w2=None), lg(e=None)] == [-1] * 18
    assert [lib.ktf_gctx_stats(P, B, T, D, D, None, 0.0, None, None), lib.ktf_gctx_stats(None, B, T, D, D, None, 0.0, P, None),
            lib.ktf_gctx_bias(P, B, D, P, A, None, A, None, A, None), lib.ktf_gctx_bias(None, B, D, P, A, None, A, P, A, None)] == [-1] * 4
    assert lg(T_=0, x=None, e=None) == 0 and ops.gctx_row_tile(1, 1) == ops.gctx_row_tile(256, 1 << 20, L.GEMM_BF16X3) == 64
    for bad in ((0, 1, 0), (257, 1, 0), (8, 0, 0), (8, 1, L.GEMM_BF16), (8, 1, 7)):
        with pytest.raises(ValueError):
            ops.gctx_row_tile(*bad)


def test_layer_option_weight_formats_config_yaml_key_and_training_refusal():
    D, A, H = 12, 8, 3
    w = [np.random.default_rng(2).standard_normal(s).astype(np.float32) for s in ((3 * D, A), (A,), (A, H), (H,))]
    layer = ktf.layers.AttentiveStatsPooling(A, heads=H, global_context=True, name="pool")
    layer.set_weights(w)
    assert layer.inputDim == D and layer.contextKernel.shape == (2 * D, A) and all(np.array_equal(a, b) for a, b in zip(layer.get_weights(), w))
    twin = ktf.layers.AttentiveStatsPooling.from_config(layer.get_config())
    twin.set_weights([w[0].T, w[1], w[2].T, w[3]], fmt="kaldi")
    assert twin.globalContext and twin.get_config() == layer.get_config() and all(np.array_equal(a, b) for a, b in zip(twin.get_weights(), w))
    fresh = ktf.layers.AttentiveStatsPooling(A, heads=H, global_context=True, name="pool")
    fresh.build((2, 7, D))
    assert [a.shape for a in fresh.get_weights()] == [(3 * D, A), (A,), (A, H), (H,)]
    for bad in ([w[0][:D], *w[1:]], [w[0][:3 * D - 1], *w[1:]], [w[0], w[1][:-1], *w[2:]], w[:3]):
        with pytest.raises(ValueError):
            layer.set_weights(bad)
    for kw in (dict(attention_activation="sigmoid"), dict(attention_units=257)):
        with pytest.raises(ValueError, match="global_context"):
            ktf.layers.AttentiveStatsPooling(**{"attention_units": A, "global_context": True, **kw})
    plain = ktf.layers.AttentiveStatsPooling(A, heads=H)
    assert not plain.globalContext and "global_context" not in plain.get_config()
    for kind in ("attentive_stats", "attentive_stats_pooling"):
        made = ktf.models.cfg2layers({"name": "pool", "type": kind, "cfg": {"attention_units": A, "heads": H, "global_context": True}})
        assert len(made) == 1 and made[0].globalContext and made[0].name == "pool"
    mdl = ktf.models.SequentialFromConfig({"layers": [{"type": "input", "shape": [None, None, 24]}, {"name": "t1", "type": ["tdnn", "relu"], "cfg": {"units": 32}},
                                                      {"name": "ctxpool", "type": "attentive_stats", "cfg": {"attention_units": 8, "global_context": True}}]})
    with pytest.raises(NotImplementedError, match="ctxpool.*global_context"):
        ktf.autograd.TrainableSequential(mdl, device="cpu")


@pytest.mark.parametrize("D,A,H", R.EXACT_SHAPES)
def test_inputs_of_the_bitwise_gpu_test_are_exact(D, A, H):
    lens, c = R.exact_case(D, A, H, ops.gctx_row_tile(A, H))
    assert all((v == np.rint(v)).all() and np.abs(v).max() <= 8 for v in c.values()) and np.abs(c["w2"]).max() <= 2 and np.abs(c["b2"]).max() <= 2
    top = (np.abs(c["x"]).astype(np.float64) @ np.abs(c["w1x"]) + np.abs(c["g"])[:, None, :]).max()           # every partial sum of h: an integer below 2^16
    assert top < 2.0 ** 16 and top * np.abs(c["w2"]).sum(0).max() + 2 < 2.0 ** 24           # ... and of e below 2^24
    for b, n in enumerate(lens):
        h, e = R.logits(c["x"][b], n, c["w1x"], c["g"][b], c["w2"], c["b2"], "relu")
        assert (h == np.rint(h)).all() and (e == np.rint(e)).all() and np.array_equal(e.astype(np.float32).astype(np.float64), e)


@pytest.mark.parametrize("D,A", [(1, 1), (5, 33), (64, 128), (130, 1)])
def test_channels_of_the_stats_test_are_well_conditioned_or_constant(D, A):
    c = R.stats_case(D, A)
    for b, n in enumerate(R.STATS_LENS[1:], 1):
        r, const = R.stats(c["x"][b], n, 1e-10), (c["x"][b, :n] == c["x"][b, 0]).all(0)
        assert (const | (r["var"] > 2.0 ** -20 * r["q"])).all() and const[0] and np.isfinite(r["sigma_bound"]).all()
