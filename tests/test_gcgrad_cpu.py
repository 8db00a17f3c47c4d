"""The gradient of global-context attention without a GPU: tests/_gcgrad_ref.py against fp64 torch.autograd on torch.cat([x, mu, sigma]) @
W1, the C-ABI of include/ktf_gcgrad.h (symbols, every refusal of rule 10) and TrainableSequential(global_context=True) on the CPU."""

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
import _gcgrad_ref as R  # noqa: E402


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("D,A,H,n", [(5, 3, 1, 70), (33, 17, 11, 1), (8, 4, 8, 129)])
def test_reference_is_autograd_of_the_attention_on_the_concatenation(D, A, H, n, act):
    c = R.case(D, A, H, n + 3, [n])
    eps = 1e-5
    r = R.utterance(c["x"][0], n, c["w1"], c["b1"], c["w2"], c["de"][0], act, eps)
    tx, tw1, tb1, tw2 = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (c["x"][0, :n], c["w1"], c["b1"], c["w2"]))
    tb2 = torch.zeros(H, dtype=torch.float64, requires_grad=True)
    mu = tx.mean(0)
    sigma = ((tx * tx).mean(0) - mu * mu).clamp(min=0).add(float(np.float32(eps))).sqrt()
    z = torch.cat([tx, mu.expand(n, D), sigma.expand(n, D)], 1) @ tw1 + tb1
    e = (torch.tanh(z) if act == "tanh" else z.clamp(min=0)) @ tw2 + tb2
    e.backward(torch.tensor(c["de"][0, :n], dtype=torch.float64))
    got = dict(dx=r["dx"][0], dw1=np.concatenate([r["dw1x"][0], r["dw1c"][0]]), db1=r["db1"][0], dw2=r["dw2"][0], db2=r["db2"][0])
    for (name, g), t in zip(got.items(), (tx, tw1, tb1, tw2, tb2)):
        assert np.abs(g - t.grad.numpy()).max() <= 1e-10 * max(1.0, float(t.grad.abs().max())), name
    assert all((S >= np.abs(v) * (1 - 1e-12)).all() for v, S in r.values())
    assert n == 1 or r["coef"][0][1, 0] == 0.0                # (the constant channel: s_c = 0)


def test_header_symbols_are_the_gcgrad_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_gcgrad.h")).read()
    protos = re.findall(r"^(?:int|int32_t|int64_t) (ktf_[a-z0-9_]+)\(([^;]*)\);", hdr[hdr.index("#ifndef KTF_GCGRAD_H_"):], flags=re.M)
    assert {n for n, _ in protos} == set(L.GCGRAD_PROTOTYPES) and len(protos) == 5 and all(n.startswith("ktf_gcgrad_") for n, _ in protos)
    ctype = {"const float*": L._P, "float*": L._P, "const double*": L._P, "double*": L._P, "const int32_t*": L._P, "void*": L._P, "int64_t": L._i64,
             "int32_t": L._i32, "float": L._f32, "size_t": C.c_size_t}
    for name, args in protos:
        assert L.GCGRAD_PROTOTYPES[name][1] == [ctype[" ".join(a.split()[:-1])] for a in args.replace("\n", " ").split(",")], name
    lib = L.load()
    others = [getattr(L, n) for n in dir(L) if n.endswith("PROTOTYPES") and n != "GCGRAD_PROTOTYPES"]
    assert all(hasattr(lib, n) for n in L.GCGRAD_PROTOTYPES) and len(others) >= 15 and not any(set(L.GCGRAD_PROTOTYPES) & set(o) for o in others)
    assert len(L.PROTOTYPES) == 120 and lib.ktf_version() == 117          # (the families that were there stay as they are)


def test_every_refusal_of_rule_10(monkeypatch):
    monkeypatch.setattr(L, "stream_ptr", lambda: None)       # host pointers and a null stream: every refusal comes before any launch
    monkeypatch.setattr(L, "on_device", lambda device: contextlib.nullcontext())
    B, T, D, A, H = 2, 5, 6, 4, 3
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)      # noqa: E731
    ws = torch.zeros(4096 + 256, dtype=torch.uint8)
    ws = ws[(-ws.data_ptr()) % 256:][:4096]
    hidden = lambda D_=None, A_=A, ldg=A, act=L.ACT_TANH, gemm=L.GEMM_F32: ops.gcgrad_hidden(      # noqa: E731
        z(B, T, D), None, z(D_ or D, A_), z(B, ldg), act, z(A_, H), gemm, z(B, T, H), z(B, T, A_), z(B, T, A_), D=D_)
    context = lambda eps=0.0, A_=A, w=ws: ops.gcgrad_context(z(B, T, A_), None, z(B, 2, D, dt=torch.float64), z(2 * D, A_), eps, None, None,      # noqa: E731
                                                             z(B, 2, D, dt=torch.float64), w)
    data = lambda D_=None, A_=A, gemm=L.GEMM_F32: ops.gcgrad_data(z(B, T, A_), None, z(D_ or D, A_), z(B, T, D), z(B, 2, D_ or D, dt=torch.float64),      # noqa: E731
                                                                  z(B, 2, D_ or D, dt=torch.float64), gemm, z(B, T, D_ or D), D=D_)
    for fn, kw, what in ((hidden, dict(D_=7), "ldx"), (hidden, dict(A_=257, ldg=257), "A 257"), (hidden, dict(ldg=3), "ldg"), (hidden, dict(act=L.ACT_NONE), "act"),
                         (hidden, dict(act=L.ACT_SIGMOID), "act"), (hidden, dict(gemm=L.GEMM_BF16), "gemm"), (hidden, dict(gemm=L.GEMM_F16MX), "gemm"),
                         (context, dict(eps=-1.0), "eps"), (context, dict(eps=float("nan")), "eps"), (context, dict(A_=257), "A 257"),
                         (context, dict(w=ws[:8]), "workspace"), (context, dict(w=ws[1:]), "workspace"), (data, dict(D_=7), "ldx"),
                         (data, dict(A_=257), "A 257"), (data, dict(gemm=L.GEMM_BF16), "gemm")):
        with pytest.raises(ValueError, match=what):
            fn(**kw)
    lib, P = L.load(), C.c_void_p(256)                         # what the wrappers cannot be asked: sizes, limits and null pointers
    hd = lambda B_=B, T_=T, D_=D, A_=A, H_=H, ldx=D, ldw1=A, ldw2=H, lde=H, ldz=A, x=P, w1=P, g=P, w2=P, de=P, dz=P, h=P: lib.ktf_gcgrad_hidden(      # noqa: E731
        x, B_, T_, D_, ldx, None, w1, ldw1, g, A, A_, L.ACT_RELU, w2, ldw2, H_, L.GEMM_BF16X3, de, lde, dz, h, ldz, None)
    assert [hd(B_=-1), hd(T_=-1), hd(B_=65536), hd(T_=(1 << 30) + 1), hd(D_=0), hd(A_=0), hd(H_=0), hd(H_=(1 << 20) + 1, ldw2=1 << 21, lde=1 << 21), hd(ldx=D - 1),
            hd(ldw1=A - 1), hd(ldw2=H - 1), hd(lde=H - 1), hd(ldz=A - 1), hd(ldz=1 << 31), hd(x=None), hd(w1=None), hd(g=None), hd(w2=None), hd(de=None),
            hd(dz=None), hd(h=None)] == [-1] * 21
    cx = lambda B_=B, ldz=A, ldw=A, lddw=A, dz=P, ctx=P, w=P, dw=P, coef=P, wsp=P, n=4096: lib.ktf_gcgrad_context(      # noqa: E731
        dz, B_, T, A, ldz, None, ctx, D, w, ldw, 0.0, dw, lddw, None, coef, wsp, n, None)
    assert [cx(B_=-1), cx(ldz=A - 1), cx(ldw=A - 1), cx(lddw=A - 1), cx(dz=None), cx(ctx=None), cx(w=None), cx(coef=None), cx(wsp=None), cx(n=8),
            cx(wsp=C.c_void_p(264))] == [-1] * 11
    dt = lambda T_=T, ldz=A, ldw1=A, ldx=D, lddx=D, dz=P, w1=P, x=P, ctx=P, coef=P, dx=P: lib.ktf_gcgrad_data(      # noqa: E731
        dz, B, T_, A, ldz, None, w1, ldw1, D, x, ldx, ctx, coef, L.GEMM_F32, 1, dx, lddx, None)
    assert [dt(T_=-1), dt(ldz=A - 1), dt(ldw1=A - 1), dt(ldx=D - 1), dt(lddx=D - 1), dt(dz=None), dt(w1=None), dt(x=None), dt(ctx=None), dt(coef=None),
            dt(dx=None)] == [-1] * 11
    assert hd(T_=0, x=None, de=None, dz=None, h=None) == 0 and dt(T_=0, dz=None, x=None, dx=None) == 0 and cx(B_=0, ctx=None, wsp=None) == 0
    assert ops.gcgrad_row_tile(1, 1) == ops.gcgrad_row_tile(256, 1 << 20, L.GEMM_BF16X3) == 64
    assert lib.ktf_gcgrad_workspace_bytes(3, 5) == 256 and lib.ktf_gcgrad_workspace_bytes(0, 5) == 0
    for bad in ((0, 1, 0), (257, 1, 0), (8, 0, 0), (8, 1, L.GEMM_BF16), (8, 1, 7)):
        with pytest.raises(ValueError):
            ops.gcgrad_row_tile(*bad)
    assert [lib.ktf_gcgrad_workspace_bytes(-1, 4), lib.ktf_gcgrad_workspace_bytes(1, 0), lib.ktf_gcgrad_workspace_bytes(1, 257)] == [-1] * 3


CFG = {"layers": [{"type": "input", "shape": [None, None, 24]}, {"name": "t1", "type": ["tdnn", "relu"], "cfg": {"units": 32}},
                  {"name": "ctxpool", "type": "attentive_stats", "cfg": {"attention_units": 8, "heads": 4, "global_context": True}},
                  {"name": "emb", "type": "tdnn", "cfg": {"units": 6, "context": [0]}}]}


def test_trainable_sequential_takes_the_layer_only_when_asked():
    mdl = ktf.models.SequentialFromConfig(CFG)
    with pytest.raises(NotImplementedError, match="ctxpool.*global_context"):
        ktf.autograd.TrainableSequential(mdl, device="cpu")
    with pytest.raises(NotImplementedError, match="bf16"):
        ktf.autograd.TrainableSequential(mdl, device="cpu", gemm="bf16", global_context=True)
    with pytest.raises(ValueError, match="global_context"):
        ktf.autograd.TrainableSequential(mdl, device="cpu", global_context=1)
    net = ktf.autograd.TrainableSequential(mdl, device="cpu", global_context=True)
    pool = mdl.get_layer("ctxpool")
    before = [w.copy() for w in pool.get_weights()]
    assert [s[0] for s in net.steps] == ["tdnn", "relu", "gctx", "tdnn"]
    assert [tuple(p.shape) for p in net.params[2:6]] == [(96, 8), (8,), (8, 4), (4,)] == [w.shape for w in before]
    assert net.export() is mdl
    assert all(a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(pool.get_weights(), before))
    with pytest.raises(L.KtfBackendError):                   # (no CPU path behind the function either)
        ktf.autograd.global_context_attention(torch.zeros(1, 4, 32), *net.params[2:6])
