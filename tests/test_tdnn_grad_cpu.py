"""The TDNN / pooling gradients without a GPU: the fp64 oracle (tests/_tdnn_grad_ref.py) against torch.autograd on an fp64 CPU
restatement (index gather followed by a matmul), the C-ABI of include/ktf_grad.h (symbols, argument refusals before any launch,
the workspace size) and the parts of ktf.autograd that are pure torch (batch normalisation, output lengths, the construction
checks of TrainableSequential)."""

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
from kaldi_tflite_amd import _lib as L, autograd as A  # noqa: E402
import _tdnn_grad_ref as R  # noqa: E402

CASES = R.cases()
F64 = torch.float64


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ----------------------------------------------------------------------------- the oracle
def restated_tdnn(x, W, bias, lens, context, sub, padding):
    """z (B, T_out, units) in torch: per utterance an index gather (T_out, nctx) -> rows, then one matmul."""
    B, Tm, D = x.shape
    valid = padding == "VALID"
    rows = []
    for b in range(B):
        n = int(lens[b])
        ol, start = R.out_len(n, context, sub, valid)
        z = torch.zeros((R.out_len(Tm, context, sub, valid)[0], W.shape[0]), dtype=x.dtype)
        if ol > 0:
            idx = (start + torch.arange(ol)[:, None] * sub + torch.tensor(context)[None, :]).clamp(0, n - 1)
            z[:ol] = x[b][idx].reshape(ol, -1) @ W.reshape(W.shape[0], -1).T + (0 if bias is None else bias)
        rows.append(z)
    return torch.stack(rows)


def restated_pool(x, lens, include_std, eps, period):
    out = []
    for b in range(x.shape[0]):
        rows = x[b, 0:int(lens[b]):period]
        mean = rows.mean(0)
        cols = [mean]
        if include_std:
            cols.append(torch.sqrt(torch.relu((rows * rows).mean(0) - mean * mean) + eps))
        out.append(torch.cat(cols))
    return torch.stack(out)


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_oracle_equals_autograd_of_the_restatement(c):
    rng = np.random.default_rng(11)
    lens = R.lens_for(c, 512)
    B, Tm = len(lens), R.T
    Tout = R.out_len(Tm, c["context"], c["sub"], c["padding"] == "VALID")[0]
    x = rng.standard_normal((B, Tm, c["din"]))
    W = rng.standard_normal((c["units"], len(c["context"]), c["din"]))
    bias = rng.standard_normal(c["units"])
    g = rng.standard_normal((B, Tout, c["units"]))
    want = R.tdnn_grads(x, W, g, lens, c["context"], c["sub"], c["padding"])
    tx, tW, tb = (torch.tensor(a, dtype=F64, requires_grad=True) for a in (x, W, bias))
    z = restated_tdnn(tx, tW, tb, lens, c["context"], c["sub"], c["padding"])
    assert _rel(R.tdnn_forward(x, W, bias, lens, c["context"], c["sub"], c["padding"]), z.detach().numpy()) <= 1e-12
    (z * torch.tensor(g)).sum().backward()
    assert _rel(want["dx"], tx.grad.numpy()) <= 1e-12
    assert _rel(want["dW"], tW.grad.numpy()) <= 1e-12
    assert _rel(want["db"], tb.grad.numpy()) <= 1e-12
    # the counts: every valid output row sends nctx rows of `units` terms into dx and one term into every element of dW / db
    rows = sum(R.out_len(n, c["context"], c["sub"], c["padding"] == "VALID")[0] for n in lens)
    assert want["dx_n"].sum() == rows * len(c["context"]) * c["units"] * c["din"]
    assert (want["dW_n"] == rows).all() and (want["db_n"] == rows).all()
    assert (want["dx_S"] >= np.abs(want["dx"]) - 1e-9).all() and (want["dW_S"] >= np.abs(want["dW"]) - 1e-9).all()
    for b, n in enumerate(lens):
        assert not want["dx"][b, n:].any()


@pytest.mark.parametrize("include_std,period", [(True, 1), (True, 3), (False, 2)])
def test_pooling_oracle_equals_autograd_of_the_restatement(include_std, period):
    rng = np.random.default_rng(5)
    lens = [1, 7, 50, 33]
    x = rng.standard_normal((4, 50, 9)) + 0.5
    x[:, :, 4] = 1.5                                           # a constant column: the relu clips, the std term has no gradient
    gout = rng.standard_normal((4, 18 if include_std else 9))
    tx = torch.tensor(x, dtype=F64, requires_grad=True)
    y = restated_pool(tx, lens, include_std, 1e-10, period)
    assert _rel(R.pool_forward(x, lens, include_std, 1e-10, period), y.detach().numpy()) <= 1e-12
    (y * torch.tensor(gout)).sum().backward()
    dx, M = R.pool_grad(x, lens, gout, include_std, 1e-10, period)
    assert _rel(dx, tx.grad.numpy()) <= 1e-12
    assert (M >= np.abs(dx) - 1e-12).all()
    assert np.allclose(dx[2, 0:50:period, 4], gout[2, 4] / len(range(0, 50, period)), rtol=1e-14)      # the mean term only
    skipped = np.ones(50, bool)
    skipped[0::period] = False
    assert not dx[:, skipped].any()                            # rows the pooling does not sample


# ----------------------------------------------------------------------------- the C-ABI
def test_header_symbols_are_the_grad_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_grad.h")).read()
    declared = set(re.findall(r"\b(ktf_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.GRAD_PROTOTYPES), declared ^ set(L.GRAD_PROTOTYPES)
    assert all(n.startswith("ktf_grad_") for n in declared)
    lib = L.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert not set(L.GRAD_PROTOTYPES) & (set(L.PROTOTYPES) | set(L.AUGMENT_PROTOTYPES) | set(L.RESAMPLE_PROTOTYPES))
    for other in ("ktf_hip.h", "ktf_augment.h", "ktf_resample.h"):
        assert "ktf_grad_" not in open(os.path.join(ROOT, "include", other)).read()
    assert len(L.PROTOTYPES) == 120 and lib.ktf_version() == 117
    assert lib.ktf_grad_tdnn_row_tile() == 64 and lib.ktf_grad_tdnn_slot_rows() == 512


def _desc(units=40, din=23, context=(-1, 2), sub=1, padding="SAME"):
    return A._desc(units, din, list(context), sub, padding)


def _refused(rc, text):
    assert rc == -1, rc
    assert text in L.last_error(), L.last_error()
    with pytest.raises(ValueError):
        L.check(rc, "x")


def test_argument_checks_without_gpu():
    lib = L.load()
    raw = (C.c_float * 4096)()
    buf = C.c_void_p((C.addressof(raw) + 255) & ~255)      # stands for any aligned non-null device pointer: every refusal comes before a launch
    odd = C.c_void_p(buf.value + 4)
    B, Tm = 2, 10
    good = _desc()
    need = lib.ktf_grad_tdnn_workspace_bytes(B, Tm, C.byref(good))
    assert need > 0

    def data(g=buf, ldg=40, B=B, T=Tm, d=good, w=buf, dx=buf, ldx=32, ws=buf, ws_bytes=None):
        return lib.ktf_grad_tdnn_data(g, ldg, B, T, None, None if d is None else C.byref(d), w, dx, ldx, ws, need if ws_bytes is None else ws_bytes,
                                      None)

    def weights(x=buf, B=B, T=Tm, ldx=32, d=good, g=buf, ldg=40, dw=buf, dbias=buf, ws=buf, ws_bytes=None):
        return lib.ktf_grad_tdnn_weights(x, B, T, ldx, None, None if d is None else C.byref(d), g, ldg, dw, dbias, ws,
                                         need if ws_bytes is None else ws_bytes, None)

    def size(d):
        return lib.ktf_grad_tdnn_workspace_bytes(B, Tm, None if d is None else C.byref(d))

    def changed(**kw):
        d = _desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    unsorted = _desc()
    unsorted.ctx[0], unsorted.ctx[1] = 2, -1
    for fn in (data, weights, size):
        call = (lambda d, fn=fn: fn(d)) if fn is size else (lambda d, fn=fn: fn(d=d))
        _refused(call(None), "null")
        _refused(call(changed(gemm=L.GEMM_BF16X3)), "KTF_GEMM_F32")
        _refused(call(changed(gemm=L.GEMM_F16MX)), "KTF_GEMM_F32")
        _refused(call(changed(act=L.ACT_RELU)), "KTF_ACT_NONE")
        _refused(call(changed(x_dtype=L.KTF_BF16)), "KTF_F32")
        _refused(call(unsorted), "ascending")
        _refused(call(changed(nctx=17)), "nctx")
        _refused(call(changed(din_pad=24)), "din_pad")
        _refused(call(changed(subsampling=0)), "subsampling")
    for fn, ptrs in ((data, ("g", "w", "dx", "ws")), (weights, ("x", "g", "dw", "ws"))):
        for name in ptrs:
            _refused(fn(**{name: None}), "null")
        _refused(fn(ldx=31), "din_pad")
        _refused(fn(ldx=34), "multiple of 4")
        _refused(fn(ldg=39), "units")
        _refused(fn(ws_bytes=need - 1), "workspace")
        _refused(fn(ws=odd), "256-byte")
        _refused(fn(B=-1), "negative size")
        _refused(fn(B=65536), "65535")
        _refused(fn(B=60000, T=1 << 20), "2^31")
    _refused(data(w=odd), "16-byte")
    _refused(data(dx=odd), "16-byte")
    _refused(weights(x=odd), "16-byte")
    _refused(weights(dw=odd), "16-byte")

    def pool(x=buf, B=2, T=10, D=8, ldx=8, period=1, std=1, gout=buf, ldg=16, dx=buf, ld_dx=8):
        return lib.ktf_grad_stats_pool(x, B, T, D, ldx, None, period, std, 1e-10, gout, ldg, dx, ld_dx, None)

    _refused(pool(x=None), "null")
    _refused(pool(gout=None), "null")
    _refused(pool(dx=None), "null")
    _refused(pool(D=0), "bad sizes")
    _refused(pool(ldx=7), "bad sizes")
    _refused(pool(ld_dx=7), "bad sizes")
    _refused(pool(period=0), "input_period")
    _refused(pool(ldg=15), "ld_gout")
    _refused(pool(B=65536), "65535")
    assert pool(std=0, ldg=8, T=0) == 0                        # no row: nothing to launch


def test_workspace_size_is_monotone_and_never_zero():
    lib = L.load()
    d = _desc(units=130, din=30, context=(-2, -1, 0, 1, 2))
    size = lambda B, T: lib.ktf_grad_tdnn_workspace_bytes(B, T, C.byref(d))  # noqa: E731
    assert size(0, 0) > 0 and size(1, 0) > 0 and size(0, 5) > 0
    rows = [(1, 1), (1, 511), (1, 512), (1, 513), (2, 512), (3, 700), (8, 1000), (64, 300)]
    sizes = [size(B, T) for B, T in sorted(rows, key=lambda bt: bt[0] * bt[1])]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1], sizes
    # one slot of (units_pad, nctx * din_pad) + units_pad floats per 512 flat rows
    assert size(1, 513) - size(1, 512) >= (256 * 5 * 32 + 256) * 4
    v = _desc(units=130, din=30, context=(-3, 0, 3), sub=3, padding="VALID")
    assert lib.ktf_grad_tdnn_workspace_bytes(4, 6, C.byref(v)) > 0          # no output row at all


# ----------------------------------------------------------------------------- ktf.autograd, the pure-torch parts
def test_tdnn_out_lens_is_the_library_rule():
    lib = L.load()
    lens = torch.tensor(R.LENS, dtype=torch.int32)
    for c in CASES:
        d = _desc(c["units"], c["din"], c["context"], c["sub"], c["padding"])
        want = [lib.ktf_tdnn_out_len(int(n), C.byref(d)) for n in R.LENS]
        assert A.tdnn_out_lens(lens, c["context"], c["sub"], c["padding"]).tolist() == want
        assert want == [R.out_len(n, c["context"], c["sub"], c["padding"] == "VALID")[0] for n in R.LENS]
    assert A.tdnn_out_lens(None, [0]) is None


def test_batch_norm_training_formulas_on_cpu():
    rng = np.random.default_rng(3)
    B, Tm, D = 4, 12, 6
    lens = torch.tensor([12, 0, 5, 9], dtype=torch.int32)
    x = torch.tensor(rng.standard_normal((B, Tm, D)), dtype=F64)
    x[0, :, 0] += 3.0
    bad = x.clone()
    for b, n in enumerate(lens.tolist()):
        bad[b, n:] = float("nan")                             # invalid rows are not read
    gamma = torch.tensor(rng.uniform(0.5, 2.0, D), dtype=F64, requires_grad=True)
    mm, mv = torch.zeros(D, dtype=F64), torch.ones(D, dtype=F64)
    xin = bad.clone().requires_grad_(True)
    y = A.batch_norm(xin, lens, mm, mv, gamma, momentum=0.9, epsilon=1e-3, training=True)
    valid = torch.cat([x[b, :n] for b, n in enumerate(lens.tolist())])
    mean, var = valid.mean(0), valid.var(0, unbiased=False)
    for b, n in enumerate(lens.tolist()):
        want = gamma.detach() * (x[b, :n] - mean) / torch.sqrt(var + 1e-3)
        assert torch.allclose(y[b, :n].detach(), want, rtol=1e-12, atol=1e-12)
        assert not y[b, n:].detach().any()
    assert torch.allclose(mm, 0.1 * mean, rtol=1e-12) and torch.allclose(mv, 0.9 + 0.1 * var, rtol=1e-12)
    # gradients against autograd of the textbook form on the packed valid rows
    w = torch.tensor(rng.standard_normal((B, Tm, D)), dtype=F64)
    (torch.nan_to_num(y) * w).sum().backward()
    packed = valid.clone().requires_grad_(True)
    g2 = gamma.detach().clone().requires_grad_(True)
    y2 = g2 * (packed - packed.mean(0)) / torch.sqrt(packed.var(0, unbiased=False) + 1e-3)
    (y2 * torch.cat([w[b, :n] for b, n in enumerate(lens.tolist())])).sum().backward()
    got = torch.cat([xin.grad[b, :n] for b, n in enumerate(lens.tolist())])
    assert torch.allclose(got, packed.grad, rtol=1e-10, atol=1e-12) and torch.allclose(gamma.grad, g2.grad, rtol=1e-10)
    for b, n in enumerate(lens.tolist()):
        assert not xin.grad[b, n:].any()
    # evaluation: the moving statistics, which stay as they are; a 2-D input without lengths
    before = (mm.clone(), mv.clone())
    z = A.batch_norm(x, lens, mm, mv, gamma.detach(), training=False, epsilon=1e-3)
    assert torch.equal(mm, before[0]) and torch.equal(mv, before[1])
    assert torch.allclose(z[0], gamma.detach() * (x[0] - mm) / torch.sqrt(mv + 1e-3), rtol=1e-12)
    p = torch.tensor(rng.standard_normal((7, D)), dtype=F64)
    m2, v2 = torch.zeros(D, dtype=F64), torch.ones(D, dtype=F64)
    y3 = A.batch_norm(p, None, m2, v2, gamma.detach(), momentum=0.5, epsilon=1e-3, training=True)
    assert torch.allclose(y3, gamma.detach() * (p - p.mean(0)) / torch.sqrt(p.var(0, unbiased=False) + 1e-3), rtol=1e-12)
    assert torch.allclose(m2, 0.5 * p.mean(0), rtol=1e-12)


def test_kernels_refuse_cpu_tensors():
    x = torch.zeros((1, 4, 8))
    with pytest.raises(ktf.KtfBackendError):
        A.tdnn_affine(x, torch.zeros((3, 1, 8)), None, [0])
    with pytest.raises(ktf.KtfBackendError):
        A.stats_pooling(x)
    with pytest.raises(NotImplementedError):
        ktf.layers.BatchNorm().call(torch.zeros((1, 4, 8)), training=True)       # the inference layer keeps refusing: training is ktf.autograd


def test_trainable_sequential_names_the_layer_it_cannot_differentiate():
    Lr, M = ktf.layers, ktf.models
    cpu = torch.device("cpu")
    ok = M.Sequential([M.Input(shape=(None, 24)), Lr.TDNN(16, [-1, 0, 1], name="t1"), Lr.ReLU(), Lr.BatchNorm(name="b1"),
                       Lr.StatsPooling(0, 0, reduce_time_axis=True, name="pool"), Lr.TDNN(8, [0], name="t2")])
    net = A.TrainableSequential(ok, device=cpu)
    assert [tuple(p.shape) for p in net.parameters()] == [(16, 3, 24), (16,), (16,), (8, 1, 32), (8,)]
    assert torch.equal(net.params[0].detach(), torch.tensor(ok.layers[0].kernel[0].transpose(2, 0, 1)))
    for bad, name in ((Lr.TDNN(16, [0], activation="tanh", name="squash"), "squash"), (Lr.CMVN(name="cm"), "cm"),
                      (Lr.StatsPooling(-2, 2, name="windows"), "windows")):
        with pytest.raises(NotImplementedError, match=name):
            A.TrainableSequential(M.Sequential([M.Input(shape=(None, 24)), Lr.TDNN(16, [0], name="t1"), bad]), device=cpu)
    with pytest.raises(NotImplementedError, match="wide"):
        A.TrainableSequential(M.Sequential([M.Input(shape=(None, 24)), Lr.StatsPooling(0, 0, reduce_time_axis=True),
                                            Lr.TDNN(16, [-1, 1], name="wide")]), device=cpu)
    with pytest.raises(ValueError, match="not built"):
        A.TrainableSequential(M.Sequential([Lr.TDNN(16, [0], name="t1")]), device=cpu)
