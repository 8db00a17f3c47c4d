"""The Res2Net backward without a GPU: tests/_res2_grad_ref.py against fp64 torch.autograd of the conv1d restatement, every new
refusal of include/ktf_res2.h rule 13 through ops, the slot rule, TrainableSequential with a Res2Conv on device="cpu", and the
small Res2Net x-vector model of tests/test_gpu_res2_grad.py with the condition on its seeded inputs: no ReLU input so close to zero
that a tested mode could flip its sign."""

import contextlib
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
import _res2_ref as R  # noqa: E402
import _res2_grad_ref as G  # noqa: E402

# the model of the GPU test: small enough that a seed exists at which all of its 2080 ReLU inputs keep the margin below
MODEL_LENS, MODEL_FEAT, MODEL_EMB, MODEL_CLASSES, MODEL_SEED = [12, 5, 9], 8, 16, 4, 3


def model():
    Lr, M = ktf.layers, ktf.models
    return M.Sequential([M.Input(shape=(None, MODEL_FEAT)), Lr.TDNN(48, [-1, 0, 1], name="t1"), Lr.ReLU(name="r1"), Lr.BatchNorm(name="b1"),
                         Lr.Res2Conv(3, dilation=2, name="res"), Lr.BatchNorm(name="b2"), Lr.StatsPooling(0, 0, reduce_time_axis=True, name="stats"),
                         Lr.TDNN(MODEL_EMB, [0], name="emb")], name="res2_xvector")


def model_inputs():
    rng = np.random.default_rng(MODEL_SEED)
    feats = rng.standard_normal((len(MODEL_LENS), max(MODEL_LENS), MODEL_FEAT)).astype(np.float32)
    return feats, np.arange(len(MODEL_LENS)) % MODEL_CLASSES


@pytest.mark.parametrize("w,s,d,n,relu,bn", [(16, 3, 2, 9, True, True), (32, 4, 3, 2, False, True), (16, 8, 8, 5, True, False),
                                             (48, 2, 1, 1, True, True), (16, 4, 3, 1, False, False), (16, 3, 4, 40, True, True)])
def test_reference_is_autograd_of_the_restatement(w, s, d, n, relu, bn):
    rng = np.random.default_rng(w + s + d + n)
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)      # noqa: E731
    x, W = t(rng.standard_normal((n, s * w))), t(rng.standard_normal((s - 1, 3, w, w)) / np.sqrt(3 * w))
    bias, nsc, nsh = (t(rng.standard_normal((s - 1, w))) for _ in range(3))
    g = rng.standard_normal((n, s * w))
    y, a = G.restatement(x, W, bias, nsc if bn else None, nsh if bn else None, s, d, relu)
    (y * torch.tensor(g)).sum().backward()
    got, _ = G.grad(x.detach().numpy(), y.detach().numpy(), a.detach().numpy() if bn else None, g, s, d, W.detach().numpy(),
                    nsc.detach().numpy() if bn else None, relu)
    want = dict(dx=x.grad, dW=W.grad, dbias=bias.grad, **(dict(dnscale=nsc.grad, dnshift=nsh.grad) if bn else {}))
    for k, v in want.items():
        assert np.abs(got[k] - v.numpy()).max() <= 1e-12, k


def test_every_new_refusal_through_ops_and_the_slot_rule(monkeypatch):
    monkeypatch.setattr(L, "stream_ptr", lambda: None)       # host pointers and a null stream: every refusal comes before any launch
    monkeypatch.setattr(L, "on_device", lambda device: contextlib.nullcontext())
    s, w, B, T = 4, 16, 2, 5
    C_, Ca = s * w, (s - 1) * w
    z = lambda *shape: torch.zeros(*shape)      # noqa: E731
    par = lambda: z(s - 1, w)      # noqa: E731

    def train(**kw):
        a = dict(x=z(B, T, C_), y=z(B, T, C_), a=z(B, T, Ca), nscale=par(), nshift=par())
        a.update(kw)
        return ops.res2_conv_train(a["x"], None, s, 1, z(s - 1, 3 * w, w), par(), a["nscale"], a["nshift"], L.ACT_RELU, L.GEMM_F32, a["y"], a["a"], C=C_)

    def data(**kw):
        a = dict(g=z(B, T, C_), y=z(B, T, C_), a=z(B, T, Ca), dx=z(B, T, C_), gt=z(B, T, Ca), nscale=par(), d=1, gemm=L.GEMM_F32)
        a.update(kw)
        return ops.res2_grad_data(a["g"], None, s, a["d"], z(s - 1, 3 * w, w), a["nscale"], a["y"], a["a"], L.ACT_RELU, a["gemm"], a["dx"], a["gt"],
                                  C=C_)

    def weights(**kw):
        a = dict(x=z(B, T, C_), y=z(B, T, C_), a=z(B, T, Ca), gt=z(B, T, Ca), nscale=par(), dw=z(s - 1, 3 * w, w), dnscale=par(),
                 scratch=ops.res2_grad_scratch(B, T, w, s, "cpu"))
        a.update(kw)
        return ops.res2_grad_weights(a["x"], None, s, 1, a["nscale"], a["y"], a["a"], a["gt"], L.ACT_RELU, L.GEMM_F32, a["dw"], par(), a["dnscale"],
                                     par() if a["nscale"] is not None else None, a["scratch"], C=C_)

    both = z(8192)
    over = lambda k, n: both[k * 8:k * 8 + B * T * n].view(B, T, n)      # noqa: E731
    for fn, kw, what in ((train, dict(a=None), "missing or misplaced"), (train, dict(nscale=None, nshift=None), "missing or misplaced"),
                         (train, dict(a=z(B, T, Ca - 4)), "lda"), (train, dict(a=z(B, T, Ca + 2)[:, :, :Ca]), "lda"),
                         (train, dict(x=over(0, C_), a=over(1, Ca)), "overlaps"),
                         (data, dict(a=None), "missing or misplaced"), (data, dict(nscale=None), "missing or misplaced"), (data, dict(d=9), "dilation"),
                         (data, dict(gemm=7), "gemm"), (data, dict(g=z(B, T, C_ - 4)), "ldg"), (data, dict(dx=z(B, T, C_ + 2)[:, :, :C_]), "lddx"),
                         (data, dict(gt=z(B, T, Ca - 4)), "ldgt"), (data, dict(g=over(0, C_), dx=over(1, C_)), "overlaps"),
                         (data, dict(y=over(0, C_), gt=over(1, Ca)), "overlaps"),
                         (weights, dict(a=None), "missing or misplaced"), (weights, dict(nscale=None, a=None), "without nscale"),
                         (weights, dict(x=z(B, T, C_ - 4)), "ldx"), (weights, dict(scratch=z(8)), "scratch"),
                         (weights, dict(x=over(0, C_), scratch=both[8:]), "overlaps")):
        with pytest.raises(ValueError, match=what):
            fn(**kw)
    assert ops.res2_grad_row_tile(64, 8, 4) == 128 and ops.res2_grad_row_tile(128, 8, 4, L.GEMM_BF16X3) == 96 and ops.res2_grad_row_tile(128, 8, 8) == 32
    assert [ops.res2_grad_slots(1, T_, 64, 8) for T_ in (1, 32, 33, 64, 65)] == [1, 1, 2, 2, 3]
    assert ops.res2_grad_slots(512, 300, 64, 8) == 37 and ops.res2_grad_slots(512, 300, 128, 2) == 64 and ops.res2_grad_slots(4, 300, 64, 8) == 37
    assert ops.res2_grad_scratch(512, 300, 128, 8, "cpu").numel() == 37 * 7 * 3 * 128 * 129
    for bad in ((-1, 5, 64, 4), (2, 5, 8, 4), (2, 5, 64, 9)):
        with pytest.raises(ValueError):
            ops.res2_grad_slots(*bad)


def test_trainable_sequential_takes_a_res2conv_in_front_of_the_pooling():
    Lr, M = ktf.layers, ktf.models
    for bn in (True, False):
        res = Lr.Res2Conv(4, dilation=2, batch_norm=bn, name="res")
        seq = M.Sequential([M.Input(shape=(None, 24)), Lr.TDNN(64, [-1, 0, 1], name="t1"), Lr.ReLU(name="r1"), Lr.BatchNorm(name="b1"), res,
                            Lr.BatchNorm(name="b2"), Lr.StatsPooling(0, 0, reduce_time_axis=True, name="stats"), Lr.TDNN(8, [0], name="emb")])
        net = ktf.autograd.TrainableSequential(seq, device="cpu")
        assert [st[0] for st in net.steps] == ["tdnn", "relu", "bn", "res2", "bn", "stats", "tdnn"]
        at = [st[2] for st in net.steps if st[0] == "res2"][0]
        assert [tuple(p.shape) for p in net.params[at:at + (4 if bn else 2)]] == [(3, 48, 16), (3, 16)] + ([(3, 16), (3, 16)] if bn else [])
        with torch.no_grad():
            for k in range(4 if bn else 2):
                net.params[at + k].add_(float(k + 1))
        before, version = [np.array(a) for a in res.get_weights()], res._version
        assert net.export() is seq and res._version > version
        for k, (was, now) in enumerate(zip(before, res.get_weights())):
            assert now.shape == was.shape and np.array_equal(now, was + np.float32(k + 1))
    behind = M.Sequential([M.Input(shape=(None, 64)), Lr.StatsPooling(0, 0, reduce_time_axis=True, name="stats"), Lr.Res2Conv(4, name="late")])
    behind.layers[-1].build((None, None, 128))
    with pytest.raises(NotImplementedError, match="late"):
        ktf.autograd.TrainableSequential(behind, device="cpu")
    with pytest.raises(L.KtfBackendError):
        ktf.autograd.res2_conv(torch.zeros(1, 4, 64), torch.zeros(3, 48, 16), None, None, None, 4, 1)


def test_relu_inputs_of_the_gpu_model_test_keep_their_sign_in_every_mode():
    """|Z| >= 2^-12 sum|terms| in fp64 for every input of the TDNN's ReLU and of the Res2Conv's: a condition on MODEL_SEED."""
    seq = model()
    feats, _ = model_inputs()
    t1, bn1, res = seq.layers[0], seq.layers[2], seq.layers[3]
    W, bias = np.asarray(t1.kernel[0], np.float64), np.asarray(t1.bias, np.float64)          # (K, D, units)
    margins, hidden = [], []
    for b, n in enumerate(MODEL_LENS):
        X = feats[b, :n].astype(np.float64)[np.clip(np.arange(n)[:, None] + np.asarray(t1.context)[None, :], 0, n - 1)]
        Z = np.einsum("nkd,kdu->nu", X, W) + bias
        margins.append(np.abs(Z) / (np.einsum("nkd,kdu->nu", np.abs(X), np.abs(W)) + np.abs(bias)))
        hidden.append(np.maximum(Z, 0.0))
    rows = np.concatenate(hidden)
    mean, var = rows.mean(0), rows.var(0)
    for h in hidden:
        trace = []
        R.conv(np.asarray(bn1.gamma, np.float64) * (h - mean) / np.sqrt(var + bn1.epsilon), res.scale, res.dilation, *res.get_weights(), trace=trace)
        margins += [np.abs(st["Z"]) / st["bound"] for st in trace]
    worst = min(float(m.min()) for m in margins)
    print(f"{sum(m.size for m in margins)} ReLU inputs, smallest |Z| / sum|terms| = {worst:.3e} (2^-12 = {2.0 ** -12:.3e})")
    assert worst >= 2.0 ** -12
