"""The squeeze-excitation gate on the GPU (include/ktf_se.h) against tests/_se_ref.py within its bounds, the bit equalities of rules 6
and 8, ktf.autograd.squeeze_excite, and the layer inside a Sequential / TrainableSequential."""

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
from kaldi_tflite_amd import ops  # noqa: E402
import _se_ref as R  # noqa: E402
import _res2_grad_ref as G  # noqa: E402
from test_loss_cpu import torch_inv_norm, torch_loss  # noqa: E402
from test_tdnn_grad_cpu import restated_pool, restated_tdnn  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 777.0


def _rows(a, lens, pad, offset, fill):
    """a (B, T, C) on the device as a (B, T, C) view of rows of stride C + pad whose base lies `offset` floats behind a 256-byte
    boundary; rows at and beyond the lengths and the pad columns hold `fill`."""
    B, T, C = a.shape
    buf = torch.full((B * T * (C + pad) + 64,), fill, dtype=torch.float32, device=DEV)
    v = buf[offset:offset + B * T * (C + pad)].view(B, T, C + pad)
    for b, n in enumerate(lens):
        v[b, :n, :C] = torch.as_tensor(a[b, :n], device=DEV)
    return v, v[:, :, :C]


def _dev(c):
    t = lambda a: None if a is None else torch.as_tensor(a, device=DEV)      # noqa: E731
    return t(c["w1"]), t(c["b1"]), t(c["w2"]), t(c["b2"])


def _run(c, var, alias=False):
    """Forward (training and inference) and backward of a case through ops -> the device outputs."""
    lens, (B, T, C), H = c["lens"], c["x"].shape, c["w1"].shape[1]
    nan = float("nan")
    w1, b1, w2, b2 = _dev(c)
    dl = torch.tensor(lens, dtype=torch.int32, device=DEV) if var["use_lens"] else None
    _, x = _rows(c["x"], lens, var["pad"], var["offset"], nan)
    _, g = _rows(c["g"], lens, var["pad"], var["offset"], nan)
    rfull, r = _rows(c["r"], lens, var["pad"], var["offset"], SENT if alias else nan) if var["residual"] else (None, None)
    new = lambda: _rows(np.zeros((B, T, C), np.float32), [0] * B, var["pad"], var["offset"], SENT)      # noqa: E731
    (yfull, y), (y2full, y2), (dxfull, dx) = ((rfull, r) if alias else new()), new(), new()
    mean, hid = (torch.empty((B, k), dtype=torch.float64, device=DEV) for k in (C, H))
    gate = torch.empty((B, C), dtype=torch.float32, device=DEV)
    if not alias:
        ops.se_gate(x, r, dl, w1, b1, w2, b2, y2, torch.empty(ops.se_gate_floats(B, C), dtype=torch.float32, device=DEV), C=C)
    ops.se_gate_train(x, r, dl, w1, b1, w2, b2, y, mean, hid, gate, C=C)
    grads = [torch.empty(s, dtype=torch.float32, device=DEV) for s in ((C, H), (H,), (H, C), (C,))]
    ops.se_gate_backward(g, x, dl, w1, w2, mean, hid, gate, dx, *grads, ops.se_gate_backward_workspace(B, C, H, DEV), C=C)
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()      # noqa: E731
    return dict(y=host(yfull), y2=host(y2full), dx=host(dxfull), mean=host(mean), hid=host(hid), gate=host(gate),
                **{k: host(v) for k, v in zip(("dw1", "db1", "dw2", "db2"), grads)})


def _reference(c, var):
    fs, bs = [], []
    for b, n in enumerate(c["lens"]):
        fs.append(R.forward(c["x"][b, :n], c["r"][b, :n] if var["residual"] else None, c["w1"], c["b1"], c["w2"], c["b2"]))
        bs.append(R.backward(c["g"][b, :n], c["x"][b, :n], c["w1"], c["w2"], fs[-1]))
    return fs, bs


@pytest.mark.parametrize("i", range(len(R.GRID)))
def test_forward_and_backward_within_the_bound(i):
    c, var = R.grid_case(i)
    lens, (B, T, C) = c["lens"], c["x"].shape
    got, again = _run(c, var), _run(c, var)
    fs, bs = _reference(c, var)
    worst = {}

    def within(name, value, want, bound):
        worst[name] = max(worst.get(name, 0.0), float((np.abs(value - want) / bound).max()) if want.size else 0.0)

    for b, n in enumerate(lens):
        f, bk = fs[b], bs[b]
        within("mean", got["mean"][b], f["mean"], f["d_mean"] + 2.0 ** -149)
        within("hid", got["hid"][b], f["hid"], f["d_hid"] + 2.0 ** -149)
        within("gate", got["gate"][b], f["gate"].astype(np.float64), f["d_gate"] + 2.0 ** -149)
        within("y", got["y"][b, :n, :C], f["y"], f["d_y"])
        within("dx", got["dx"][b, :n, :C], bk["dx"], bk["d_dx"])
        assert (got["y"][b, n:] == SENT).all() and (got["y"][b, :, C:] == SENT).all(), "rows beyond the length and pad columns of y stay"
        assert (got["dx"][b, n:, :C] == 0).all() and (got["dx"][b, :, C:] == SENT).all()
        if n == 0:
            assert not got["mean"][b].any() and not got["hid"][b].any() and not got["gate"][b].any()
    for k, (v, bound) in R.param_grads(fs, bs).items():
        if c["b1"] is not None or k not in ("db1", "db2"):
            within(k, got[k], v, bound)
    print(f"case {i} {R.GRID[i]} {var}: worst |err| / bound {worst}")
    assert max(worst.values()) <= 1.0, worst
    assert np.array_equal(got["y"], got["y2"], equal_nan=True), "the training and the inference forward give the same bits"
    assert all(np.array_equal(got[k], again[k], equal_nan=True) for k in got), "a repeated call gives the same bits"


def test_alone_and_in_a_batch_on_both_squeeze_shapes_and_y_aliasing_r():
    """B = 90 utterances of C = 516 take the wide squeeze mapping (3 x 90 >= 256 workgroups), one utterance alone the narrow one."""
    C, H, lens = 516, 17, [129, 65, 1, 0, 64] * 18
    c = R.case(C, H, lens, 130, 5)
    var = dict(residual=True, pad=0, offset=0, use_lens=True)
    full = _run(c, var)
    for b in (0, 1, 2, 89):
        one = _run({k: (v[b:b + 1] if k in ("x", "r", "g") else v) for k, v in dict(c, lens=lens[b:b + 1]).items()}, var)
        assert all(np.array_equal(one[k][0], full[k][b], equal_nan=True) for k in ("y", "gate", "dx", "mean")), b
    aliased = _run(c, var, alias=True)
    for b, n in enumerate(lens):
        assert np.array_equal(aliased["y"][b, :n], full["y"][b, :n]) and np.array_equal(aliased["y"][b, n:], np.full((130 - n, C), SENT, np.float32))


def test_autograd_function_gives_the_bits_of_the_ops_calls_and_the_half_gate():
    c = R.case(64, 17, [65, 0, 129, 2], 129, 9)
    var = dict(residual=True, pad=0, offset=0, use_lens=True)
    got = _run(c, var)
    t = lambda a: torch.tensor(a, device=DEV, requires_grad=True)      # noqa: E731
    x, r, w1, b1, w2, b2 = (t(c[k]) for k in ("x", "r", "w1", "b1", "w2", "b2"))
    lens = torch.tensor(c["lens"], dtype=torch.int32, device=DEV)
    y = ktf.autograd.squeeze_excite(x, w1, b1, w2, b2, lens, r)
    g = torch.tensor(c["g"], device=DEV)
    y.backward(g)
    for b, n in enumerate(c["lens"]):
        assert np.array_equal(y[b, :n].detach().cpu().numpy(), got["y"][b, :n]) and not y[b, n:].any()
        assert np.array_equal(x.grad[b, :n].cpu().numpy(), got["dx"][b, :n]) and not x.grad[b, n:].any()
    assert torch.equal(r.grad, g), "the residual's gradient is the arriving gradient"
    assert all(np.array_equal(p.grad.cpu().numpy(), got[k]) for p, k in ((w1, "dw1"), (b1, "db1"), (w2, "dw2"), (b2, "db2")))
    with torch.no_grad():
        half = ktf.autograd.squeeze_excite(x, w1, b1, torch.zeros_like(w2), None, None, r)
    assert torch.equal(half, x.detach() * 0.5 + r.detach()), "W2 = 0, b2 = 0: the gate is exactly 1/2"


def _restated_block(seq, params, feats, lens):
    """The model of the test below in torch ops on fp64; params in TrainableSequential's order."""
    x, it, kept = feats, iter(params), {}
    rows = torch.arange(feats.shape[1])[None, :, None] < torch.tensor(lens)[:, None, None]
    for l in seq.layers:
        if isinstance(l, ktf.layers.TDNN) and x.dim() == 3:
            x = restated_tdnn(x, next(it), next(it), lens, [0], 1, "SAME")
            x = torch.relu(x) if l.activation == "relu" else x
        elif isinstance(l, ktf.layers.TDNN):
            x = x @ next(it)[:, 0, :].T + next(it)
        elif isinstance(l, ktf.layers.Res2Conv):
            k, b = next(it).view(l.scale - 1, 3, l.width, l.width), next(it)
            ys = [G.restatement(x[i, :n], k, b, None, None, l.scale, l.dilation)[0] for i, n in enumerate(lens)]
            x = torch.stack([torch.cat([y, torch.zeros((x.shape[1] - len(y), x.shape[2]), dtype=x.dtype)]) for y in ys])
        elif isinstance(l, ktf.layers.SqueezeExcite):
            w1, b1, w2, b2 = (next(it) for _ in range(4))
            mean = torch.stack([x[i, :n].mean(0) for i, n in enumerate(lens)])
            x = (x * torch.sigmoid(torch.relu(mean @ w1 + b1) @ w2 + b2).unsqueeze(1) + kept[l.residualFrom]) * rows
        else:
            x = restated_pool(x, lens, l.includeStd, l.epsilon, l.inputPeriod)
        kept[l.name] = x
    return x


@pytest.mark.parametrize("gemm,tol", [("f32", 3e-5), ("bf16x3", 3e-4)])      # (the limits of tests/test_gpu_parity.py's Sequential tests)
def test_block_in_a_sequential_and_under_trainable_sequential_with_a_classifier_head(gemm, tol):
    """TDNN -> [TDNN, Res2Conv, TDNN, SqueezeExcite(residual_from=first)] -> StatsPooling -> TDNN. Inference through run_ragged against
    the fp64 composition within the parity limits; with an AAM ClassifierHead the first-step gradients of every parameter and of the
    input against fp64 autograd, per tensor |got - ref| <= 14 (n + 2) 2^-24 * 8 * max|ref| with n = B T rows (the bound
    tests/test_gpu_tdnn_grad.py derives); export() against the module's eval output; W2 = 0, b2 = 0 gives fl32(x / 2) + r bit for bit
    (test_autograd_function_gives_the_bits_of_the_ops_calls_and_the_half_gate)."""
    D, C, B, T, EMB, CLASSES = 24, 32, 3, 40, 8, 4
    rng = np.random.default_rng(11)
    tdnn = lambda name, units=C, **kw: ktf.layers.TDNN(units, name=name, **kw)      # noqa: E731
    layers = [tdnn("first", activation="relu"), tdnn("a", activation="relu"), ktf.layers.Res2Conv(2, dilation=2, batch_norm=False, name="res"), tdnn("b"),
              ktf.layers.SqueezeExcite(8, residual_from="first", name="se"), ktf.layers.StatsPooling(0, 10000, reduce_time_axis=True), tdnn("out", EMB)]
    mdl = ktf.models.Sequential([ktf.models.Input(shape=(None, D))] + layers, name="block")
    mdl.gemm = gemm
    se = layers[4]
    se.set_weights([a + rng.standard_normal(a.shape).astype(np.float32) * 0.3 for a in se.get_weights()])
    lens = [40, 17, 1]
    feats = rng.standard_normal((B, T, D)).astype(np.float32)
    buf = torch.zeros((B, T, 32), device=DEV)
    buf[:, :, :D] = torch.as_tensor(feats)
    dl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    assert [st[0] for st in mdl._plan()] == ["tdnn", "tdnn", "res2", "tdnn", "se", "stats", "tdnn"]

    torch.manual_seed(5)
    net = ktf.autograd.TrainableSequential(mdl, device=DEV, gemm=gemm).train()
    head = ktf.autograd.ClassifierHead(EMB, CLASSES, kind="aam", margin=0.2, scale=16.0, gemm=gemm, device=DEV)
    tf_ = torch.tensor(feats, device=DEV, requires_grad=True)
    labels = torch.arange(B) % CLASSES
    params = [tf_] + list(net.params) + [head.weight]
    ref = [p.detach().cpu().to(torch.float64).requires_grad_(True) for p in params]
    with torch.no_grad():
        want = _restated_block(mdl, ref[1:-1], ref[0], lens).numpy()
    got = mdl.run_ragged(buf[:, :, :D], dl).cpu().numpy()[:, 0]
    print(f"{gemm} inference: max |err| {np.abs(got - want).max():.3e}, limit {tol * max(1.0, np.abs(want).max()):.3e}")
    assert np.abs(got - want).max() < tol * max(1.0, np.abs(want).max())

    loss, _ = head(net(tf_, dl), labels.to(DEV))
    loss.backward()
    emb = _restated_block(mdl, ref[1:-1], ref[0], lens)
    ref_loss = torch_loss(emb @ ref[-1].T, labels, torch_inv_norm(emb, 1e-12), torch_inv_norm(ref[-1], 1e-12), "aam", 0.2, 16.0).mean()
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
    factor = 14 * (B * T + 2) * 2.0 ** -24 * 8
    worst = []
    for i, (p, r) in enumerate(zip(params, ref)):
        err, top = float((p.grad.cpu().to(torch.float64) - r.grad).abs().max()), float(r.grad.abs().max())
        print(f"{gemm} tensor {i} {tuple(p.shape)}: max |err| {err:.3e}, max |ref| {top:.3e}, bound {factor * top:.3e}")
        worst.append((err, factor * top, i))
    assert all(top > 0 for _, top, _ in worst)
    for err, bound, i in worst:
        assert err <= bound, (gemm, i, err, bound)

    with torch.no_grad():
        for p in net.params:
            p -= 0.01 * p.grad
        stepped = net.eval()(tf_.detach(), dl).cpu().numpy()
    assert net.export() is mdl and all(np.array_equal(w, net.params[net.steps[4][2] + k].detach().cpu().numpy()) for k, w in enumerate(se.get_weights()))
    again = mdl.run_ragged(buf[:, :, :D], dl).cpu().numpy()[:, 0]
    print(f"{gemm} export: max |inference - eval| {np.abs(again - stepped).max():.3e}")
    assert np.abs(again - stepped).max() < tol * max(1.0, np.abs(stepped).max()) and np.abs(again - got).max() > 0
