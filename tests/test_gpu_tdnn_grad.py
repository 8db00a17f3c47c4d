"""The TDNN / pooling gradient kernels (csrc/tdnn_grad.hip, include/ktf_grad.h) and ktf.autograd on the GPU, against the fp64 oracle of
tests/_tdnn_grad_ref.py.

Tile sizes the lengths are chosen around: the data gradient works on 64 input rows x 128 features per workgroup
(ktf_grad_tdnn_row_tile() = 64), the weight gradient on 128 units x 128 features reduced in steps of 16 rows, one partial sum per
512 flat rows b * T_out + t (ktf_grad_tdnn_slot_rows() = 512). Every batch holds the lengths 0, 1, 3 (shorter than the span of
every multi-offset context), 15 / 16 / 17, 63 / 64 / 65, 129 / 130 and some in between, rotated per case so that one utterance's
rows lie in two slots (_tdnn_grad_ref.lens_for). The cases are every context x padding x subsampling with the (din, units) pairs dealt
round, so that each of the nine pairs occurs.

Bounds. Exact test: integers in [-4, 4] and [-2, 2], every sum of magnitudes below 2^24 (asserted): fp32 is exact in any order,
the results must EQUAL the oracle. Rounding test: |got - ref64| <= (n + 2) 2^-24 S per element (n terms of magnitudes summing to S:
an fp32 dot product in any order, plus one rounding). The network test states its own."""

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
from kaldi_tflite_amd import autograd as A, ops  # noqa: E402
import _tdnn_grad_ref as R  # noqa: E402
from test_tdnn_grad_cpu import restated_pool, restated_tdnn  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = R.cases()
U = 2.0 ** -24
DEV = "cuda:0"
NAN = float("nan")


def _tout(c):
    return R.out_len(R.T, c["context"], c["sub"], c["padding"] == "VALID")[0]


def _inputs(c, rng, integers):
    lens = R.lens_for(c, ops.grad_tdnn_slot_rows())
    shapes = ((len(lens), R.T, c["din"]), (c["units"], len(c["context"]), c["din"]), (len(lens), _tout(c), c["units"]))
    if integers:
        x, W, g = (rng.integers(-m, m + 1, s).astype(np.float32) for m, s in zip((4, 2, 4), shapes))
    else:
        x, W, g = (rng.standard_normal(s).astype(np.float32) for s in shapes)
    return lens, x, W, g


def run_kernels(c, lens, x, W, g, ldx_extra=0, ldg_extra=0, poison=False):
    """The two C-ABI calls on padded operands -> (dx (B, T, din), dW (units, nctx, din), db) as numpy, after checking that every
    element of the padded outputs was written and that the pad regions hold zero. `poison`: NaN in every row of x and g that is
    not valid (columns that are never read hold NaN always)."""
    B, Tm, D = x.shape
    units, nctx, _ = W.shape
    d = A._desc(units, D, c["context"], c["sub"], c["padding"])
    Dp, Up, Tout = d.din_pad, ops.round_up(units, 256), g.shape[1]
    ldx, ldg = Dp + ldx_extra, units + ldg_extra
    valid = c["padding"] == "VALID"
    xp = np.full((B, Tm, ldx), NAN, np.float32)
    xp[:, :, :Dp] = 0.0
    xp[:, :, :D] = x
    gp = np.full((B, Tout, ldg), NAN, np.float32)
    gp[:, :, :units] = g
    if poison:
        for b, n in enumerate(lens):
            xp[b, n:] = NAN
            gp[b, R.out_len(n, c["context"], c["sub"], valid)[0]:] = NAN
    wp = np.zeros((Up, nctx, Dp), np.float32)
    wp[:units, :, :D] = W
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    xp, gp, wp, tl = t(xp), t(gp), t(wp).view(Up, nctx * Dp), t(np.asarray(lens, np.int32))
    ws = ops.grad_tdnn_workspace(B, Tm, d, xp.device)
    ws.fill_(0xFF)                                              # NaN patterns: a slot that is read before it is written shows
    dxp = torch.full((B, Tm, ldx), NAN, device=DEV)
    dwp = torch.full((Up, nctx * Dp), NAN, device=DEV)
    db = torch.full((units,), NAN, device=DEV)
    ops.grad_tdnn_data(gp, tl, d, wp, dxp, ws)
    ops.grad_tdnn_weights(xp, tl, d, gp, dwp, db, ws)
    dxp, dwp, db = dxp.cpu().numpy(), dwp.cpu().numpy().reshape(Up, nctx, Dp), db.cpu().numpy()
    assert not np.isnan(dxp).any() and not np.isnan(dwp).any() and not np.isnan(db).any()
    assert not dxp[:, :, D:].any() and not dwp[units:].any() and not dwp[:, :, D:].any()
    for b, n in enumerate(lens):
        assert not dxp[b, n:].any()
    return dxp[:, :, :D], dwp[:units, :, :D], db


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ----------------------------------------------------------------------------- the GEMM gradients
@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_exact_integers(c):
    lens, x, W, g = _inputs(c, np.random.default_rng(101), integers=True)
    want = R.tdnn_grads(x, W, g, lens, c["context"], c["sub"], c["padding"])
    assert max(np.abs(want[k + "_S"]).max() for k in ("dx", "dW", "db")) < 2 ** 24
    dx, dW, db = run_kernels(c, lens, x, W, g, ldx_extra=4 * (c["sub"] == 3), ldg_extra=3 * (c["padding"] == "VALID"))
    for name, got in (("dx", dx), ("dW", dW), ("db", db)):
        bad = np.argwhere(got != want[name].astype(np.float32))
        assert len(bad) == 0, (name, len(bad), bad[:5].tolist())


# up to 5 * 256 (+ the folded rows' 3 * 256 at the edges) terms per element of dx, the batch's ~740 valid rows per element of dW / db
ROUNDING = [dict(context=[-2, -1, 0, 1, 2], padding="SAME", sub=1, din=64, units=256),
            dict(context=[-3, 0, 3], padding="VALID", sub=3, din=30, units=130),
            dict(context=[-1, 2], padding="SAME", sub=3, din=23, units=256)]


@pytest.mark.parametrize("c", ROUNDING, ids=R.case_id)
def test_rounding_bound_determinism_and_invalid_rows(c):
    lens, x, W, g = _inputs(c, np.random.default_rng(202), integers=False)
    want = R.tdnn_grads(x, W, g, lens, c["context"], c["sub"], c["padding"])
    assert want["dx_n"].max() <= 2600 and want["dW_n"].max() <= 2000       # "about 2000" terms: the edge rows of dx take the folded ones too
    first = run_kernels(c, lens, x, W, g)
    for name, got in zip(("dx", "dW", "db"), first):
        err = np.abs(got.astype(np.float64) - want[name])
        bound = (want[name + "_n"] + 2) * U * want[name + "_S"]
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{R.case_id(c)} {name}: max |err| {err.max():.3e}, worst err / bound {worst:.3f}")
        assert (err <= bound).all(), (name, worst)
    again = run_kernels(c, lens, x, W, g)
    poisoned = run_kernels(c, lens, x, W, g, ldx_extra=8, ldg_extra=1, poison=True)
    for name, a, b, p in zip(("dx", "dW", "db"), first, again, poisoned):
        assert np.array_equal(_bits(a), _bits(b)), f"{name}: two calls differ"
        assert np.array_equal(_bits(a), _bits(p)), f"{name}: NaN in invalid rows (or other strides) changed the result"


def test_tdnn_affine_is_the_kernels_behind_autograd():
    c = dict(context=[-2, 0, 2], padding="SAME", sub=1, din=30, units=130)
    lens = [70, 0, 1, 64, 33]
    rng = np.random.default_rng(7)
    x = rng.standard_normal((5, 70, 30)).astype(np.float32)
    W = rng.standard_normal((130, 3, 30)).astype(np.float32)
    bias = rng.standard_normal(130).astype(np.float32)
    g = rng.standard_normal((5, 70, 130)).astype(np.float32)
    tx, tW, tb = (torch.as_tensor(a, device=DEV).requires_grad_(True) for a in (x, W, bias))
    z = A.tdnn_affine(tx, tW, tb, c["context"], torch.as_tensor(lens, device=DEV))
    zr = R.tdnn_forward(x, W, bias, lens, c["context"])
    S = R.tdnn_forward(np.abs(x), np.abs(W), np.abs(bias), lens, c["context"])       # 3 * 30 products and the bias per element
    assert z.shape == zr.shape and (np.abs(z.detach().cpu().numpy() - zr) <= (91 + 2) * U * S).all()
    z.backward(torch.as_tensor(g, device=DEV))
    for got, direct in zip((tx.grad, tW.grad, tb.grad), run_kernels(c, lens, x, W, g)):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(direct))
    # no bias, no lengths, a frozen input
    z2 = A.tdnn_affine(torch.as_tensor(x, device=DEV), tW, None, c["context"])
    assert np.abs(z2.detach().cpu().numpy() - R.tdnn_forward(x, W, None, [70] * 5, c["context"])).max() < 1e-3
    tW.grad = None
    z2.backward(torch.as_tensor(g, device=DEV))
    want = R.tdnn_grads(x, W, g, [70] * 5, c["context"])
    assert (np.abs(tW.grad.cpu().numpy() - want["dW"]) <= (want["dW_n"] + 2) * U * want["dW_S"]).all()


# ----------------------------------------------------------------------------- the pooling gradient
@pytest.mark.parametrize("include_std,period", [(True, 1), (True, 3), (False, 1)])
def test_pooling_gradient(include_std, period):
    rng = np.random.default_rng(33)
    lens = [0, 1, 7, 50, 33, 2]
    B, Tm, D = len(lens), 50, 70                                # two column blocks of 64, the second partly filled
    x = (rng.standard_normal((B, Tm, D)) + 0.5 * rng.uniform(-1, 1, D)).astype(np.float32)        # |mean| <= std per column
    x[:, :, 5] = 1.5                                            # a constant column: E[x^2] - mean^2 = 0 exactly, the relu clips
    gout = rng.standard_normal((B, 2 * D if include_std else D)).astype(np.float32)
    poisoned = x.copy()
    for b, n in enumerate(lens):
        poisoned[b, n:] = NAN
    tl = torch.as_tensor(lens, device=DEV)
    tx = torch.as_tensor(poisoned, device=DEV).requires_grad_(True)
    y = A.stats_pooling(tx, tl, include_std, 1e-10, period)
    yr = R.pool_forward(x, lens, include_std, 1e-10, period)
    live = [b for b, n in enumerate(lens) if n > 0]
    assert np.abs(y.detach().cpu().numpy()[live] - yr[live]).max() <= 4 * U * np.abs(yr[live]).max()
    y.backward(torch.as_tensor(gout, device=DEV))
    got = tx.grad.cpu().numpy()
    want, M = R.pool_grad(x, lens, gout, include_std, 1e-10, period)
    err = np.abs(got.astype(np.float64) - want)
    print(f"pooling std={include_std} period={period}: max |err| {err.max():.3e}, worst err / bound {(err / np.maximum(4 * U * M, 1e-300)).max():.3f}")
    assert (err <= 4 * U * M).all()
    for b, n in enumerate(lens):
        assert not got[b, n:].any()
        n_rows = len(range(0, n, period))
        if n_rows:                                              # the clipped relu: the mean term alone, rounded once
            assert np.array_equal(got[b, 0:n:period, 5], np.full(n_rows, np.float32(np.float64(gout[b, 5]) / n_rows)))
    # a row stride of its own for the gradient buffer, pad columns written as zero
    dx = torch.full((B, Tm, D + 3), NAN, device=DEV)
    ops.grad_stats_pool(torch.as_tensor(poisoned, device=DEV), D, tl.to(torch.int32), period, include_std, 1e-10,
                        torch.as_tensor(gout, device=DEV), dx)
    dx = dx.cpu().numpy()
    assert np.array_equal(_bits(dx[:, :, :D]), _bits(got)) and not dx[:, :, D:].any()


# ----------------------------------------------------------------------------- the network
FEAT, UNITS, CLASSES = 24, 64, 4
NET_LENS = [40, 90, 57, 64, 65, 71, 83, 48]


def _stack():
    Lr, M = ktf.layers, ktf.models
    layers = [M.Input(shape=(None, FEAT))]
    for i, ctx in enumerate(([-2, -1, 0, 1, 2], [-2, 0, 2], [0])):
        layers += [Lr.TDNN(UNITS, ctx, name=f"tdnn{i + 1}"), Lr.ReLU(name=f"relu{i + 1}"), Lr.BatchNorm(name=f"bn{i + 1}")]
    layers += [Lr.StatsPooling(0, 0, reduce_time_axis=True, name="stats"), Lr.TDNN(UNITS, [0], name="affine1"), Lr.ReLU(name="relu4"),
               Lr.BatchNorm(name="bn4"), Lr.TDNN(UNITS, [0], name="affine2")]
    return M.Sequential(layers, name="small_xvector")


def _problem(seed=17):
    """8 utterances of 40-90 frames, 4 classes: a class-dependent offset under unit noise."""
    rng = np.random.default_rng(seed)
    labels = np.arange(len(NET_LENS)) % CLASSES
    centres = rng.standard_normal((CLASSES, FEAT))
    feats = (rng.standard_normal((len(NET_LENS), max(NET_LENS), FEAT)) + centres[labels][:, None, :]).astype(np.float32)
    head = (rng.standard_normal((CLASSES, UNITS)) / np.sqrt(UNITS)).astype(np.float32)
    return feats, labels, head


def _restated_bn(x, lens, gamma, eps):
    """Training-mode BatchNorm on the valid rows, textbook form; (B, T, D) with lens, or (B, D)."""
    if lens is None:
        return gamma * (x - x.mean(0)) / torch.sqrt(x.var(0, unbiased=False) + eps)
    rows = torch.cat([x[b, :n] for b, n in enumerate(lens)])
    mean, var = rows.mean(0), rows.var(0, unbiased=False)
    mask = (torch.arange(x.shape[1])[None, :] < torch.tensor(lens)[:, None]).unsqueeze(-1)
    return torch.where(mask, gamma * (x - mean) / torch.sqrt(var + eps), torch.zeros((), dtype=x.dtype))


def _restated_net(seq, params, feats, lens):
    x, it, pooled = feats, iter(params), False
    for l in seq.layers:
        if isinstance(l, ktf.layers.TDNN):
            w, b = next(it), next(it)
            if pooled:
                x = x @ w[:, 0, :].T + b
            else:
                x = restated_tdnn(x, w, b, lens, list(l.context), 1, "SAME")
        elif isinstance(l, ktf.layers.ReLU):
            x = torch.relu(x)
        elif isinstance(l, ktf.layers.BatchNorm):
            x = _restated_bn(x, None if pooled else lens, next(it), l.epsilon)
        else:
            x, pooled = restated_pool(x, lens, l.includeStd, l.epsilon, l.inputPeriod), True
    return x


def test_trainable_sequential_gradients_training_and_export():
    """First-step parameter gradients against fp64 autograd of the CPU restatement. Bound, per parameter tensor:
    |got - ref| <= 14 * (n + 2) * 2^-24 * 8 * max|ref|, from the rounding test's (n + 2) 2^-24 S per stage with n = 8 * 90 = 720, the
    rows of the batch (the longest sum any stage takes: dW, dbias and the BatchNorm statistics; the GEMMs' own reductions have at most
    5 * 64 terms), 14 stages between the loss and the first layer's weights (five GEMMs, four normalisations and the pooling, forward
    and back, the elementwise ones counted with their GEMM), and a factor 8 for S / |value| and the 1 / std of the normalisations
    (inputs of unit scale, gamma = 1). That is 4.8e-3 of the tensor's largest gradient: bf16 anywhere in the chain (2^-9 per stage)
    does not pass, fp32 throughout is expected three orders below."""
    seq = _stack()
    feats, labels, head = _problem()
    net = A.TrainableSequential(seq).train()
    tf_, tl, th = torch.as_tensor(feats, device=DEV), torch.as_tensor(NET_LENS, device=DEV), torch.as_tensor(head, device=DEV)
    ty = torch.as_tensor(labels, device=DEV)
    loss_fn = torch.nn.functional.cross_entropy

    out = net(tf_, tl)
    assert out.shape == (len(NET_LENS), UNITS)
    loss = loss_fn(out @ th.T, ty)
    loss.backward()
    ref_params = [p.detach().cpu().to(torch.float64).requires_grad_(True) for p in net.params]
    ref_loss = loss_fn(_restated_net(seq, ref_params, torch.tensor(feats, dtype=torch.float64), NET_LENS) @ torch.tensor(head, dtype=torch.float64).T,
                       torch.tensor(labels))
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
    factor = 14 * (8 * 90 + 2) * U * 8
    for i, (p, r) in enumerate(zip(net.params, ref_params)):
        err = float((p.grad.cpu().to(torch.float64) - r.grad).abs().max())
        scale = float(r.grad.abs().max())
        print(f"parameter {i} {tuple(p.shape)}: max |err| {err:.3e}, max |ref| {scale:.3e}, bound {factor * scale:.3e}")
        assert err <= factor * scale, (i, err, factor * scale)

    # 30 SGD steps on the fixed problem lower the loss
    opt = torch.optim.SGD(list(net.parameters()), lr=0.05)
    losses = [loss.item()]
    for _ in range(30):
        opt.zero_grad()
        step_loss = loss_fn(net(tf_, tl) @ th.T, ty)
        step_loss.backward()
        opt.step()
        losses.append(step_loss.item())
    print(f"loss: first {losses[0]:.4f}, after 30 steps {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]

    # export: the layers hold the parameters bit for bit, and the Sequential runs on the inference kernels
    versions = [l._version for l in seq.layers if hasattr(l, "_version")]
    assert net.export() is seq
    assert all(l._version > v for l, v in zip([l for l in seq.layers if hasattr(l, "_version")], versions))
    it = iter(net.params)
    for l in seq.layers:
        if isinstance(l, ktf.layers.TDNN):
            kernel, bias = l.get_weights()
            assert np.array_equal(_bits(kernel[0].transpose(2, 0, 1)), _bits(next(it).detach().cpu().numpy()))
            assert np.array_equal(_bits(bias), _bits(next(it).detach().cpu().numpy()))
        elif isinstance(l, ktf.layers.BatchNorm):
            at = [s[2] for s in net.steps if s[1] is l][0]
            gamma, mean, var = l.get_weights()
            assert np.array_equal(_bits(gamma), _bits(next(it).detach().cpu().numpy()))
            assert np.array_equal(_bits(mean), _bits(getattr(net, f"moving_mean_{at}").cpu().numpy()))
            assert np.array_equal(_bits(var), _bits(getattr(net, f"moving_var_{at}").cpu().numpy()))
            assert not np.array_equal(mean, np.zeros_like(mean))        # training moved the statistics
    one = tf_[1:2]                                              # the longest utterance: no padding rows, no lengths needed
    with torch.no_grad():
        want = net.eval()(one, None).cpu().numpy().reshape(-1)
    assert seq.gemm == "f32"
    got = seq(one).cpu().numpy().reshape(-1)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
