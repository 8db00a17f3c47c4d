"""ReLU + BatchNorm training kernels (include/ktf_norm.h) on the GPU against the fp64 oracle of tests/_norm_ref.py, and
ktf.autograd.relu_batch_norm / TrainableSequential(fused_norm=True) over them.

Bounds (u = 2^-24, the unit roundoff of fp32; every output is fp64 arithmetic rounded once, so u times the value is what the
rounding alone may cost and the bounds below leave a factor 2):
    y        |got - ref| <= 2 u (|a| + |mean|) |gamma invstd|
    dz       |got - ref| <= 2 u |gamma invstd| (|gy| + |s1 / n| + |ahat s2 / n|)
    dgamma   |got - ref| <= u |s2| + n 2^-53 sum |gy ahat|       (one rounding of s2, which may use all of u |s2|, plus the fp64 sum)
The worst ratios measured are in DESIGN.md section 7."""

import functools
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
import _norm_ref as N  # noqa: E402
from test_tdnn_grad_cpu import restated_pool, restated_tdnn  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DEV = "cuda:0"
NAN = float("nan")
MOMENTUM, EPS = 0.9, 1e-3


def _shape():
    """B, T, lens from the slot size: B * T spans four slots with a partial last one; lengths 0, 1 and T; the last utterance, of
    full length, crosses a slot boundary."""
    slot = ops.norm_slot_rows()
    B, T = 5, slot * 45 // 64
    lens = [T, 0, 1, T - 3, T]
    assert 3 * slot < B * T < 4 * slot and (4 * T) // slot != (5 * T - 1) // slot
    return B, T, lens


def _dev(a):
    return torch.as_tensor(np.array(a), device=DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _buffer(values, lens, extra, offset, poison):
    """A (B, T, D + extra) device view holding `values` in its valid rows and first D columns, starting `offset` floats into its
    allocation; everything else is NaN (poison) or zero."""
    B, T, D = values.shape
    ld = D + extra
    host = np.full((B, T, ld), NAN if poison else 0.0, dtype=np.float32)
    for b in range(B):
        n = T if lens is None else lens[b]
        host[b, :n, :D] = values[b, :n]
    if not poison:
        host[:, :, :D] = values
    flat = torch.full((B * T * ld + offset,), NAN, dtype=torch.float32, device=DEV)
    view = flat[offset:].view(B, T, ld)
    view.copy_(torch.as_tensor(host))
    return view


def run_kernels(z, gy, lens, relu, training, gamma, mm, mv, momentum=MOMENTUM, eps=EPS, extra=0, offset=0, poison=False):
    """Both calls on fresh buffers whose outputs start as NaN. Returns numpy: y and dz with their pad columns, saved, the moving
    statistics after the forward call, dgamma."""
    B, T, D = z.shape
    tl = None if lens is None else torch.as_tensor(lens, dtype=torch.int32, device=DEV)
    tz, tg = _buffer(z, lens, extra, offset, poison), _buffer(gy, lens, extra, offset, poison)
    ty = torch.full((B * T * (D + extra) + offset,), NAN, dtype=torch.float32, device=DEV)[offset:].view(B, T, D + extra)
    tdz = torch.full((B * T * (D + extra) + offset,), NAN, dtype=torch.float32, device=DEV)[offset:].view(B, T, D + extra)
    tgam = _dev(np.asarray(gamma, dtype=np.float32))
    tmm, tmv = (_dev(np.asarray(a, dtype=np.float32)) for a in (mm, mv))
    saved = torch.full((2, D), NAN, dtype=torch.float64, device=DEV)
    dgamma = torch.full((D,), NAN, dtype=torch.float32, device=DEV)
    ws = ops.norm_workspace(B, T, D, DEV)
    ws.fill_(0xFF)
    ops.norm_relu_bn_forward(tz, D, tl, relu, training, tgam, tmm, tmv, momentum, eps, ty, saved, ws)
    ops.norm_relu_bn_backward(tg, tz, D, tl, relu, training, tgam, saved, tdz, dgamma, ws)
    torch.cuda.synchronize()
    return dict(y=ty.cpu().numpy(), dz=tdz.cpu().numpy(), saved=saved.cpu().numpy(), mm=tmm.cpu().numpy(), mv=tmv.cpu().numpy(),
                dgamma=dgamma.cpu().numpy())


def check_zero_regions(got, lens, D):
    for name in ("y", "dz"):
        out = got[name]
        assert not out[:, :, D:].any() and not np.isnan(out).any(), name
        for b, n in enumerate(lens or []):
            assert not out[b, n:].any(), (name, b)


@functools.lru_cache(maxsize=None)
def _gaussian(D, relu=True, training=True, with_lens=True):
    """Inputs of one width and their oracle, computed once and shared by the tests that use them (read-only)."""
    B, T, lens = _shape()
    lens = lens if with_lens else None
    rng = np.random.default_rng(100 + D)
    z = (rng.standard_normal((B, T, D)) + 0.25).astype(np.float32)
    gy = rng.standard_normal((B, T, D)).astype(np.float32)
    gamma = rng.uniform(0.5, 2.0, D).astype(np.float32)
    mm, mv = rng.standard_normal(D).astype(np.float32), rng.uniform(0.5, 2.0, D).astype(np.float32)
    f = N.forward(z, lens, relu, training, gamma, mm, mv, MOMENTUM, EPS)
    g = N.backward(gy, z, lens, relu, training, gamma, f["mean"], f["invstd"])
    for a in (z, gy, gamma, mm, mv):
        a.setflags(write=False)
    return dict(z=z, gy=gy, lens=lens, gamma=gamma, mm=mm, mv=mv, f=f, g=g)


def check_against_oracle(got, c, D, training, tag):
    f, g = c["f"], c["g"]
    y, dz = got["y"][:, :, :D].astype(np.float64), got["dz"][:, :, :D].astype(np.float64)
    ratios = {}
    for name, err, bound in (("y", np.abs(y - f["y"]), 2 * U * f["y_mag"]), ("dz", np.abs(dz - g["dz"]), 2 * U * g["dz_mag"]),
                             ("dgamma", np.abs(got["dgamma"].astype(np.float64) - g["dgamma"]),
                              U * np.abs(g["s2"]) + g["n"] * 2.0 ** -53 * g["dgamma_abs"])):
        live = bound > 0
        ratios[name] = float((err[live] / bound[live]).max()) if live.any() else 0.0
        assert (err[~live] == 0).all(), name                     # a zero bound: an exact zero is expected
    print(f"{tag}: worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    # the statistics: fp64 sums in another order than the oracle's; the moving statistics are those rounded once
    for got_s, want in ((got["saved"][0], f["mean"]), (got["saved"][1], f["invstd"])):
        assert np.abs(got_s - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    for got_m, want, before in ((got["mm"], f["moving_mean"], c["mm"]), (got["mv"], f["moving_var"], c["mv"])):
        if training:
            assert (np.abs(got_m.astype(np.float64) - want) <= U * np.abs(want) + 1e-12).all()
        else:
            assert np.array_equal(_bits(got_m), _bits(before))
    return ratios


# ----------------------------------------------------------------------------- rounding bounds: every width and stride
@pytest.mark.parametrize("extra", [0, 4], ids=["ld=D", "ld=D+4"])
@pytest.mark.parametrize("D", [1, 23, 40, 512, 1500])
def test_gaussian_inputs_within_the_bounds(D, extra):
    c = _gaussian(D)
    got = run_kernels(c["z"], c["gy"], c["lens"], True, True, c["gamma"], c["mm"], c["mv"], extra=extra)
    check_zero_regions(got, c["lens"], D)
    check_against_oracle(got, c, D, True, f"D={D} ld=D+{extra}")


@pytest.mark.parametrize("relu,training,with_lens", [(True, False, True), (False, True, True), (False, False, False), (True, True, False)])
def test_modes(relu, training, with_lens):
    D = 40
    c = _gaussian(D, relu, training, with_lens)
    got = run_kernels(c["z"], c["gy"], c["lens"], relu, training, c["gamma"], c["mm"], c["mv"])
    check_zero_regions(got, c["lens"], D)
    check_against_oracle(got, c, D, training, f"relu={relu} training={training} lens={with_lens}")


def test_unaligned_base_and_the_pooled_form():
    """A base 4 bytes off a 16-byte boundary takes the element-wise path: the bits are those of the aligned call (rule 9). The
    (N, D) input behind the pooling is B = 1, T = N: the same rows as one sequence give the same bits as (B, T) without lengths."""
    D = 40
    c = _gaussian(D, True, True, False)
    args = (True, True, c["gamma"], c["mm"], c["mv"])
    base = run_kernels(c["z"], c["gy"], None, *args, extra=4)
    off = run_kernels(c["z"], c["gy"], None, *args, extra=4, offset=1)
    B, T, _ = c["z"].shape
    flat = run_kernels(c["z"].reshape(1, B * T, D), c["gy"].reshape(1, B * T, D), None, *args, extra=4)
    for k in base:
        assert np.array_equal(_bits(base[k]), _bits(off[k])), k
        assert np.array_equal(_bits(base[k].reshape(flat[k].shape)), _bits(flat[k])), k
    check_against_oracle(off, c, D, True, "unaligned base")


# ----------------------------------------------------------------------------- exact cases
def test_exact_integers():
    """Small integers, n = 256: every sum, the mean and the variance are exact in fp64. Every column takes two values d apart, half
    of the valid rows each, so var = d^2 / 4 = 1 and, with eps = 3, invstd = 1 / 2: saved, the moving statistics (momentum 0.5),
    dgamma, y and dz equal the oracle bit for bit."""
    slot = ops.norm_slot_rows()
    B, T, D = 4, slot, 37
    lens = [100, 28, 0, 128]
    assert sum(lens) == 256
    rng = np.random.default_rng(2)
    centre = rng.integers(2, 9, D).astype(np.float32)
    z = np.zeros((B, T, D), dtype=np.float32)
    signs = np.concatenate([np.ones(128), -np.ones(128)])
    valid = [(b, t) for b in range(B) for t in range(lens[b])]
    for c in range(D):
        for (b, t), s in zip(valid, rng.permutation(signs)):
            z[b, t, c] = centre[c] + s
    z[:, :, 5] = np.where(z[:, :, 5] > centre[5], 2.0, -3.0)     # under relu: 0 or 2
    for b in range(B):
        z[b, lens[b]:] = 77.0
    gy = rng.integers(-4, 5, (B, T, D)).astype(np.float32)
    gamma = np.ones(D, dtype=np.float32)
    mm, mv = rng.integers(-3, 4, D).astype(np.float32), rng.integers(1, 4, D).astype(np.float32)
    f = N.forward(z, lens, True, True, gamma, mm, mv, 0.5, 3.0)
    g = N.backward(gy, z, lens, True, True, gamma, f["mean"], f["invstd"])
    assert np.array_equal(f["invstd"], np.full(D, 0.5)) and f["mean"][5] == 1.0
    for extra in (0, 3):
        got = run_kernels(z, gy, lens, True, True, gamma, mm, mv, momentum=0.5, eps=3.0, extra=extra)
        check_zero_regions(got, lens, D)
        assert np.array_equal(_bits(got["saved"]), _bits(np.stack([f["mean"], f["invstd"]])))
        assert np.array_equal(_bits(got["mm"]), _bits(f["moving_mean"].astype(np.float32)))
        assert np.array_equal(_bits(got["mv"]), _bits(f["moving_var"].astype(np.float32)))
        assert np.array_equal(_bits(got["dgamma"]), _bits(g["dgamma"].astype(np.float32)))
        assert np.array_equal(_bits(got["y"][:, :, :D]), _bits(f["y"].astype(np.float32)))
        assert np.array_equal(_bits(got["dz"][:, :, :D]), _bits(g["dz"].astype(np.float32)))


# ----------------------------------------------------------------------------- corner values
def test_corner_values():
    rng = np.random.default_rng(3)
    B, T, D = 2, 9, 6
    z = rng.standard_normal((B, T, D)).astype(np.float32)
    z[:, :, 1] = -np.abs(z[:, :, 1])                                  # every z <= 0: a = 0, var = 0, y = 0, dz = 0
    z[0, 0, 2], z[0, 1, 2], z[1, 0, 2] = 0.0, -0.0, 0.0               # relu's gradient at 0 and -0.0 is 0
    gy = rng.standard_normal((B, T, D)).astype(np.float32)
    gamma, mm, mv = np.full(D, 1.5, np.float32), np.zeros(D, np.float32), np.ones(D, np.float32)
    got = run_kernels(z, gy, None, True, True, gamma, mm, mv)
    assert not got["y"][:, :, 1].any() and not got["dz"][:, :, 1].any() and got["dgamma"][1] == 0
    assert got["saved"][0, 1] == 0 and got["saved"][1, 1] == 1.0 / np.sqrt(EPS)
    assert got["dz"][0, 0, 2] == 0 and got["dz"][0, 1, 2] == 0 and got["dz"][1, 0, 2] == 0
    assert not np.signbit(got["y"][0, 1, 1])                          # max(-0.0, 0) = +0.0 - mean 0
    # n = 1
    one = run_kernels(z, gy, [0, 1], True, True, gamma, mm, mv)
    check_zero_regions(one, [0, 1], D)
    assert np.array_equal(one["saved"][0], np.maximum(z[1, 0], 0).astype(np.float64))
    assert np.array_equal(one["saved"][1], np.full(D, 1.0 / np.sqrt(np.float64(EPS))))
    assert not one["y"].any() and not one["dz"].any() and not one["dgamma"].any()
    assert np.array_equal(one["mv"], np.full(D, np.float32(MOMENTUM)))          # 1 * momentum + 0 * (1 - momentum)
    # n = 0: every length 0, in both modes, and B * T = 0
    for training in (True, False):
        none = run_kernels(z, gy, [0, 0], True, training, gamma, mm + 2, mv, poison=True)
        assert not none["y"].any() and not none["dz"].any() and not none["dgamma"].any() and not none["saved"].any()
        assert np.array_equal(none["mm"], mm + 2) and np.array_equal(none["mv"], mv)
    for shape in ((0, 5, D), (3, 0, D)):
        e = run_kernels(np.zeros(shape, np.float32), np.zeros(shape, np.float32), None, True, True, gamma, mm + 2, mv)
        assert not e["dgamma"].any() and not e["saved"].any() and np.array_equal(e["mm"], mm + 2) and np.array_equal(e["mv"], mv)


# ----------------------------------------------------------------------------- determinism, rows and columns that are not read
@pytest.mark.parametrize("D,extra", [(40, 4), (23, 4), (512, 4)], ids=["vector", "scalar", "two-chunks"])
def test_determinism_and_invalid_data(D, extra):
    c = _gaussian(D)
    args = (c["z"], c["gy"], c["lens"], True, True, c["gamma"], c["mm"], c["mv"])
    first, second = run_kernels(*args, extra=extra), run_kernels(*args, extra=extra)
    poisoned = run_kernels(*args, extra=extra, poison=True)          # NaN in every invalid row and pad column of z and gy
    check_zero_regions(poisoned, c["lens"], D)
    for k in first:
        assert np.array_equal(_bits(first[k]), _bits(second[k])), k
        assert np.array_equal(_bits(first[k]), _bits(poisoned[k])), k


# ----------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("pooled", [False, True])
def test_relu_batch_norm_is_the_kernels_behind_autograd(pooled):
    D = 40
    c = _gaussian(D, True, True, not pooled)
    z, gy, lens = c["z"], c["gy"], c["lens"]
    if pooled:
        z, gy = z.reshape(1, -1, D), gy.reshape(1, -1, D)
    want = run_kernels(z, gy, lens, True, True, c["gamma"], c["mm"], c["mv"])
    tz = _dev(z[0] if pooled else z).requires_grad_(True)
    tg = _dev(c["gamma"]).requires_grad_(True)
    mm, mv = _dev(c["mm"]), _dev(c["mv"])
    tl = None if lens is None else torch.as_tensor(lens, device=DEV)
    y = A.relu_batch_norm(tz, tl, mm, mv, tg, momentum=MOMENTUM, epsilon=EPS, training=True)
    assert y.shape == tz.shape
    y.backward(_dev(gy[0] if pooled else gy))
    for got, k in ((y.detach(), "y"), (tz.grad, "dz"), (tg.grad, "dgamma"), (mm, "mm"), (mv, "mv")):
        assert np.array_equal(_bits(got.cpu().numpy().reshape(want[k].shape)), _bits(want[k])), k
    with pytest.raises(ValueError):
        A.relu_batch_norm(tz.detach(), tl, mm.double(), mv, tg.detach())
    with pytest.raises(ValueError):
        A.relu_batch_norm(tz.detach()[..., :8], tl, mm, mv, tg.detach())


# ----------------------------------------------------------------------------- the network (that of test_gpu_tdnn_grad.py)
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
            x = x @ w[:, 0, :].T + b if pooled else restated_tdnn(x, w, b, lens, list(l.context), 1, "SAME")
        elif isinstance(l, ktf.layers.ReLU):
            x = torch.relu(x)
        elif isinstance(l, ktf.layers.BatchNorm):
            x = _restated_bn(x, None if pooled else lens, next(it), l.epsilon)
        else:
            x, pooled = restated_pool(x, lens, l.includeStd, l.epsilon, l.inputPeriod), True
    return x


def test_trainable_sequential_with_fused_norm(monkeypatch):
    """The network test of test_gpu_tdnn_grad.py with fused_norm=True, under that test's bound: per parameter tensor
    |got - ref| <= 14 * (n + 2) * 2^-24 * 8 * max|ref| with n = 8 * 90 rows (derived there; the fused block's fp64 statistics only
    lower the error of four of the 14 stages). The evaluation outputs of the fused and the torch module, built from the same
    exported weights, differ by what four normalisations round differently: per block at most u M (fused: one rounding) plus
    5 u M (torch: subtraction, var + eps, rsqrt and two products in fp32) with M = (|a| + |mean|) |gamma invstd|, that is three
    times the y bound 2 u M; with the factor 8 of the bound above for M / |value| and what the following layers make of it,
    |fused - torch| <= 4 * 3 * 2 u * 8 * max|torch|."""
    seq = _stack()
    feats, labels, head = _problem()
    calls = []
    real = A.relu_batch_norm
    monkeypatch.setattr(A, "relu_batch_norm", lambda *a, **k: (calls.append(k.get("relu")), real(*a, **k))[1])
    net = A.TrainableSequential(seq, fused_norm=True).train()
    tf_, tl, th = torch.as_tensor(feats, device=DEV), torch.as_tensor(NET_LENS, device=DEV), torch.as_tensor(head, device=DEV)
    ty = torch.as_tensor(labels, device=DEV)
    loss_fn = torch.nn.functional.cross_entropy

    out = net(tf_, tl)
    assert out.shape == (len(NET_LENS), UNITS) and calls == [True] * 4           # every ReLU went into its BatchNorm
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

    # export: the layers hold the parameters and the moving statistics bit for bit
    assert net.export() is seq
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

    # evaluation: the torch module built from the exported layers
    plain = A.TrainableSequential(seq).eval()
    assert list(plain.state_dict()) == list(net.state_dict())
    with torch.no_grad():
        want = plain(tf_, tl).cpu().numpy()
        got = net.eval()(tf_, tl).cpu().numpy()
    diff, tol = float(np.abs(got - want).max()), 4 * 3 * 2 * U * 8 * float(np.abs(want).max())
    print(f"eval: max |fused - torch| {diff:.3e}, tolerance {tol:.3e}")
    assert got.shape == want.shape and diff <= tol
