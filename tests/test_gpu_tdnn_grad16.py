"""The 16-bit TDNN gradient kernels (csrc/tdnn_grad16.hip, include/ktf_grad.h rules 6 - 9) and the `gemm=` modes of ktf.autograd on the
GPU, against the fp64 oracle and the a-priori bounds of tests/_tdnn_grad16_ref.py. Shapes, lengths and strides are those of
tests/test_gpu_tdnn_grad.py (the 64-row tile of the data gradient, the 512-row slots and the edge rows are where they were; the K-step
is 32 instead of 16, and every length that straddles 16 straddles or precedes 32 as well: 15 / 16 / 17, 33, 63 / 64 / 65).

Exact test: every operand is a bf16 number and every sum of magnitudes is below 2^24, so the results must EQUAL the oracle; g goes up
to 255 so that a fold of two or three rows needs more than the 8 bits of one bf16. Single-product test: round to nearest even, not
truncation, bit for bit. Rounding test: Gaussian operands fed unrounded, every element within its bound."""

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
from kaldi_tflite_amd import _lib as L, autograd as A, ops  # noqa: E402
import _tdnn_grad_ref as R  # noqa: E402
import _tdnn_grad16_ref as R16  # noqa: E402
from _tdnn16_ref import X3_OPERANDS, bf16_rne  # noqa: E402
from test_tdnn_grad_cpu import restated_pool, restated_tdnn  # noqa: E402
from test_gpu_tdnn_grad import NET_LENS, ROUNDING, _bits, _problem, _restated_bn, _restated_net, _stack, _tout  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = R.cases()
MODES = R16.MODES
CODE = {"bf16": L.GEMM_BF16, "bf16x3": L.GEMM_BF16X3}
U = 2.0 ** -24
DEV = "cuda:0"
NAN = float("nan")


def run_kernels16(mode, c, lens, x, W, g, ldx_extra=0, ldg_extra=0, poison=False):
    """test_gpu_tdnn_grad.run_kernels on the ktf_grad_tdnn16_* calls in `mode`: -> (dx (B, T, din), dW (units, nctx, din), db) as numpy,
    after checking that every element of the padded outputs was written and that the pad regions and the rows at or beyond an
    utterance's length hold zero. Outputs and workspace start as NaN patterns. `poison`: NaN in every invalid row of x and g."""
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
    ws = ops.grad_tdnn16_workspace(B, Tm, d, CODE[mode], xp.device)
    ws.fill_(0xFF)
    dxp = torch.full((B, Tm, ldx), NAN, device=DEV)
    dwp = torch.full((Up, nctx * Dp), NAN, device=DEV)
    db = torch.full((units,), NAN, device=DEV)
    ops.grad_tdnn16_data(gp, tl, d, wp, dxp, ws, CODE[mode])
    ops.grad_tdnn16_weights(xp, tl, d, gp, dwp, db, ws, CODE[mode])
    dxp, dwp, db = dxp.cpu().numpy(), dwp.cpu().numpy().reshape(Up, nctx, Dp), db.cpu().numpy()
    assert not np.isnan(dxp).any() and not np.isnan(dwp).any() and not np.isnan(db).any()
    assert not dxp[:, :, D:].any() and not dwp[units:].any() and not dwp[:, :, D:].any()
    for b, n in enumerate(lens):
        assert not dxp[b, n:].any()
    return dxp[:, :, :D], dwp[:units, :, :D], db


# ----------------------------------------------------------------------------- 1. exact
_EXACT = {}


def _exact_problem(c):
    """Integer operands and their fp64 gradients, computed once per case and shared by the modes (read only)."""
    key = R.case_id(c)
    if key not in _EXACT:
        rng = np.random.default_rng(161)
        lens = R.lens_for(c, ops.grad_tdnn_slot_rows())
        shapes = ((len(lens), R.T, c["din"]), (c["units"], len(c["context"]), c["din"]), (len(lens), _tout(c), c["units"]))
        x, W, g = (rng.integers(-m, m + 1, s).astype(np.float32) for m, s in zip((4, 2, 255), shapes))
        assert all(np.array_equal(bf16_rne(a), a) for a in (x, W, g))         # bf16 numbers: both modes multiply the same operands
        want = R.tdnn_grads(x, W, g, lens, c["context"], c["sub"], c["padding"])
        assert max(np.abs(want[k + "_S"]).max() for k in ("dx", "dW", "db")) < 2 ** 24
        for a in (x, W, g) + tuple(want.values()):
            a.setflags(write=False)
        _EXACT[key] = (lens, x, W, g, want)
    return _EXACT[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_exact_integers(c, mode):
    lens, x, W, g, want = _exact_problem(c)
    if c["padding"] == "SAME":                                    # a fold of two rows or more does not fit one bf16
        low = [t for t in range(_tout(c)) if t * c["sub"] + c["context"][0] < 0]          # the longest utterance's rows clamped to row 0
        assert len(low) == -(-max(-c["context"][0], 0) // c["sub"])
        if len(low) >= 2:
            f = g[int(np.argmax(lens)), low].sum(0)
            assert (bf16_rne(f) != f).any()
    dx, dW, db = run_kernels16(mode, c, lens, x, W, g, ldx_extra=4 * (c["sub"] == 3), ldg_extra=3 * (c["padding"] == "VALID"))
    for name, got in (("dx", dx), ("dW", dW), ("db", db)):
        bad = np.argwhere(got != want[name].astype(np.float32))
        assert len(bad) == 0, (name, len(bad), bad[:5].tolist())


# ----------------------------------------------------------------------------- 2. single products
def _tie_values(n, seed):
    """fp32 values on and next to bf16 ties: upper halves with an even and an odd last bit, both signs, several exponents; lower
    halves exactly half a bf16 ulp (the tie), one fp32 ulp below and above it, zero, one ulp above zero and one below the next."""
    uppers = [0x3F80, 0x3F81, 0xBF80, 0xBF81, 0x4049, 0xC048, 0x3EAA, 0xBEAB, 0x41FF, 0xC1FE]
    lowers = [0x8000, 0x7FFF, 0x8001, 0x0000, 0x0001, 0xFFFF]
    bits = np.array([(u << 16) | lo for u in uppers for lo in lowers], np.uint32)
    vals = np.random.default_rng(seed).permutation(bits)
    return np.resize(vals, n).view(np.float32)


def test_single_products_round_to_nearest_even():
    mode = "bf16"
    ties = _tie_values(60, 0)
    r = bf16_rne(ties)
    on_tie = (ties.view(np.uint32) & 0xFFFF) == 0x8000
    assert on_tie.any() and ((r.view(np.uint32)[on_tie] >> 16) & 1 == 0).all()          # the reference itself rounds ties to even
    assert (r != (ties.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)).any()  # ... and is not truncation
    lens = [1]
    # dx: one unit, one context, one row: dx[0, 0, d] = bf16(g) * bf16(W[0, 0, d])
    c = dict(context=[0], padding="SAME", sub=1, din=23, units=1)
    W = _tie_values(23, 1).reshape(1, 1, 23)
    for gv in _tie_values(60, 2)[:8]:
        g = np.full((1, 1, 1), gv, np.float32)
        dx, _, db = run_kernels16(mode, c, lens, np.zeros((1, 1, 23), np.float32), W, g)
        want = (bf16_rne(g).astype(np.float64).reshape(()) * bf16_rne(W).astype(np.float64).reshape(23)).astype(np.float32)
        assert np.array_equal(_bits(dx.reshape(23)), _bits(want)), (gv, dx, want)
        assert np.array_equal(_bits(db), _bits(g.reshape(1)))                            # the bias gradient is not rounded
    # dW: dW[u, 0, d] = bf16(g[u]) * bf16(x[d])
    c = dict(context=[0], padding="SAME", sub=1, din=23, units=40)
    g = _tie_values(40, 3).reshape(1, 1, 40)
    x = _tie_values(23, 4).reshape(1, 1, 23)
    _, dW, db = run_kernels16(mode, c, lens, x, np.zeros((40, 1, 23), np.float32), g)
    want = np.outer(bf16_rne(g).astype(np.float64).reshape(40), bf16_rne(x).astype(np.float64).reshape(23)).astype(np.float32)
    assert np.array_equal(_bits(dW.reshape(40, 23)), _bits(want))
    assert np.array_equal(_bits(db), _bits(g.reshape(40)))


# ----------------------------------------------------------------------------- 3. rounding, determinism, invalid rows
_GAUSS = {}


def _gauss_problem(c):
    key = R.case_id(c)
    if key not in _GAUSS:
        rng = np.random.default_rng(202)
        lens = R.lens_for(c, ops.grad_tdnn_slot_rows())
        shapes = ((len(lens), R.T, c["din"]), (c["units"], len(c["context"]), c["din"]), (len(lens), _tout(c), c["units"]))
        _GAUSS[key] = (lens,) + tuple(rng.standard_normal(s).astype(np.float32) for s in shapes)
    return _GAUSS[key]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", ROUNDING, ids=R.case_id)
def test_rounding_bound_determinism_and_invalid_rows(c, mode):
    lens, x, W, g = _gauss_problem(c)
    want = R16.tdnn_grads16(x, W, g, lens, c["context"], c["sub"], c["padding"], mode)
    assert want["dx_n"].max() <= 2600 and want["dW_n"].max() <= 2000
    first = run_kernels16(mode, c, lens, x, W, g)
    for name, got in zip(("dx", "dW", "db"), first):
        err = np.abs(got.astype(np.float64) - want[name])
        bound = want[name + "_bound"]
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{mode} {R.case_id(c)} {name}: max |err| {err.max():.3e}, worst err / bound {worst:.3f}")
        assert (err <= bound).all(), (name, worst)
    again = run_kernels16(mode, c, lens, x, W, g)
    poisoned = run_kernels16(mode, c, lens, x, W, g, ldx_extra=8, ldg_extra=1, poison=True)
    for name, a, b, p in zip(("dx", "dW", "db"), first, again, poisoned):
        assert np.array_equal(_bits(a), _bits(b)), f"{name}: two calls differ"
        assert np.array_equal(_bits(a), _bits(p)), f"{name}: NaN in invalid rows (or other strides) changed the result"


# ----------------------------------------------------------------------------- 4. autograd is the kernels
@pytest.mark.parametrize("mode", MODES)
def test_tdnn_affine_is_the_kernels_behind_autograd(mode):
    c = dict(context=[-2, 0, 2], padding="SAME", sub=1, din=30, units=130)
    lens = [70, 0, 1, 64, 33]
    rng = np.random.default_rng(7)
    x = rng.standard_normal((5, 70, 30)).astype(np.float32)
    W = rng.standard_normal((130, 3, 30)).astype(np.float32)
    bias = rng.standard_normal(130).astype(np.float32)
    g = rng.standard_normal((5, 70, 130)).astype(np.float32)
    tx, tW, tb = (torch.as_tensor(a, device=DEV).requires_grad_(True) for a in (x, W, bias))
    tl = torch.as_tensor(lens, device=DEV)
    z = A.tdnn_affine(tx, tW, tb, c["context"], tl, gemm=mode)
    # the forward: ktf_tdnn in that mode on the fp32 x, with the weight operand(s) rounded from the fp32 parameter
    d = A._desc(130, 30, c["context"], 1, "SAME")
    d.gemm, d.w_dtype = CODE[mode], L.KTF_BF16
    xp = torch.nn.functional.pad(tx.detach(), (0, 2)).contiguous()
    wp = torch.zeros((256, 3, 32), device=DEV)
    wp[:130, :, :30] = tW.detach()
    wp = wp.view(256, 96)
    wh = wp.to(torch.bfloat16)
    wl = (wp - wh.to(torch.float32)).to(torch.bfloat16) if mode == "bf16x3" else None
    y = torch.zeros((5, 70, 130), device=DEV)
    ops.tdnn(xp, tl.to(torch.int32), d, wh, wl, tb.detach(), None, None, y)
    assert ops.last_kernel().startswith("tdnn_bf16_kernel")
    assert np.array_equal(_bits(z.detach().cpu().numpy()), _bits(y.cpu().numpy()))
    # ... and the layer's value: operands off by 2^-8 each in the one-pass mode, _tdnn16_ref's items 1 and 2 in the split mode
    zr = R.tdnn_forward(x, W, bias, lens, c["context"])
    S = R.tdnn_forward(np.abs(x), np.abs(W), np.abs(bias), lens, c["context"])       # 3 * 30 products and the bias per element
    allowed = (2.0 ** -7 + 2.0 ** -16 + 93 * U) * S if mode == "bf16" else ((3 * 91 + 2) * U * 1.02 + X3_OPERANDS) * S
    assert (np.abs(z.detach().cpu().numpy() - zr) <= allowed).all()
    z.backward(torch.as_tensor(g, device=DEV))
    for got, direct in zip((tx.grad, tW.grad, tb.grad), run_kernels16(mode, c, lens, x, W, g)):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(direct))
    # "f32" stays the fp32 calls: other bits than the 16-bit modes' on Gaussian operands
    tW.grad = None
    A.tdnn_affine(tx.detach(), tW, None, c["context"], tl).backward(torch.as_tensor(g, device=DEV))
    f32 = tW.grad.cpu().numpy()
    want = R.tdnn_grads(x, W, g, lens, c["context"])
    assert (np.abs(f32 - want["dW"]) <= (want["dW_n"] + 2) * U * want["dW_S"]).all()


# ----------------------------------------------------------------------------- 5. the network
def _bf(t):
    """fp64 values as the kernels see them in the one-pass mode: the fp32 value rounded to bf16, nearest even."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


class _RoundedTdnn(torch.autograd.Function):
    """The contract of KTF_GEMM_BF16 in fp64: forward on bf16(x), bf16(W); dx from bf16(g), bf16(W); dW from bf16(g), bf16(x); dbias
    from the unrounded g."""

    @staticmethod
    def forward(ctx, x, W, b, lens, context):
        ctx.save_for_backward(x, W, b)
        ctx.cfg = (lens, context)
        return restated_tdnn(_bf(x), _bf(W), b, lens, context, 1, "SAME")

    @staticmethod
    def backward(ctx, g):
        x, W, b = ctx.saved_tensors
        lens, context = ctx.cfg
        with torch.enable_grad():
            xq, Wq, bq = (t.detach().requires_grad_(True) for t in (_bf(x), _bf(W), b))
            z = restated_tdnn(xq, Wq, bq, lens, context, 1, "SAME")
            dx, dW = torch.autograd.grad(z, (xq, Wq), _bf(g), retain_graph=True)
            db, = torch.autograd.grad(z, (bq,), g)
        return dx, dW, db, None, None


def _restated_net_rounded(seq, params, feats, lens):
    x, it, pooled = feats, iter(params), False
    for l in seq.layers:
        if isinstance(l, ktf.layers.TDNN):
            w, b = next(it), next(it)
            if pooled:                                          # the (B, units) affines run in the same mode: one sequence of B rows
                x = _RoundedTdnn.apply(x.unsqueeze(0), w, b, [x.shape[0]], [0]).squeeze(0)
            else:
                x = _RoundedTdnn.apply(x, w, b, lens, list(l.context))
        elif isinstance(l, ktf.layers.ReLU):
            x = torch.relu(x)
        elif isinstance(l, ktf.layers.BatchNorm):
            x = _restated_bn(x, None if pooled else lens, next(it), l.epsilon)
        else:
            x, pooled = restated_pool(x, lens, l.includeStd, l.epsilon, l.inputPeriod), True
    return x


@pytest.mark.parametrize("mode", MODES)
def test_trainable_sequential_in_a_16_bit_mode(mode):
    """First-step parameter gradients against fp64 autograd of a CPU restatement: the unrounded one for "bf16x3", the one with the
    contract's operand rounding in every TDNN forward and backward for "bf16". Bound per parameter tensor: the fp32 network test's,
    14 * (8 * 90 + 2) * 2^-24 * 8 * max|ref| (its docstring derives it); the x3 operand term, 3 * 2^-16 per stage, is two orders below.
    Measured on the MI355X: "bf16x3" within 0.004 of the bound on every tensor; "bf16" within 0.16 to 0.87 of it -- the rounded
    restatement is sensitive by itself (an fp32 activation that differs from the fp64 one in its last bits now and then rounds to the
    other bf16 neighbour, which moves a whole row of the next layer by 2^-8 of a term), so that margin is the reference's, not rounding
    error of the kernels. The distance of the "bf16" gradients to the UNROUNDED fp64 ones, printed only: 0.5 % to
    33 % of the tensor's largest gradient."""
    seq = _stack()
    feats, labels, head = _problem()
    net = A.TrainableSequential(seq, gemm=mode).train()
    tf_, tl, th = torch.as_tensor(feats, device=DEV), torch.as_tensor(NET_LENS, device=DEV), torch.as_tensor(head, device=DEV)
    ty = torch.as_tensor(labels, device=DEV)
    loss_fn = torch.nn.functional.cross_entropy

    out = net(tf_, tl)
    loss = loss_fn(out @ th.T, ty)
    loss.backward()
    f64 = torch.float64
    restate = _restated_net_rounded if mode == "bf16" else _restated_net
    ref_params = [p.detach().cpu().to(f64).requires_grad_(True) for p in net.params]
    ref_loss = loss_fn(restate(seq, ref_params, torch.tensor(feats, dtype=f64), NET_LENS) @ torch.tensor(head, dtype=f64).T, torch.tensor(labels))
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
    factor = 14 * (8 * 90 + 2) * U * 8
    worst = []
    for i, (p, r) in enumerate(zip(net.params, ref_params)):
        err = float((p.grad.cpu().to(f64) - r.grad).abs().max())
        scale = float(r.grad.abs().max())
        print(f"{mode} parameter {i} {tuple(p.shape)}: max |err| {err:.3e}, max |ref| {scale:.3e}, bound {factor * scale:.3e}")
        worst.append((err, factor * scale, i))
    if mode == "bf16":                                           # printed, not asserted: the distance to the UNROUNDED fp64 gradients
        exact = [p.detach().cpu().to(f64).requires_grad_(True) for p in net.params]
        loss_fn(_restated_net(seq, exact, torch.tensor(feats, dtype=f64), NET_LENS) @ torch.tensor(head, dtype=f64).T, torch.tensor(labels)).backward()
        for i, (p, r) in enumerate(zip(net.params, exact)):
            dev = float((p.grad.cpu().to(f64) - r.grad).abs().max() / r.grad.abs().max())
            print(f"bf16 parameter {i}: max |grad - unrounded fp64 grad| / max |unrounded| = {dev:.3e}")
    for err, bound, i in worst:
        assert err <= bound, (mode, i, err, bound)

    opt = torch.optim.SGD(list(net.parameters()), lr=0.05)
    losses = [loss.item()]
    for _ in range(30):
        opt.zero_grad()
        step_loss = loss_fn(net(tf_, tl) @ th.T, ty)
        step_loss.backward()
        opt.step()
        losses.append(step_loss.item())
    print(f"{mode} loss: first {losses[0]:.4f}, after 30 steps {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]

    # export is the same in every mode: fp32 parameters, and the Sequential runs on the inference kernels in bf16x3. Compared with the
    # exported weights on the fp32 path; per GEMM stage the split operands add (3 + 2^-6) 2^-16 of S (five stages, the factor 8 of the
    # gradient bound for S / |value| and the normalisations), on top of the fp32 test's own 1e-4.
    assert all(p.dtype == torch.float32 for p in net.parameters())
    assert net.export() is seq
    it = iter(net.params)
    for l in seq.layers:
        if isinstance(l, ktf.layers.TDNN):
            kernel, b = l.get_weights()
            assert np.array_equal(_bits(kernel[0].transpose(2, 0, 1)), _bits(next(it).detach().cpu().numpy()))
            assert np.array_equal(_bits(b), _bits(next(it).detach().cpu().numpy()))
        elif isinstance(l, ktf.layers.BatchNorm):
            next(it)
    one = tf_[1:2]
    with torch.no_grad():
        want = A.TrainableSequential(seq).eval()(one, None).cpu().numpy().reshape(-1)
    seq.gemm = "bf16x3"
    got = seq(one).cpu().numpy().reshape(-1)
    assert got.shape == want.shape and np.isfinite(got).all()
    assert np.abs(got - want).max() <= (1e-4 + 5 * 8 * X3_OPERANDS) * max(1.0, np.abs(want).max())
