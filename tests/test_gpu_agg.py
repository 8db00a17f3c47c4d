"""Multi-layer feature aggregation on the GPU (include/ktf_agg.h): bit for bit against tests/_agg_ref.py on exactly representable inputs
in all three modes, the bit-level invariances of rules 1 - 6, every mode against torch.cat + the TDNN kernels (the limit is measured on
that composition: e_new <= 2 e_comp + 2^-20 max|ref|), the layer inside the fused runner in every gemm mode, and training under
TrainableSequential with a ClassifierHead. Every comparison prints its figures."""

import os
import sys
import warnings

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
import _agg_ref as R  # noqa: E402
from test_loss_cpu import torch_inv_norm, torch_loss  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77.0
MODES = {"f32": L.GEMM_F32, "bf16": L.GEMM_BF16, "bf16x3": L.GEMM_BF16X3}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows(a, ld, off, fill):
    """a (..., C) fp32 as a device tensor (..., ld) whose base lies `off` floats behind a 256-byte boundary; pad columns = fill."""
    n, C = int(np.prod(a.shape[:-1])), a.shape[-1]
    buf = torch.full((n * ld + 64 + off,), fill, dtype=torch.float32, device=DEV)
    at = (-buf.data_ptr() // 4) % 64 + off
    v = buf[at:at + n * ld].view(*a.shape[:-1], ld)
    v[..., :C] = torch.as_tensor(a, device=DEV)
    return v


def run(c, lens, gemm=L.GEMM_F32, relu=True, bn=True, pad=(0, 0, 0), off=0, only=None):
    """One call on copies of c["xs"] with NaN in every row from the utterance's length on and in every pad column of every source and
    of w, into a y full of SENTINEL -> y (B, T, ldy) as numpy. pad: extra columns of (source s: pad[0] * (s + 1), w, y); `only`: that
    utterance alone."""
    xs = [np.array(x if only is None else x[only:only + 1], np.float32) for x in c["xs"]]
    lens = lens if only is None or lens is None else lens[only:only + 1]
    B, T, U = xs[0].shape[0], xs[0].shape[1], c["w"].shape[0]
    for x in xs:
        for b in range(B if lens is not None else 0):
            x[b, R.clamp_len(lens[b], T):] = np.nan
    txs = [_rows(x, x.shape[2] + pad[0] * (s + 1), off, np.nan)[:, :, :x.shape[2]] for s, x in enumerate(xs)]
    ty = _rows(np.full((B, T, U), SENTINEL, np.float32), -(-(U + pad[2]) // 4) * 4, off, SENTINEL)      # (a leading dimension is a multiple of 4)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)      # noqa: E731
    ops.agg_conv(txs, None if lens is None else dev(np.asarray(lens, np.int32)), _rows(c["w"], c["w"].shape[1] + pad[1], off, np.nan)[:, :c["w"].shape[1]],
                 dev(c["bias"]), dev(c["nscale"]) if bn else None, dev(c["nshift"]) if bn else None, L.ACT_RELU if relu else L.ACT_NONE, gemm, ty[:, :, :U])
    torch.cuda.synchronize()
    return ty.cpu().numpy()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("widths,units", R.EXACT_SHAPES)
def test_exact_inputs_give_the_reference_bit_for_bit(widths, units, mode):
    lens = R.exact_lens(ops.agg_row_tile(units, sum(widths), MODES[mode]))
    c = R.exact_case(widths, units, lens)
    for ls in (lens, None):
        ref = R.batch(c["xs"], ls, c["w"], bias=c["bias"], nscale=c["nscale"], nshift=c["nshift"], relu=True)
        y = run(c, ls, MODES[mode], pad=(4, 4, 8))
        assert (y[:, :, units:] == SENTINEL).all()
        for b, r in enumerate(ref):
            assert np.array_equal(_bits(y[b, :len(r), :units]), _bits(r)), (widths, units, mode, b, len(r))
            assert (y[b, len(r):] == SENTINEL).all(), (b, len(r))


@pytest.mark.parametrize("mode", list(MODES))
def test_strides_alignment_batch_and_the_division_of_k_do_not_change_a_bit(mode):
    widths, U, Rt = (64, 32), 136, ops.agg_row_tile(136, 96)
    lens = [Rt + 3, 0, 5, 2 * Rt + 1]
    rng = np.random.default_rng(5)
    c = R.exact_case(widths, U, lens)
    c.update(xs=[rng.standard_normal(x.shape).astype(np.float32) for x in c["xs"]], w=(rng.standard_normal(c["w"].shape) / np.sqrt(96)).astype(np.float32))
    for relu, bn in ((True, True), (False, False)):
        plain = run(c, lens, MODES[mode], relu, bn)
        assert np.isfinite(plain[0, :lens[0]]).all() and np.array_equal(_bits(plain), _bits(run(c, lens, MODES[mode], relu, bn)))
        for pad, off in (((4, 0, 0), 0), ((0, 4, 0), 0), ((0, 0, 8), 0), ((0, 0, 0), 4), ((4, 4, 8), 4), ((4, 4, 8), 1)):      # (off 1: no 16-byte alignment, the scalar feed)
            moved = run(c, lens, MODES[mode], relu, bn, pad=pad, off=off)
            assert np.array_equal(_bits(moved[:, :, :U]), _bits(plain)) and (moved[:, :, U:] == SENTINEL).all(), (pad, off)
        for b in (0, 3):
            assert np.array_equal(_bits(run(c, lens, MODES[mode], relu, bn, only=b)[0]), _bits(plain[b])), b
        cat = np.concatenate(c["xs"], 2)
        other = dict(c, xs=[cat[:, :, :32], cat[:, :, 32:]])                   # the same K as 32 + 64
        assert np.array_equal(_bits(run(other, lens, MODES[mode], relu, bn)), _bits(plain))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("widths,units", [((96, 96, 96), 288), ((256, 128), 130)])
def test_random_inputs_against_cat_and_the_tdnn_kernels(widths, units, mode):
    lens, K = [37, ops.agg_row_tile(units, sum(widths), MODES[mode]) + 5], sum(widths)
    rng = np.random.default_rng(9)
    xs = [rng.standard_normal((2, max(lens), C)).astype(np.float32) for C in widths]
    w, bias = (rng.standard_normal((units, K)) / np.sqrt(K)).astype(np.float32), (0.1 * rng.standard_normal(units)).astype(np.float32)
    nsc, nsh = rng.uniform(0.5, 2.0, units).astype(np.float32), (0.1 * rng.standard_normal(units)).astype(np.float32)
    ref = R.batch(xs, lens, w, bias=bias, nscale=nsc, nshift=nsh, relu=True)
    dev = lambda a: torch.as_tensor(a, device=DEV)      # noqa: E731
    tl = dev(np.asarray(lens, np.int32))
    got = ops.agg_conv([dev(x) for x in xs], tl, dev(w), dev(bias), dev(nsc), dev(nsh), L.ACT_RELU, MODES[mode],
                       torch.zeros((2, max(lens), ops.round_up(units, 4)), device=DEV)[:, :, :units]).cpu().numpy()
    t = ktf.layers.TDNN(units, [0], name="composition")
    t.set_weights([w.T[None, None], bias], fmt="tensorflow")
    cat = torch.cat([dev(x) for x in xs], 2).contiguous()
    comp = t.forward(t.prepare_input(cat, MODES[mode]), lens=tl, relu=True, bn=(dev(nsc), dev(nsh)), gemm=MODES[mode])[:, :, :units].float().cpu().numpy()
    e_new, e_comp = (max(float(np.abs(a[b, :n] - ref[b]).max()) for b, n in enumerate(lens)) for a in (got, comp))
    top = max(float(np.abs(r).max()) for r in ref)
    print(f"widths {widths} units {units} {mode}: e_new {e_new:.3e} e_comp {e_comp:.3e} max|ref| {top:.3e}")
    assert e_new <= 2 * e_comp + 2.0 ** -20 * top


FEAT, LENS = 24, (9, 150, 61)
_tdnn = lambda n, u, t=("tdnn",), **kw: {"name": n, "type": list(t), "cfg": dict(units=u, **kw)}      # noqa: E731
_POOL = [{"name": "pool", "type": "stats_pooling", "cfg": {"left_context": 0, "right_context": 10000, "reduce_time_axis": True}}, _tdnn("embed", 16)]
_block = lambda n, prev: [_tdnn(f"{n}.a", 32, activation="relu"), {"name": f"{n}.res", "type": "res2_conv", "cfg": {"scale": 2, "dilation": 2}},      # noqa: E731
                          _tdnn(f"{n}.c", 32), {"name": f"{n}.se", "type": "squeeze_excite", "cfg": {"bottleneck": 8, "residual_from": prev}}]
CHAINS = {"A": [_tdnn("t1", 32, ("tdnn", "relu", "bn"), context=[-2, -1, 0, 1, 2]), _tdnn("t2", 64), _tdnn("t3", 32),
                {"name": "mfa", "type": ["aggregate", "relu", "bn"], "cfg": {"units": 48, "sources": ["t1.batchnorm", "t2.affine"]}}] + _POOL,
          "B": [_tdnn("t0", 32, ("tdnn", "relu", "bn"), context=[-2, -1, 0, 1, 2])] + _block("b1", "t0.batchnorm") + _block("b2", "b1.se")
               + [{"name": "mfa", "type": ["aggregate", "relu"], "cfg": {"units": 96, "sources": ["b1.se"]}}] + _POOL}


def _layer_by_layer(mdl, x, tl, mode):
    """The model's own layer objects, evaluated as sub-chains up to every kept output, SqueezeExcite.forward and Aggregate(x, sources=...)."""
    wanted = {n for l in mdl.layers for n in getattr(l, "sources", []) + [getattr(l, "residualFrom", None)]}
    kept, chain = {}, []

    def flush(x):
        if chain:
            sub = ktf.models.Sequential([ktf.models.Input(shape=(None, None))] + chain, gemm=mode)
            sub.min_tiles, sub.min_frames = {}, {}
            x = sub.run_ragged(ktf.models._padded_copy(x, torch.float32), tl if x.shape[1] > 1 else None).float().clone()
            chain.clear()
        return x

    for l in mdl.layers:
        if isinstance(l, (ktf.layers.SqueezeExcite, ktf.layers.Aggregate)):
            x = flush(x).contiguous()
            if isinstance(l, ktf.layers.Aggregate):
                l.gemm = mode
                x = l(x, sources=[kept[n] for n in l.sources])
            else:
                x = l.forward(x, tl, kept[l.residualFrom])
        else:
            chain.append(l)
        if l.name in wanted:
            x = kept[l.name] = flush(x).contiguous()
    return flush(x)


@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16x3", "f16mx"])
@pytest.mark.parametrize("case", list(CHAINS))
def test_layer_in_the_fused_runner_in_every_mode(case, mode):
    mdl = ktf.models.SequentialFromConfig({"layers": [{"type": "input", "shape": [None, None, FEAT]}] + CHAINS[case]}, None, "mfa", gemm=mode)
    mdl.min_tiles, mdl.min_frames = {}, {}               # every batch on the mode's own kernels
    kinds = [st[0] for st in mdl._plan()]
    assert kinds.count("agg") == 1 and (case == "A" or kinds.count("se") == 2)
    x = torch.as_tensor(np.random.default_rng(22).standard_normal((len(LENS), max(LENS), FEAT)).astype(np.float32), device=DEV)
    tl = torch.as_tensor(np.asarray(LENS, np.int32), device=DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = [mdl.run_ragged(ktf.models._padded_copy(x, torch.float32), tl).float().cpu().numpy().reshape(len(LENS), -1) for _ in range(2)]
        want = _layer_by_layer(mdl, x, tl, mode).cpu().numpy().reshape(len(LENS), -1)
    tol = {"f32": 3e-5, "bf16x3": 3e-4, "bf16": 6e-2, "f16mx": 2e-3}[mode] * max(1.0, float(np.abs(want).max()))      # (tests/test_gpu_parity.py)
    print(f"runner {case} {mode}: max |err| {np.abs(got[0] - want).max():.3e}, limit {tol:.3e}")
    assert np.array_equal(_bits(got[0]), _bits(got[1])) and np.abs(got[0] - want).max() < tol


@pytest.mark.parametrize("gemm,tol", [("f32", 2e-5), ("bf16x3", 2e-4)])
def test_training_under_trainable_sequential_with_a_classifier_head(gemm, tol):
    """First-step gradients of every parameter and of the input against fp64 autograd of the torch.cat restatement, per tensor
    |got - ref| <= 14 (n + 2) 2^-24 * 8 * max|ref| with n = B T rows (the bound tests/test_gpu_tdnn_grad.py derives); export() against the
    module's eval output."""
    t = R.TRAIN
    mdl, feats = R.train_model(ktf)
    mdl.gemm = gemm
    lens, B, T, D = t["lens"], t["B"], t["T"], t["D"]
    buf = torch.zeros((B, T, 32), device=DEV)
    buf[:, :, :D] = torch.as_tensor(feats)
    dl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    torch.manual_seed(5)
    net = ktf.autograd.TrainableSequential(mdl, device=DEV, gemm=gemm).train()
    head = ktf.autograd.ClassifierHead(t["EMB"], 4, kind="aam", margin=0.2, scale=16.0, gemm=gemm, device=DEV)
    tf_ = torch.tensor(feats, device=DEV, requires_grad=True)
    labels = torch.arange(B) % 4
    params = [tf_] + list(net.params) + [head.weight]
    assert all(np.array_equal(p.detach().cpu().numpy(), q) for p, q in zip(net.params, R.train_params(mdl)))
    ref = [p.detach().cpu().to(torch.float64).requires_grad_(True) for p in params]
    got = mdl.run_ragged(buf[:, :, :D], dl).cpu().numpy()[:, 0]
    loss, _ = head(net(tf_, dl), labels.to(DEV))
    loss.backward()
    emb = R.restated(mdl, ref[1:-1], ref[0], lens)
    ref_loss = torch_loss(emb @ ref[-1].T, labels, torch_inv_norm(emb, 1e-12), torch_inv_norm(ref[-1], 1e-12), "aam", 0.2, 16.0).mean()
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
    factor = 14 * (B * T + 2) * 2.0 ** -24 * 8
    worst = []
    for i, (p, r) in enumerate(zip(params, ref)):
        err, top = float((p.grad.cpu().to(torch.float64) - r.grad).abs().max()), float(r.grad.abs().max())
        print(f"{gemm} tensor {i} {tuple(p.shape)}: max |err| {err:.3e}, max |ref| {top:.3e}, bound {factor * top:.3e}")
        worst.append((err, factor * top, i))
    assert all(bound > 0 and err <= bound for err, bound, _ in worst), worst
    with torch.no_grad():
        for p in net.params:
            p -= 0.01 * p.grad
        stepped = net.eval()(tf_.detach(), dl).cpu().numpy()
    assert net.export() is mdl and np.array_equal(mdl.get_layer("mfa").kernel.T, net.params[net.steps[3][2]].detach().cpu().numpy())
    again = mdl.run_ragged(buf[:, :, :D], dl).cpu().numpy()[:, 0]
    print(f"{gemm} export: max |inference - eval| {np.abs(again - stepped).max():.3e}")
    assert np.abs(again - stepped).max() < tol * max(1.0, np.abs(stepped).max()) and np.abs(again - got).max() > 0
