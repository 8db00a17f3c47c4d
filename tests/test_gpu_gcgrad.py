"""The gradient of global-context attention on the GPU (include/ktf_gcgrad.h) against tests/_gcgrad_ref.py within k u S of rule 9, its
independence of layout, batch and repetition bit for bit, and a model trained through TrainableSequential(global_context=True)."""

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
import _gcgrad_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, SENT, EPS = float("nan"), 7.0, 1e-5
MODES = {"f32": L.GEMM_F32, "bf16x3": L.GEMM_BF16X3}
ACTS = {"tanh": L.ACT_TANH, "relu": L.ACT_RELU}
TILE = 64
# D, A and H each beside a multiple of 32 once, the extremes of each, and T in {1, R - 1, R + 1, 2 R + 3} twice
SHAPES = [(1, 1, 1, 1), (33, 33, 1, TILE - 1), (130, 1, 130, TILE + 1), (1, 256, 1, 2 * TILE + 3), (33, 256, 130, 1), (130, 33, 1, TILE - 1),
          (31, 64, 33, TILE + 1), (96, 128, 32, 2 * TILE + 3)]


def _rows(a, pad=0, off=0, fill=NAN):
    """a (..., C) as a device tensor (..., C + pad) whose base lies `off` floats behind a 256-byte boundary; pad columns = fill."""
    a = np.asarray(a, np.float32)
    C, n = a.shape[-1], int(np.prod(a.shape[:-1]))
    buf = torch.full((n * (C + pad) + 8,), fill, dtype=torch.float32, device=DEV)
    v = buf[off:off + n * (C + pad)].view(*a.shape[:-1], C + pad)
    v[..., :C] = torch.as_tensor(a, device=DEV)
    return v


def run(c, lens, act, mode, pad=0, off=0):
    """The three calls on the operands of case c laid out with `pad` extra columns and a base `off` floats off alignment; NaN in every
    row at or beyond an utterance's length and in every pad column of the inputs, a sentinel in the pad columns of the outputs."""
    B, T, D = c["x"].shape
    A, H = c["w2"].shape
    x, de, dx0 = c["x"].copy(), c["de"].copy(), c["dx_in"].copy()
    for b, n in enumerate(lens):
        x[b, n:], de[b, n:], dx0[b, n:] = NAN, NAN, SENT
    tl = torch.as_tensor(np.asarray(lens, np.int32), device=DEV)
    tx, tde, w1, w2 = (_rows(a, pad, off) for a in (x, de, c["w1"], c["w2"]))
    vx, w1x, w1c = tx[..., :D], w1[:D, :A], w1[D:, :A]
    ctx = ops.gctx_stats(vx, tl, EPS, torch.zeros((B, 2, D), dtype=torch.float64, device=DEV))
    g = _rows(np.zeros((B, A)), pad, off)
    ops.gctx_bias(ctx, w1c, torch.as_tensor(c["b1"], device=DEV), g[:, :A])
    dz, h, dx, dw1c = (_rows(a, pad + 1, off, SENT) for a in (np.full((B, T, A), SENT), np.full((B, T, A), SENT), dx0, np.full((2 * D, A), SENT)))
    ops.gcgrad_hidden(vx, tl, w1x, g[:, :A], ACTS[act], w2[:, :H], MODES[mode], tde[..., :H], dz[..., :A], h[..., :A])
    db1 = torch.full((A,), SENT, device=DEV)
    coef = torch.full((B, 2, D), SENT, dtype=torch.float64, device=DEV)
    ops.gcgrad_context(dz[..., :A], tl, ctx, w1c, EPS, dw1c[:, :A], db1, coef, ops.gcgrad_workspace(B, A, DEV))
    ops.gcgrad_data(dz[..., :A], tl, w1x, vx, ctx, coef, MODES[mode], dx[..., :D])
    torch.cuda.synchronize()
    for name, t, C in (("dz", dz, A), ("h", h, A), ("dx", dx, D), ("dw1c", dw1c, A)):
        assert bool((t[..., C:] == SENT).all()), f"{name}: a pad column was written"
    return {k: v.cpu().numpy() for k, v in dict(dz=dz[..., :A], h=h[..., :A], dx=dx[..., :D], dw1c=dw1c[:, :A], db1=db1, coef=coef).items()}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_kernels_within_k_u_s_of_the_reference(i, mode):
    D, A, H, T = SHAPES[i]
    act = ("tanh", "relu")[i % 2]
    assert ops.gcgrad_row_tile(A, H, MODES[mode]) == TILE
    lens = sorted({0, 1, min(37, T), T})
    c = R.case(D, A, H, T, lens)
    got = run(c, lens, act, mode, pad=1)
    ref = [R.utterance(c["x"][b], n, c["w1"], c["b1"], c["w2"], c["de"][b], act, EPS, c["dx_in"][b]) for b, n in enumerate(lens)]
    u, worst = R.U[mode], {}

    def check(name, g, v, S):
        ratio = float((np.abs(g - v) / np.maximum(R.K[name] * u * S, 1e-300)).max()) if v.size else 0.0
        worst[name] = max(worst.get(name, 0.0), ratio)

    for b, n in enumerate(lens):
        for name in ("dz", "h", "dx"):
            check(name, got[name][b, :n], *ref[b][name])
        check("coef", got["coef"][b], *ref[b]["coef"])
        assert not got["dz"][b, n:].any() and not got["h"][b, n:].any() and (got["dx"][b, n:] == SENT).all()
    for name in ("dw1c", "db1"):
        check(name, got[name], sum(r[name][0] for r in ref), sum(r[name][1] for r in ref))
    print(f"D={D} A={A} H={H} T={T} {act} {mode}: max |err| / (k u S) " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert (got["coef"][0] == 0).all() and (got["coef"][:, 1, 0] == 0).all()      # (the empty utterance; the constant channel)


@pytest.mark.parametrize("mode,act", [("f32", "tanh"), ("bf16x3", "relu")])
def test_bits_do_not_depend_on_layout_batch_or_repetition(mode, act):
    D, A, H, T = 96, 64, 32, 2 * TILE + 3                     # (multiples of 32: the aligned layouts take the DMA feed)
    lens = [T, 5, 0, 70, TILE, 1, TILE + 1]
    c = R.case(D, A, H, T, lens)
    base = run(c, lens, act, mode)
    for pad, off in ((0, 0), (3, 0), (4, 0), (0, 1)):
        again = run(c, lens, act, mode, pad, off)
        for k in base:
            assert np.array_equal(base[k].view(np.uint8), again[k].view(np.uint8)), (k, pad, off)
    for b in (3, 6):
        alone = run({k: (v[b:b + 1] if k in ("x", "de", "dx_in") else v) for k, v in c.items()}, [lens[b]], act, mode)
        for k in ("dz", "h", "dx", "coef"):
            assert np.array_equal(base[k][b].view(np.uint8), alone[k][0].view(np.uint8)), (k, b)


CFG = {"layers": [{"type": "input", "shape": [None, None, 24]}, {"name": "t1", "type": ["tdnn", "relu"], "cfg": {"units": 32, "context": [-1, 0, 1]}},
                  {"name": "ctxpool", "type": "attentive_stats", "cfg": {"attention_units": 8, "heads": 4, "global_context": True, "epsilon": 1e-5}},
                  {"name": "emb", "type": "tdnn", "cfg": {"units": 6, "context": [0]}}]}
TRAIN_LENS = [40, 90, 57, 64, 65, 71]


@pytest.mark.parametrize("mode", list(MODES))
def test_training_step_gradients_and_export(mode):
    """First-step gradients of every parameter and of the features against fp64 autograd of the torch composition, within the bound of
    test_gpu_attn.py's training test: 16 stages * (n + 2) * 2^-24 * 8 * max |ref|, n = 6 * 90 rows (b2 as there: a softmax does not see a
    shift of its logits, so its scale is what the sum is made of); after an SGD step and export() the inference model reproduces the
    module in eval mode within the same factor."""
    from test_attn_cpu import torch_pool
    from test_tdnn_grad_cpu import restated_tdnn
    F64 = torch.float64
    seq = ktf.models.SequentialFromConfig(CFG, None, "gcgrad", gemm=mode)
    rng = np.random.default_rng(3)
    feats = rng.standard_normal((len(TRAIN_LENS), max(TRAIN_LENS), 24)).astype(np.float32)
    gout = torch.as_tensor(rng.standard_normal((len(TRAIN_LENS), 6)).astype(np.float32), device=DEV)
    net = ktf.autograd.TrainableSequential(seq, gemm=mode, global_context=True).train()
    tf_ = torch.as_tensor(feats, device=DEV).requires_grad_(True)
    tl = torch.as_tensor(TRAIN_LENS, device=DEV)
    (net(tf_, tl) * gout).sum().backward()

    params = list(net.params)
    w0, b0, w1, b1, w2, b2, w3, b3 = ref = [p.detach().cpu().to(F64).requires_grad_(True) for p in params]
    rf = torch.tensor(feats, dtype=F64, requires_grad=True)
    x = torch.relu(restated_tdnn(rf, w0, b0, TRAIN_LENS, [-1, 0, 1], 1, "SAME"))
    pooled, es = [], []
    for b, n in enumerate(TRAIN_LENS):
        xb = x[b, :n]
        mu = xb.mean(0)
        sigma = ((xb * xb).mean(0) - mu * mu).clamp(min=0).add(float(np.float32(1e-5))).sqrt()
        e = torch.tanh(torch.cat([xb, mu.expand(n, 32), sigma.expand(n, 32)], 1) @ w1 + b1) @ w2 + b2
        e.retain_grad()
        es.append(e)
        pooled.append(torch_pool(x[b], torch.cat([e, e.new_zeros(x.shape[1] - n, 4)]), n, True, 1e-5))
    ((torch.stack(pooled) @ w3[:, 0, :].T + b3) * gout.cpu().to(F64)).sum().backward()
    factor = 16 * (len(TRAIN_LENS) * max(TRAIN_LENS) + 2) * 2.0 ** -24 * 8
    for i, (g, r) in enumerate(zip([p.grad for p in params] + [tf_.grad], [r.grad for r in ref] + [rf.grad])):
        err, scale = float((g.cpu().to(F64) - r).abs().max()), float(r.abs().max())
        if i == 5:
            scale = float(torch.cat([e.grad.abs() for e in es]).sum(0).max()) / 8
        print(f"{mode} tensor {i} {tuple(g.shape)}: max |err| {err:.3e}, max |ref| {scale:.3e}, bound {factor * scale:.3e}")
        assert scale > 0 and err <= factor * scale, (mode, i, err, factor * scale)

    with torch.no_grad():
        for p in params:
            p -= 0.05 * p.grad
    assert net.export() is seq
    for a, p in zip(seq.get_layer("ctxpool").get_weights(), params[2:6]):
        assert np.array_equal(a.view(np.uint32), p.detach().cpu().numpy().view(np.uint32))
    with torch.no_grad():
        want = net.eval()(tf_.detach(), tl).cpu().numpy()
    seq.min_tiles, seq.min_frames = {}, {}
    got = seq.run_ragged(ktf.models._padded_copy(tf_.detach(), torch.float32), tl.to(torch.int32)).float().cpu().numpy().reshape(len(TRAIN_LENS), -1)
    d = np.abs(got - want).max() / max(1.0, np.abs(want).max())
    print(f"{mode}: exported model against the module in eval mode: {d:.3e} (limit {factor:.3e})")
    assert d <= factor
