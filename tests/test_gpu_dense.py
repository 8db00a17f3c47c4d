"""The dense affine kernels (include/ktf_dense.h) on the GPU against a plain fp64 numpy matmul of the operands each mode multiplies.
Bounds, with S = sum |term| of an element and n the fp32 additions into it (forward: D; data gradient: N plus the number of slots;
weight gradient: M): (n + 2) u S for "f32" and for "bf16" on its rounded operands, (3 n + 2) u 1.02 S + X3_OPERANDS S for "bf16x3",
u = 2^-24 (tests/_tdnn_grad_ref.py, tests/_tdnn_grad16_ref.py); dbias is an fp64 sum rounded once: 1.01 u sum |g|."""

import numpy as np
import pytest
import torch

from kaldi_tflite_amd import _lib as L, autograd as A, ops           # (tests/conftest.py puts the package and tests/ on sys.path)
from _tdnn16_ref import X3_OPERANDS, bf16_rne
from test_gpu_loss import _labels, head_reference

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DEV = "cuda:0"
NAN = float("nan")
_bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
SLOT = 256
MODES = {"f32": L.GEMM_F32, "bf16": L.GEMM_BF16, "bf16x3": L.GEMM_BF16X3}
# (M, N, D) around the tiles (32; 64 from 512 tiles of 64 x 64 on: the last two, in all three calls), the step 32 and the slots
EDGES = [(1, 1, 1), (31, SLOT - 1, 31), (32, SLOT, 32), (33, SLOT + 1, 33), (63, 2 * SLOT + 3, 1), (64, SLOT - 1, 64), (65, 1, 65),
         (1, SLOT + 1, 32), (32, 1, 33), (33, 2 * SLOT + 3, 31), (64, 128 * SLOT + 1, 256), (65, 128 * SLOT + 1, 65)]
VALUES = [(33, 2 * SLOT + 3, 31), (64, SLOT - 1, 64), (65, 128 * SLOT + 1, 65)]


def _wide(rows, cols, odd, offset, values=None):
    """A (rows, cols) view `offset` floats into a NaN-filled buffer and its (rows, ld) parent; holding `values` if given. `odd`: the
    leading dimension is the next odd number above cols, so that rows cycle through every 4-byte alignment; otherwise it is cols."""
    pad = (1 + cols % 2) if odd else 0
    parent = torch.full((offset + rows * (cols + pad),), NAN, device=DEV)[offset:].view(rows, cols + pad)
    view = parent[:, :cols]
    if values is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32)))
    return view, parent


def run(mode, x, w, b, g, odd=False, offset=0):
    """The three calls on operands and outputs placed by _wide -> numpy; every output pad column must be zero."""
    (M, D), N = x.shape, w.shape[0]
    tx, tw, tg = (_wide(*a.shape, odd, offset, a)[0] for a in (x, w, g))
    outs = {"z": _wide(M, N, odd, offset), "dx": _wide(M, D, odd, offset), "dw": _wide(N, D, odd, offset)}
    db = torch.full((N,), NAN, device=DEV)
    ops.dense_forward(tx, tw, torch.from_numpy(b).to(DEV), MODES[mode], outs["z"][0])
    ops.dense_grad_data(tg, tw, MODES[mode], outs["dx"][0], ops.dense_workspace(M, N, D, DEV))
    ops.dense_grad_weights(tg, tx, MODES[mode], outs["dw"][0], db)
    got = {"db": db.cpu().numpy()}
    for k, (view, parent) in outs.items():
        got[k] = view.cpu().numpy()
        assert not parent[:, view.shape[1]:].cpu().numpy().any(), k
    return got


def reference(mode, x, w, b, g):
    """fp64 results of the operands `mode` multiplies and the bounds of the docstring."""
    q = bf16_rne if mode == "bf16" else np.asarray
    xq, wq, gq = (q(a).astype(np.float64) for a in (x, w, g))
    (M, D), N = x.shape, w.shape[0]
    acc = (lambda n: (3 * n + 2) * U * 1.02 + X3_OPERANDS) if mode == "bf16x3" else (lambda n: (n + 2) * U)
    want = {"z": xq @ wq.T + b, "dx": gq @ wq, "dw": gq.T @ xq, "db": g.astype(np.float64).sum(0)}
    bound = {"z": acc(D) * (np.abs(xq) @ np.abs(wq).T + np.abs(b)), "dx": acc(N - (-N // SLOT)) * (np.abs(gq) @ np.abs(wq)),
             "dw": acc(M) * (np.abs(gq).T @ np.abs(xq)), "db": 1.01 * U * np.abs(g).sum(0)}
    return want, bound


def operands(M, N, D, integers):
    rng = np.random.default_rng(M + 7 * N + 13 * D)
    draw = (lambda *s: rng.integers(-4, 5, s).astype(np.float32)) if integers else (lambda *s: rng.standard_normal(s).astype(np.float32))
    return draw(M, D), draw(N, D), draw(N), draw(M, N)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("M,N,D", EDGES)
def test_small_integers_are_exact_at_every_edge(M, N, D, mode):
    """Every product and sum is exact in bf16 and fp32: all three calls equal the fp64 reference bit for bit, dbias included."""
    ops_ = operands(M, N, D, integers=True)
    got, (want, _) = run(mode, *ops_), reference(mode, *ops_)
    for k in want:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("M,N,D", VALUES)
def test_gaussian_values_determinism_and_placement(M, N, D, mode):
    ops_ = operands(M, N, D, integers=False)
    got, (want, bound) = run(mode, *ops_), reference(mode, *ops_)
    ratios = {k: float((np.abs(got[k] - want[k]) / bound[k]).max()) for k in want}
    print(f"dense {mode} {(M, N, D)}: worst |err| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    again, placed = run(mode, *ops_), run(mode, *ops_, odd=True, offset=5)                  # odd leading dimensions, 4-byte-aligned bases
    for k in want:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), k
        assert np.array_equal(_bits(got[k]), _bits(placed[k])), k


def test_bf16_ties_round_to_even():
    x, w = np.float32([[1 + 2.0 ** -8]]), np.float32([[1 + 3 * 2.0 ** -8]])             # -> 1 (down) and 1 + 2^-6 (up): the even neighbours
    got = run("bf16", x, w, np.float32([0]), np.float32([[1]]))
    assert got["z"][0, 0] == np.float32(1 + 2.0 ** -6) and got["dx"][0, 0] == np.float32(1 + 2.0 ** -6) and got["dw"][0, 0] == 1.0


@pytest.mark.parametrize("expanded", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_autograd_against_fp64_torch(mode, expanded, monkeypatch):
    """expanded: the loss goes through z.sum(0), which hands the backward a gradient of row stride 0 (copied, not read as M rows)."""
    M, N, D = 33, 2 * SLOT + 3, 31
    q = bf16_rne if mode == "bf16" else np.asarray                 # "bf16" on operands it leaves as they are: torch rounds nothing
    x, w, b, g = (q(a) for a in operands(M, N, D, integers=False))
    g = np.ascontiguousarray(np.broadcast_to(g[:1], g.shape)) if expanded else g
    loss = (lambda z, gt: (z.sum(0) * gt[0]).sum()) if expanded else (lambda z, gt: (z * gt).sum())
    t64 = [torch.from_numpy(a).double().requires_grad_(True) for a in (x, w, b)]
    loss(t64[0] @ t64[1].T + t64[2], torch.from_numpy(g).double()).backward()
    t32 = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in (x, w, b)]
    z = A.dense_affine(*t32, gemm=mode)
    loss(z, torch.from_numpy(g).to(DEV)).backward()
    want, bound = reference(mode, x, w, b, g)
    for k, a, t in zip(("dx", "dw", "db"), t64, t32):
        assert np.abs(a.grad.numpy() - want[k]).max() <= 1e-9
        assert (np.abs(t.grad.cpu().numpy() - want[k]) <= bound[k]).all(), k
    assert (np.abs(z.detach().cpu().numpy() - want["z"]) <= bound["z"]).all()
    # only the gradients that are asked for
    calls = []
    monkeypatch.setattr(ops, "dense_grad_weights", lambda *a, **k: calls.append(a))
    tx, tw = torch.from_numpy(x).to(DEV).requires_grad_(True), torch.from_numpy(w).to(DEV)
    loss(A.dense_affine(tx, tw, gemm=mode), torch.from_numpy(g).to(DEV)).backward()
    assert not calls and tw.grad is None and (np.abs(tx.grad.cpu().numpy() - want["dx"]) <= bound["dx"]).all()


@pytest.mark.parametrize("kind", ["aam", "softmax"])
@pytest.mark.parametrize("mode", list(MODES))
def test_classifier_head_on_the_dense_route(mode, kind):
    B, D, N = 19, 64, 300
    rng = np.random.default_rng(21)
    torch.manual_seed(21)
    x, labels = rng.standard_normal((B, D)).astype(np.float32), _labels(B, N, rng)
    head = A.ClassifierHead(D, N, kind=kind, gemm=mode, normalize=True, device=DEV, affine="dense")
    ref = head_reference(x, head.weight.detach().cpu().numpy(), labels, kind, head.margin, head.scale, mode)
    emb = torch.from_numpy(x).to(DEV).requires_grad_(True)
    loss, pred = head(emb, torch.from_numpy(labels).to(DEV))
    loss.backward()
    assert abs(loss.item() - ref["loss"]) <= ref["loss_bound"]
    for k, t in (("dx", emb), ("dw", head.weight)):
        assert (np.abs(t.grad.cpu().numpy() - ref[k]) <= ref[k + "_bound"]).all(), k
    sure = ref["gap"] > 1e-3
    assert np.array_equal(pred.cpu().numpy()[sure], ref["pred"][sure])


def test_sub_centre_head_equals_the_tdnn_route_on_integers():
    """Integer-valued operands: both routes' logits are exact, so everything behind them is the same."""
    B, D, N, K = 19, 64, 300, 2
    rng = np.random.default_rng(5)
    w = rng.integers(-3, 4, (N * K, D)).astype(np.float32)
    w[:, 0] = 1.0                                                  # no zero row
    emb, labels = torch.from_numpy(rng.integers(-3, 4, (B, D)).astype(np.float32)).to(DEV), torch.from_numpy(_labels(B, N, rng)).to(DEV)
    seen = {}
    for affine in ("tdnn", "dense"):
        head = A.ClassifierHead(D, N, sub_centers=K, top_k=3, penalty=0.06, label_smoothing=0.1, device=DEV, affine=affine)
        with torch.no_grad():
            head.weight.copy_(torch.from_numpy(w))
        seen[affine] = (head(emb, labels)[1].cpu().numpy(), head.center_counts.cpu().numpy())
    assert seen["dense"][1].sum() > 0 and all(np.array_equal(a, b) for a, b in zip(seen["dense"], seen["tdnn"]))
    assert head.dominant().affine == "dense"
