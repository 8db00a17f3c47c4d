"""The head's loss with sub-centres, the inter-top-k penalty and label smoothing without a GPU: the fp64 oracle (tests/_head_ref.py)
against fp64 torch.autograd of a torch restatement and against tests/_loss_ref.py, hand-computed values on every branch of H2 and H3,
the C-ABI of include/ktf_head.h (symbols, argument refusals before any launch, the workspace size) and the host side of
ktf.autograd.margin_softmax_loss / ClassifierHead (argument checks, center_counts, dominant())."""

import ctypes as C
import math
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
import _head_ref as H  # noqa: E402
import _loss_ref as R  # noqa: E402
from test_loss_cpu import FLOOR, _close, _head_inputs, _refused, torch_inv_norm  # noqa: E402

F64 = torch.float64
BIAS = 1e-9            # the index bias of the restatement's top-k: distinct cosines are asserted to lie further apart than N * BIAS


# ----------------------------------------------------------------------------- the oracle
def torch_head_loss(z, labels, ix, iw, kind, margin, scale, K=1, topk=0, penalty=0.0, eps=0.0):
    """The rules of ktf_head.h in torch ops, for autograd: per-row losses (B,). `amax` over the centres, `topk` over the class
    cosines with the target masked and the tie rule (the lower class first) enforced by a tiny bias, smoothed cross entropy."""
    B, N = z.shape[0], z.shape[1] // K
    ck = z if ix is None else z * ix[:, None] * iw[None, :]
    c = ck.view(B, N, K).amax(dim=2)
    valid = (labels >= 0) & (labels < N)
    y = labels.clamp(0, N - 1)[:, None]
    cy = c.gather(1, y)[:, 0]
    if kind == "am":
        py = cy - margin
    elif kind == "aam":
        cm, sm = math.cos(margin), math.sin(margin)
        py = torch.where(cy > -cm, cy * cm - torch.sqrt(torch.clamp(1.0 - cy * cy, min=FLOOR)) * sm, cy - margin * sm)
    else:
        py = cy
    ly = scale * torch.where(valid, py, cy)
    pen = torch.zeros_like(c)
    n = min(topk, N - 1)
    if n > 0:
        key = (c.detach() - BIAS * torch.arange(N, dtype=c.dtype)[None, :]).scatter(1, y, -float("inf"))
        pen = pen.scatter(1, key.topk(n, dim=1).indices, penalty) * valid[:, None]
    logits = (scale * (c + pen)).scatter(1, y, ly[:, None])
    smooth = (1.0 - eps) * ly + eps * logits.mean(dim=1)
    return torch.where(valid, torch.logsumexp(logits, dim=1) - smooth, torch.zeros((), dtype=z.dtype))


KINDS = [("softmax", 0.0, 12.0), ("am", 0.25, 16.0), ("aam", 0.3, 16.0)]


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("topk", [0, 1, 5])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("kind,margin,scale", KINDS)
def test_oracle_equals_autograd_of_the_torch_restatement(kind, margin, scale, K, topk, eps):
    """Loss and gradients in z and in both norms, and through the norms in x and w."""
    rng = np.random.default_rng(100 * K + topk)
    N, pen, e0 = 11, (0.06 if topk else 0.0), 1e-12
    x, w = rng.standard_normal((7, 5)), rng.standard_normal((N * K, 5))
    labels = np.array([0, N - 1, 4, 5, -1, N, 3])
    gloss = rng.standard_normal(7)
    gloss[1] = 0.0
    # class-major rows: the targets of rows 2 and 3 (classes 4 and 5) have cosines near -1 (every centre of class 4 lies close to
    # the first, apart enough for no tie) and near +1 (the last centre of class 5)
    for k in range(1, K):
        w[4 * K + k] = w[4 * K] + 0.03 * k * rng.standard_normal(5)
    x[2] = -3.0 * w[4 * K]
    x[3] = 2.0 * w[5 * K + K - 1] + 0.5 * rng.standard_normal(5)
    nx, nw = R.inv_norm(x, e0), R.inv_norm(w, e0)
    z = x @ w.T
    f = H.forward(z, labels, nx["inv"], nw["inv"], kind, margin, scale, K, topk, pen, eps)
    g = H.backward(z, labels, nx["inv"], nw["inv"], kind, margin, scale, K, topk, pen, eps, f["lse"], f["hard"], gloss)
    assert list(f["valid"]) == [True, True, True, True, False, False, True]
    flat = np.sort(f["c"], axis=1)
    assert (np.diff(flat, axis=1) > 10 * N * BIAS).all()          # no near-ties: the biased top-k of the restatement is the rule
    if kind == "aam":
        assert f["c"][2, 4] < -math.cos(margin) < f["c"][3, 5]
        for b in np.flatnonzero(f["valid"]):
            cy = f["c"][b, labels[b]]
            assert abs(cy + math.cos(margin)) > 1e-3 and abs(cy - math.sqrt(1.0 - FLOOR)) > 1e-3
    if K > 1:
        assert len(set(f["kstar"].reshape(-1))) == K and f["sub_y"][4] == f["sub_y"][5] == -1
    assert (f["hard"][4] == -1).all() and (f["hard"][5] == -1).all()
    assert ((f["hard"][f["valid"]][:, :min(topk, N - 1)] >= 0).all()) and (f["hard"][:, min(topk, N - 1):] == -1).all()

    tx, tw = torch.tensor(x, dtype=F64, requires_grad=True), torch.tensor(w, dtype=F64, requires_grad=True)
    tz, tix, tiw = tx @ tw.T, torch_inv_norm(tx, e0), torch_inv_norm(tw, e0)
    for t in (tz, tix, tiw):
        t.retain_grad()
    loss = torch_head_loss(tz, torch.tensor(labels), tix, tiw, kind, margin, scale, K, topk, pen, eps)
    (loss * torch.tensor(gloss)).sum().backward()
    _close(f["loss"], loss.detach().numpy(), "loss")
    _close(g["dz"], tz.grad.numpy(), "dz")
    _close(g["dinv_x"], tix.grad.numpy(), "dinv_x")
    _close(g["dinv_w"], tiw.grad.numpy(), "dinv_w")
    dx = g["dz"] @ w + R.inv_norm_backward(x, e0, nx["inv"], g["dinv_x"])
    dw = g["dz"].T @ x + R.inv_norm_backward(w, e0, nw["inv"], g["dinv_w"])
    _close(dx, tx.grad.numpy(), "dx")
    _close(dw, tw.grad.numpy(), "dw")
    assert (g["dz_mag"] >= np.abs(g["dz"]) * (1 - 1e-12)).all()
    assert (g["dinv_x_abs"] >= np.abs(g["dinv_x"]) - 1e-12).all() and (g["dinv_w_abs"] >= np.abs(g["dinv_w"]) - 1e-12).all()
    assert not g["dz"][:, ~g["selected"]].any() and not g["dinv_w"][~g["selected"]].any() and not g["dz"][[1, 4, 5]].any()
    assert np.array_equal(f["pred"], np.argmax(f["c"], axis=1))


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_plain_head_with_smoothing_equals_autograd(eps):
    rng = np.random.default_rng(3)
    z, labels, gloss = 3.0 * rng.standard_normal((6, 9)), np.array([0, 8, -1, 9, 4, 4]), rng.standard_normal(6)
    f = H.forward(z, labels, None, None, "softmax", 0.0, 1.5, 1, 0, 0.0, eps)
    g = H.backward(z, labels, None, None, "softmax", 0.0, 1.5, 1, 0, 0.0, eps, f["lse"], f["hard"], gloss)
    tz = torch.tensor(z, dtype=F64, requires_grad=True)
    loss = torch_head_loss(tz, torch.tensor(labels), None, None, "softmax", 0.0, 1.5, eps=eps)
    (loss * torch.tensor(gloss)).sum().backward()
    _close(f["loss"], loss.detach().numpy(), "loss")
    _close(g["dz"], tz.grad.numpy(), "dz")
    ce = torch.nn.functional.cross_entropy(1.5 * torch.tensor(z), torch.tensor(labels).clamp(-1, 8).where(torch.tensor(labels) < 9, torch.tensor(-1)),
                                           ignore_index=-1, label_smoothing=eps, reduction="none")
    _close(f["loss"], ce.numpy(), "torch's label_smoothing")


@pytest.mark.parametrize("kind,margin,scale,cosine", [("softmax", 0.0, 1.0, False), ("softmax", 0.0, 12.0, True), ("am", 0.25, 16.0, True),
                                                      ("aam", 0.3, 16.0, True)])
def test_with_everything_off_the_oracle_is_that_of_the_plain_loss(kind, margin, scale, cosine):
    rng = np.random.default_rng(11)
    x, w, labels, gloss = _head_inputs(kind, margin, rng)
    z = x @ w.T
    ix = R.inv_norm(x, 1e-12)["inv"] if cosine else None
    iw = R.inv_norm(w, 1e-12)["inv"] if cosine else None
    f, f0 = H.forward(z, labels, ix, iw, kind, margin, scale), R.forward(z, labels, ix, iw, kind, margin, scale)
    for k in ("loss", "lse", "ly", "pred", "valid", "c"):
        assert np.array_equal(f[k], f0[k]), k
    g = H.backward(z, labels, ix, iw, kind, margin, scale, 1, 0, 0.0, 0.0, f["lse"], f["hard"], gloss)
    g0 = R.backward(z, labels, ix, iw, kind, margin, scale, f0["lse"], gloss)
    for k in g0:
        assert np.array_equal(g[k], g0[k]), k
    assert (f["hard"] == -1).all() and f["hard"].shape == (7, 1) and list(f["sub_y"]) == [0, 0, 0, 0, -1, -1, 0]


def test_every_branch_of_the_rules_by_hand():
    one = np.ones(1)
    # H1: two classes of two centres; ties between centres take the lower k; lse and pred run over classes
    z = np.array([[0.5, 0.5, 0.25, 0.75]])
    f = H.forward(z, [0], one, np.ones(4), "softmax", 0.0, 2.0, K=2)
    assert list(f["c"][0]) == [0.5, 0.75] and list(f["kstar"][0]) == [0, 1] and f["sub_y"][0] == 0 and f["pred"][0] == 1
    assert f["lse"][0] == 1.5 + math.log(math.exp(1.0 - 1.5) + 1.0) and f["loss"][0] == f["lse"][0] - 1.0
    g = H.backward(z, [0], one, np.ones(4), "softmax", 0.0, 2.0, 2, 0, 0.0, 0.0, f["lse"], f["hard"])
    p = np.exp(np.array([1.0, 1.5]) - f["lse"][0])
    assert np.array_equal(g["dz"][0], [2.0 * (p[0] - 1.0), 0.0, 0.0, 2.0 * p[1]]) and list(g["selected"]) == [True, False, False, True]
    assert g["dinv_w"][1] == 0.0 == g["dinv_w"][2] and g["dinv_w"][3] == (2.0 * p[1]) * 0.75
    assert g["dinv_x"][0] == np.sum(g["dz"][0] * z[0])

    # H2: four classes, target 1 holds the largest cosine and is never a member; 0 and 3 tie: the lower class first
    c = np.array([[0.25, 0.9, -0.5, 0.25]])
    w4 = np.ones(4)
    for topk, want in ((0, [-1]), (1, [0]), (2, [0, 3]), (3, [0, 3, 2]), (5, [0, 3, 2, -1, -1]), (64, [0, 3, 2] + [-1] * 61)):
        f = H.forward(c, [1], one, w4, "am", 0.125, 4.0, topk=topk, penalty=0.0625 if topk else 0.0)
        assert list(f["hard"][0]) == want, topk
        l = [4.0 * (0.25 + (0.0625 if 0 in want else 0.0)), 4.0 * (0.9 - 0.125), 4.0 * (-0.5 + (0.0625 if 2 in want else 0.0)),
             4.0 * (0.25 + (0.0625 if 3 in want else 0.0))]
        assert list(f["l"][0]) == l and f["pred"][0] == 1
        assert f["loss"][0] == f["lse"][0] - l[1]
    assert list(H.forward(c, [0], one, w4, "am", 0.125, 4.0, topk=2, penalty=0.1)["hard"][0]) == [1, 3]    # a tie across the target
    assert list(H.forward(-0.0 * c + np.array([[0.0, 0.0, -0.0, 0.0]]), [3], one, w4, "am", 0.1, 4.0, topk=2, penalty=0.1)["hard"][0]) == [0, 1]
    ign = H.forward(c, [4], one, w4, "am", 0.125, 4.0, topk=2, penalty=0.0625)                              # ignored: no penalty
    assert list(ign["hard"][0]) == [-1, -1] and list(ign["l"][0]) == list(4.0 * c[0]) and ign["loss"][0] == 0 and ign["sub_y"][0] == -1
    # the penalty is additive: the derivative of a member's logit is `scale`
    f = H.forward(c, [1], one, w4, "am", 0.125, 4.0, topk=1, penalty=0.0625)
    g = H.backward(c, [1], one, w4, "am", 0.125, 4.0, 1, 1, 0.0625, 0.0, f["lse"], f["hard"])
    p = np.exp(f["l"][0] - f["lse"][0])
    assert np.array_equal(g["dz"][0], 4.0 * (p - np.array([0.0, 1.0, 0.0, 0.0])))
    # N = 1: an empty H_b, loss and dz exactly 0, with smoothing too
    f = H.forward(np.array([[0.3]]), [0], one, one, "aam", 0.2, 30.0, topk=3, penalty=0.1, eps=0.1)
    g = H.backward(np.array([[0.3]]), [0], one, one, "aam", 0.2, 30.0, 1, 3, 0.1, 0.1, f["lse"], f["hard"])
    assert list(f["hard"][0]) == [-1, -1, -1] and f["loss"][0] == 0.0 and g["dz"][0, 0] == 0.0

    # H3: two classes, e = 0.25 (exact in binary): loss = (lse - l_y) + e (l_y - mean), dc = g s ((p - hot) + e (hot - 1/N))
    z2 = np.array([[1.0, -1.0]])
    f = H.forward(z2, [0], None, None, "softmax", 0.0, 2.0, eps=0.25)
    lse = 2.0 + math.log(1.0 + math.exp(-4.0))
    assert f["lse"][0] == lse and f["lmean"][0] == 0.0 and f["loss"][0] == (lse - 2.0) + 0.25 * (2.0 - 0.0)
    assert abs(f["loss"][0] - (lse - (0.75 * 2.0 + 0.25 * 0.0))) <= 1e-15
    g = H.backward(z2, [0], None, None, "softmax", 0.0, 2.0, 1, 0, 0.0, 0.25, f["lse"], f["hard"], np.array([3.0]))
    p = np.exp(np.array([2.0, -2.0]) - lse)
    assert np.array_equal(g["dz"][0], [6.0 * ((p[0] - 1.0) + 0.25 * 0.5), 6.0 * (p[1] + 0.25 * -0.5)])
    assert abs(g["dz"][0].sum()) <= 1e-15                         # the smoothed target sums to one as the probabilities do


# ----------------------------------------------------------------------------- the C-ABI
def test_header_symbols_are_the_head_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_head.h")).read()
    code = hdr[hdr.index("#ifndef KTF_HEAD_H_"):]
    protos = re.findall(r"^(?:int|int32_t|int64_t) (ktf_[a-z0-9_]+)\(([^;]*)\);", code, flags=re.M)
    assert {n for n, _ in protos} == set(L.HEAD_PROTOTYPES) == set(re.findall(r"\b(ktf_[a-z0-9_]+)\s*\(", code))
    ctype = {"const float*": L._P, "float*": L._P, "const double*": L._P, "double*": L._P, "const int32_t*": L._P, "int32_t*": L._P,
             "void*": L._P, "int64_t": L._i64, "int32_t": L._i32, "double": C.c_double, "size_t": C.c_size_t}
    for name, args in protos:
        args = [a.strip() for a in args.replace("\n", " ").split(",")]
        want = [] if args == ["void"] else [ctype[a.rsplit(" ", 1)[0]] for a in args]
        assert L.HEAD_PROTOTYPES[name][1] == want, name
    assert all(n.startswith("ktf_head_") for n in L.HEAD_PROTOTYPES)
    lib = L.load()
    for name in L.HEAD_PROTOTYPES:
        assert hasattr(lib, name), name
    families = [L.PROTOTYPES, L.AUGMENT_PROTOTYPES, L.RESAMPLE_PROTOTYPES, L.GRAD_PROTOTYPES, L.NORM_PROTOTYPES, L.LOSS_PROTOTYPES,
                L.EGS_PROTOTYPES, L.OPTIM_PROTOTYPES]
    assert not set(L.HEAD_PROTOTYPES) & set().union(*families)
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "ktf_head.h":
            assert "ktf_head_" not in open(os.path.join(ROOT, "include", other)).read(), other
    for prefix in ("ktf_aug_", "ktf_rs_", "ktf_grad_", "ktf_norm_", "ktf_loss_", "ktf_egs_", "ktf_optim_"):
        assert prefix not in hdr, prefix
    assert len(L.PROTOTYPES) == 120 and lib.ktf_version() == 117 and len(L.LOSS_PROTOTYPES) == 6      # the existing families are as they were
    assert lib.ktf_head_slot_rows() == int(re.search(r"#define KTF_HEAD_SLOT_ROWS (\d+)", hdr).group(1)) == lib.ktf_loss_slot_rows()
    assert int(re.search(r"#define KTF_HEAD_MAX_CENTERS (\d+)", hdr).group(1)) == L.HEAD_MAX_CENTERS == H.MAX_CENTERS == 8
    assert int(re.search(r"#define KTF_HEAD_MAX_TOPK (\d+)", hdr).group(1)) == L.HEAD_MAX_TOPK == H.MAX_TOPK == 64
    assert int(re.search(r"#define KTF_HEAD_CHUNK_CLASSES (\d+)", hdr).group(1)) == 256


def test_argument_checks_without_gpu():
    lib = L.load()
    raw = (C.c_float * 16384)()
    buf = C.c_void_p((C.addressof(raw) + 255) & ~255)      # stands for any aligned non-null device pointer: every refusal comes before a launch
    far = C.c_void_p(buf.value + 32768)
    odd = C.c_void_p(buf.value + 4)
    B, N, K = 5, 6, 2
    need = lib.ktf_head_workspace_bytes(B, N, K)
    assert need > 0
    inf, nan = float("inf"), float("nan")

    def fwd(z=buf, ldz=12, B=B, N=N, K=K, labels=buf, inv_x=buf, inv_w=buf, kind=2, margin=0.2, scale=30.0, topk=5, penalty=0.06, eps=0.1,
            loss=buf, pred=buf, lse=buf, hard=buf, sub_y=buf, ws=buf, ws_bytes=None):
        return lib.ktf_head_forward(z, ldz, B, N, K, labels, inv_x, inv_w, kind, margin, scale, topk, penalty, eps, loss, pred, lse, hard,
                                    sub_y, ws, need if ws_bytes is None else ws_bytes, None)

    def bwd(z=buf, ldz=12, B=B, N=N, K=K, labels=buf, inv_x=buf, inv_w=buf, kind=2, margin=0.2, scale=30.0, topk=5, penalty=0.06, eps=0.1,
            lse=buf, hard=buf, gloss=None, dz=far, lddz=12, dinv_x=buf, dinv_w=buf, ws=buf, ws_bytes=None):
        return lib.ktf_head_backward(z, ldz, B, N, K, labels, inv_x, inv_w, kind, margin, scale, topk, penalty, eps, lse, hard, gloss, dz,
                                     lddz, dinv_x, dinv_w, ws, need if ws_bytes is None else ws_bytes, None)

    for name in ("z", "labels", "loss", "lse", "ws"):
        _refused(fwd(**{name: None}), "null")
    for name in ("z", "labels", "lse", "dz", "ws"):
        _refused(bwd(**{name: None}), "null")
    for fn, lds in ((fwd, ("ldz",)), (bwd, ("ldz", "lddz"))):
        plain = dict(inv_x=None, inv_w=None, K=1, topk=0, penalty=0.0, **({"dinv_x": None, "dinv_w": None} if fn is bwd else {}))
        # rule 10 of ktf_loss.h on these arguments
        _refused(fn(inv_x=None), "go together")
        _refused(fn(inv_w=None), "go together")
        _refused(fn(**dict(plain, kind=1)), "cosine head")
        _refused(fn(**dict(plain, kind=2)), "cosine head")
        _refused(fn(kind=0, margin=0.1), "margin must be 0")
        for bad in (0.0, -1.0, inf, nan):
            _refused(fn(scale=bad), "scale")
        for bad in (-0.1, inf, nan):
            _refused(fn(margin=bad), "margin")
        _refused(fn(margin=math.pi / 2), "pi / 2")
        for bad in (-1, 3, 7):
            _refused(fn(kind=bad), "unknown kind")
        _refused(fn(B=-1), "negative size")
        _refused(fn(N=0), "below 1")
        _refused(fn(B=1 << 31), "2^31")
        _refused(fn(N=1 << 30, **{ld: 1 << 31 for ld in lds}), "2^31")                   # N * K reaches 2^31
        _refused(fn(N=1 << 31, K=1, **{ld: 1 << 31 for ld in lds}), "2^31")
        _refused(fn(B=1 << 30, N=1 << 29, **{ld: 1 << 30 for ld in lds}), "too large")
        for ld in lds:
            _refused(fn(**{ld: 11}), "leading dimension")                                # below N * K = 12
            _refused(fn(**{ld: 1 << 31}), "2^31")
        _refused(fn(ws_bytes=need - 1), "workspace")
        _refused(fn(ws=odd), "256-byte")
        # H7
        for bad in (0, -1, 9):
            _refused(fn(K=bad, N=1), "K ")
        _refused(fn(**dict(plain, K=2, kind=0, margin=0.0)), "sub-centres")
        _refused(fn(**dict(plain, topk=1, kind=0, margin=0.0)), "topk > 0 needs")
        for bad in (-1, 65):
            _refused(fn(topk=bad), "topk")
        for bad in (-0.01, inf, nan):
            _refused(fn(penalty=bad), "penalty")
        _refused(fn(topk=0, penalty=0.06), "penalty must be 0")
        for bad in (-0.1, 1.0, 1.5, inf, nan):
            _refused(fn(eps=bad), "smoothing")
        _refused(fn(hard=None), "null hard")
        _refused(fn(topk=0, penalty=0.0, hard=None, ws_bytes=0), "workspace")            # a null hard is allowed then: the next refusal
        # smoothing alone is allowed on a plain head: the next refusal is the workspace's
        _refused(fn(**dict(plain, kind=0, margin=0.0, ws_bytes=0)), "workspace")
    _refused(bwd(dinv_x=None), "dinv_x")
    _refused(bwd(dinv_w=None), "dinv_x")
    _refused(bwd(kind=0, margin=0.0, inv_x=None, inv_w=None, K=1, topk=0, penalty=0.0), "dinv_x")
    _refused(bwd(dz=buf, lddz=16), "overlaps z")
    _refused(bwd(dz=odd), "overlaps z")
    _refused(bwd(dz=C.c_void_p(buf.value + 4 * ((B - 1) * 12 + N * K - 1))), "overlaps z")
    _refused(bwd(z=C.c_void_p(far.value + 4 * (B * 12 - 1))), "overlaps z")
    for bad in ((-1, 4, 1), (4, 0, 1), (1 << 31, 4, 1), (4, 1 << 31, 1), (4, 1 << 30, 2), (1 << 30, 1 << 30, 1), (4, 4, 0), (4, 4, 9)):
        assert lib.ktf_head_workspace_bytes(*bad) == -1, bad


def test_workspace_size_is_its_formula():
    lib = L.load()
    slot, cls = lib.ktf_head_slot_rows(), 256
    al = lambda b: (b + 255) & ~255  # noqa: E731
    for B, N, K in [(0, 1, 1), (0, 7323, 2), (1, 1, 8), (slot, 23, 3), (slot + 1, 23, 3), (5, cls, 2), (5, cls + 1, 2), (64, 7323, 2),
                    (512, 7324, 1), (3 * slot - 2, 8192, 8)]:
        want = al(max(-(-B // slot), 1) * N * K * 8) + al(-(-N // cls) * max(B, 1) * 8)
        assert lib.ktf_head_workspace_bytes(B, N, K) == want > 0, (B, N, K)
        if K == 1:
            assert want == lib.ktf_loss_workspace_bytes(B, N)


# ----------------------------------------------------------------------------- ktf.autograd
def test_value_errors_name_the_argument():
    z, labels, ix, iw = torch.zeros((3, 6)), torch.tensor([0, 1, 2]), torch.ones(3), torch.ones(6)
    cos = dict(kind="aam", margin=0.2, scale=30.0, inv_norm_x=ix, inv_norm_w=iw)
    bad = [("sub_centers", dict(cos, sub_centers=0)), ("sub_centers", dict(cos, sub_centers=9)), ("sub_centers", dict(cos, sub_centers=2.0)),
           ("sub_centers", dict(sub_centers=2)), ("sub_centers", dict(cos, sub_centers=4)), ("top_k", dict(cos, top_k=-1)),
           ("top_k", dict(cos, top_k=65)), ("top_k", dict(cos, top_k=True)), ("top_k", dict(top_k=1)), ("penalty", dict(cos, top_k=2, penalty=-0.1)),
           ("penalty", dict(cos, penalty=0.1)), ("penalty", dict(cos, top_k=2, penalty=float("nan"))), ("label_smoothing", dict(label_smoothing=1.0)),
           ("label_smoothing", dict(cos, label_smoothing=-0.1)), ("label_smoothing", dict(label_smoothing=float("nan"))),
           ("inv_norm_w", dict(cos, sub_centers=2, inv_norm_w=torch.ones(3)))]
    for name, kw in bad:
        with pytest.raises(ValueError, match=name):
            A.margin_softmax_loss(z, labels, **kw)
    with pytest.raises(ktf.KtfBackendError):                       # good arguments get as far as the device check
        A.margin_softmax_loss(z, labels, **dict(cos, sub_centers=2, top_k=2, penalty=0.1, label_smoothing=0.1))
    cpu = torch.device("cpu")
    for name, kw in [("sub_centers", dict(sub_centers=0)), ("sub_centers", dict(sub_centers=9)), ("top_k", dict(top_k=65)),
                     ("sub_centers", dict(kind="softmax", sub_centers=2)), ("top_k", dict(kind="softmax", top_k=2, penalty=0.1)),
                     ("penalty", dict(penalty=0.1)), ("penalty", dict(top_k=2, penalty=-1.0)), ("label_smoothing", dict(label_smoothing=1.0))]:
        with pytest.raises(ValueError, match=name):
            A.ClassifierHead(**dict(dict(dim=6, num_classes=9, device=cpu), **kw))
    h = A.ClassifierHead(6, 9, sub_centers=3, top_k=5, penalty=0.06, label_smoothing=0.1, device=cpu)
    assert tuple(h.weight.shape) == (27, 6) and (h.sub_centers, h.top_k, h.penalty, h.label_smoothing) == (3, 5, 0.06, 0.1)
    assert tuple(h.center_counts.shape) == (9, 3) and h.center_counts.dtype == torch.int64 and not h.center_counts.any()
    assert set(h.state_dict()) == {"weight", "center_counts"}
    p = A.ClassifierHead(6, 9, kind="softmax", label_smoothing=0.1, device=cpu)     # smoothing alone goes with a plain head
    assert p.center_counts is None and set(p.state_dict()) == {"weight"}
    # the three are plain attributes read at every call: a bad assignment is refused then, by name
    for name, val in (("top_k", 65), ("penalty", -0.5), ("label_smoothing", 1.0)):
        old = getattr(h, name)
        setattr(h, name, val)
        with pytest.raises(ValueError, match=name):
            h(torch.ones((2, 6)), torch.tensor([0, 1]))
        setattr(h, name, old)
    with pytest.raises(ktf.KtfBackendError):
        h(torch.ones((2, 6)), torch.tensor([0, 1]))


def test_dominant_keeps_the_most_selected_centre_and_the_lowest_on_ties():
    cpu = torch.device("cpu")
    torch.manual_seed(1)
    h = A.ClassifierHead(4, 5, kind="am", margin=0.1, scale=20.0, sub_centers=3, top_k=2, penalty=0.05, label_smoothing=0.1, gemm="bf16x3",
                         device=cpu).eval()
    counts = torch.tensor([[0, 0, 0], [1, 5, 5], [7, 2, 7], [0, 0, 1], [2, 3, 1]])
    h.center_counts.copy_(counts)
    assert list(A.dominant_centers(counts)) == [0, 1, 0, 2, 1]
    want = [int(np.flatnonzero(r == r.max())[0]) for r in counts.numpy()]          # the host rule
    assert want == [0, 1, 0, 2, 1]
    d = h.dominant()
    assert isinstance(d, A.ClassifierHead) and d.sub_centers == 1 and d.center_counts is None and not d.training
    assert (d.kind, d.margin, d.scale, d.gemm, d.top_k, d.penalty, d.label_smoothing) == ("am", 0.1, 20.0, "bf16x3", 2, 0.05, 0.1)
    assert tuple(d.weight.shape) == (5, 4) and d.weight.data_ptr() != h.weight.data_ptr()
    assert torch.equal(d.weight, h.weight.view(5, 3, 4)[torch.arange(5), torch.tensor(want)])
    restored = A.ClassifierHead(4, 5, kind="am", sub_centers=3, device=cpu)
    restored.load_state_dict(h.state_dict())
    assert torch.equal(restored.center_counts, counts)
    one = A.ClassifierHead(4, 5, device=cpu)
    assert torch.equal(one.dominant().weight, one.weight)
