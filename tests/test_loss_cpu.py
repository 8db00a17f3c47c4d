"""The classification head's loss without a GPU: the fp64 oracle (tests/_loss_ref.py) against fp64 torch.autograd of a torch
restatement, hand-computed values on every branch of psi, the C-ABI of include/ktf_loss.h (symbols, argument refusals before any
launch, the workspace size) and the argument checks of ktf.autograd.row_inv_norm / margin_softmax_loss / ClassifierHead."""

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
import _loss_ref as R  # noqa: E402

F64 = torch.float64
FLOOR = 2.0 ** -20


def _close(got, want, what):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    scale = max(float(np.abs(np.asarray(want)).max()), 1.0)
    assert err <= 1e-12 * scale, (what, err, scale)


# ----------------------------------------------------------------------------- the oracle
def torch_loss(z, labels, ix, iw, kind, margin, scale):
    """The rules of ktf_loss.h in torch ops, for autograd: per-row losses (B,)."""
    N = z.shape[1]
    c = z if ix is None else z * ix[:, None] * iw[None, :]
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
    logits = (scale * c).scatter(1, y, ly[:, None])
    return torch.where(valid, torch.logsumexp(logits, dim=1) - ly, torch.zeros((), dtype=z.dtype))


def torch_inv_norm(x, eps):
    return 1.0 / torch.clamp(torch.sqrt((x * x).sum(1)), min=eps)


CASES = [("softmax", 0.0, 1.0, False), ("softmax", 0.0, 12.0, True), ("am", 0.25, 16.0, True), ("aam", 0.3, 16.0, True)]


def _head_inputs(kind, margin, rng, B=7, N=11, D=5):
    x, w = rng.standard_normal((B, D)), rng.standard_normal((N, D))
    x[2] = -3.0 * w[4]                                            # a target cosine of -1: the fallback branch of aam
    x[3] = 2.0 * w[5] + 0.5 * rng.standard_normal(D)              # ... and one near +1
    labels = np.array([0, N - 1, 4, 5, -1, N, 3])
    gloss = rng.standard_normal(B)
    gloss[1] = 0.0
    return x, w, labels, gloss


@pytest.mark.parametrize("kind,margin,scale,cosine", CASES)
def test_oracle_equals_autograd_of_the_torch_restatement(kind, margin, scale, cosine):
    rng = np.random.default_rng(11)
    x, w, labels, gloss = _head_inputs(kind, margin, rng)
    B, N, eps = x.shape[0], w.shape[0], 1e-12
    z = x @ w.T + (0.0 if cosine else rng.standard_normal(N)[None, :])         # a plain head: bias-like offsets
    ix = R.inv_norm(x, eps)["inv"] if cosine else None
    iw = R.inv_norm(w, eps)["inv"] if cosine else None
    f = R.forward(z, labels, ix, iw, kind, margin, scale)
    g = R.backward(z, labels, ix, iw, kind, margin, scale, f["lse"], gloss)

    # no target cosine within 1e-3 of a kink of psi (-cos m, and sqrt(1 - floor) where the sine floor sets in)
    for b in np.flatnonzero(f["valid"]):
        cy = f["c"][b, labels[b]]
        if kind == "aam":
            assert abs(cy + math.cos(margin)) > 1e-3 and abs(cy - math.sqrt(1.0 - FLOOR)) > 1e-3, (b, cy)
    assert list(f["valid"]) == [True, True, True, True, False, False, True]
    if kind == "aam":
        assert f["c"][2, 4] < -math.cos(margin) < f["c"][3, 5]    # both branches are taken

    tz = torch.tensor(z, dtype=F64, requires_grad=True)
    tix = torch.tensor(ix, dtype=F64, requires_grad=True) if cosine else None
    tiw = torch.tensor(iw, dtype=F64, requires_grad=True) if cosine else None
    tl = torch.tensor(labels)
    loss = torch_loss(tz, tl, tix, tiw, kind, margin, scale)
    (loss * torch.tensor(gloss)).sum().backward()
    _close(f["loss"], loss.detach().numpy(), "loss")
    _close(f["lse"][f["valid"]] - f["ly"][f["valid"]], f["loss"][f["valid"]], "lse - ly")
    _close(g["dz"], tz.grad.numpy(), "dz")
    assert not f["loss"][4] and not f["loss"][5] and not g["dz"][4].any() and not g["dz"][5].any() and not g["dz"][1].any()
    assert (g["dz_mag"] >= np.abs(g["dz"]) * (1 - 1e-12)).all()
    if cosine:
        _close(g["dinv_x"], tix.grad.numpy(), "dinv_x")
        _close(g["dinv_w"], tiw.grad.numpy(), "dinv_w")
        assert (g["dinv_x_abs"] >= np.abs(g["dinv_x"]) - 1e-12).all() and (g["dinv_w_abs"] >= np.abs(g["dinv_w"]) - 1e-12).all()
        assert not g["dinv_x"][4] and not g["dinv_x"][5]
    else:
        assert not g["dinv_x"].any() and not g["dinv_w"].any()
    assert np.array_equal(f["pred"], np.argmax(f["c"], axis=1))


@pytest.mark.parametrize("kind,margin,scale,cosine", [c for c in CASES if c[3]])
def test_oracle_through_the_inverse_norms_equals_autograd_in_x_and_w(kind, margin, scale, cosine):
    rng = np.random.default_rng(12)
    x, w, labels, gloss = _head_inputs(kind, margin, rng)
    eps = 1e-12
    nx, nw = R.inv_norm(x, eps), R.inv_norm(w, eps)
    z = x @ w.T
    f = R.forward(z, labels, nx["inv"], nw["inv"], kind, margin, scale)
    g = R.backward(z, labels, nx["inv"], nw["inv"], kind, margin, scale, f["lse"], gloss)
    dx = g["dz"] @ w + R.inv_norm_backward(x, eps, nx["inv"], g["dinv_x"])
    dw = g["dz"].T @ x + R.inv_norm_backward(w, eps, nw["inv"], g["dinv_w"])

    tx, tw = torch.tensor(x, dtype=F64, requires_grad=True), torch.tensor(w, dtype=F64, requires_grad=True)
    loss = torch_loss(tx @ tw.T, torch.tensor(labels), torch_inv_norm(tx, eps), torch_inv_norm(tw, eps), kind, margin, scale)
    (loss * torch.tensor(gloss)).sum().backward()
    _close(f["loss"], loss.detach().numpy(), "loss")
    _close(dx, tx.grad.numpy(), "dx")
    _close(dw, tw.grad.numpy(), "dw")


def test_inverse_norm_oracle_and_its_clamp():
    x = np.array([[3.0, 4.0], [0.0, 0.0], [1e-3, 0.0], [1e-5, 0.0]])
    n = R.inv_norm(x, 1e-4)
    assert np.array_equal(n["inv"], [0.2, 1e4, 1.0 / 1e-3, 1e4]) and list(n["clamped"]) == [False, True, False, True]
    ginv = np.array([2.0, np.nan, -1.0, np.nan])
    dx = R.inv_norm_backward(x, 1e-4, n["inv"], ginv)
    _close(dx[0], -2.0 * 0.2 ** 3 * x[0], "dx")
    assert not dx[1].any() and not dx[3].any() and np.isfinite(dx).all()
    tx = torch.tensor(x, dtype=F64, requires_grad=True)
    (torch_inv_norm(tx, 1e-4) * torch.tensor(np.nan_to_num(ginv))).sum().backward()
    _close(dx[[0, 2, 3]], tx.grad.numpy()[[0, 2, 3]], "dx against autograd")        # (torch's sqrt has no gradient at the zero row)


def test_psi_on_every_branch_by_hand():
    m = 0.2
    cm, sm = math.cos(m), math.sin(m)
    root = 2.0 ** -10                                             # sqrt of the floor
    assert R.psi(0.3, "softmax", 0.0) == (0.3, 1.0)
    assert R.psi(0.3, "am", 0.25) == (0.3 - 0.25, 1.0)

    def angle(c):                                                 # cos(theta + m) and its derivative in c, away from the floor
        th = math.acos(c)
        return math.cos(th + m), math.sin(th + m) / math.sin(th)
    for c in (0.9, 0.0, -0.5, -cm + 1e-9):                        # the main branch, up to just above -cos m
        p, d = R.psi(c, "aam", m)
        assert abs(p - angle(c)[0]) <= 1e-12 and abs(d - angle(c)[1]) <= 1e-9 * max(1.0, abs(d)), c
    for c in (-cm - 1e-9, -cm, -0.999, -1.0):                     # the fallback from -cos m down (the comparison is strict)
        assert R.psi(c, "aam", m) == (c - m * sm, 1.0), c
    # its two values at -cos m: cos(pi) = -1 from above, -cos m - m sin m at and below (the usual fallback is not continuous)
    assert abs(R.psi(-cm + 1e-12, "aam", m)[0] - (-1.0)) <= 1e-9 and abs(R.psi(-cm, "aam", m)[0] - (-cm - m * sm)) <= 1e-15

    above, below = math.sqrt(1.0 - FLOOR * (1 + 1e-6)), math.sqrt(1.0 - FLOOR * (1 - 1e-6))
    assert 1.0 - above * above > FLOOR > 1.0 - below * below
    p, d = R.psi(above, "aam", m)
    S = math.sqrt(1.0 - above * above)
    assert p == above * cm - S * sm and d == cm + (sm * above) / S and d > 200.0
    for c in (below, 1.0, 1.0 + 2.0 ** -23):                      # the floor holds, |c| marginally above 1 included
        assert R.psi(c, "aam", m) == (c * cm - root * sm, cm), c
    assert R.psi(1.0, "aam", m) == (cm - root * sm, cm)
    assert R.psi(-1.0, "aam", m) == (-1.0 - m * sm, 1.0)


def test_degenerate_rows_of_the_oracle():
    for kind, margin, cos in (("softmax", 0.0, False), ("am", 0.3, True), ("aam", 0.3, True)):
        one = np.ones(1) if cos else None
        f = R.forward([[0.7]], [0], one, one, kind, margin, 8.0)  # N = 1
        g = R.backward([[0.7]], [0], one, one, kind, margin, 8.0, f["lse"])
        assert f["loss"][0] == 0.0 and g["dz"][0, 0] == 0.0 and f["pred"][0] == 0
    z = np.array([[2.0, 5.0, 5.0, -1.0]])
    f = R.forward(z, [7], None, None, "softmax", 0.0, 1.0)        # ignored: lse and pred all the same
    assert f["pred"][0] == 1 and f["loss"][0] == 0.0 and abs(f["lse"][0] - math.log(np.exp(z).sum())) < 1e-12
    z = np.array([[64.0, -64.0, 0.0]])                            # the others underflow to p = 0
    f = R.forward(z, [0], None, None, "softmax", 0.0, 1.0)
    g = R.backward(z, [0], None, None, "softmax", 0.0, 1.0, f["lse"])
    assert f["loss"][0] < 1e-27 and np.isfinite(g["dz"]).all() and 0.0 < g["dz"][0, 1] < 1e-50


# ----------------------------------------------------------------------------- the C-ABI
def test_header_symbols_are_the_loss_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_loss.h")).read()
    code = hdr[hdr.index("#ifndef KTF_LOSS_H_"):]
    protos = re.findall(r"^(?:int|int32_t|int64_t) (ktf_[a-z0-9_]+)\(([^;]*)\);", code, flags=re.M)
    assert {n for n, _ in protos} == set(L.LOSS_PROTOTYPES) == set(re.findall(r"\b(ktf_[a-z0-9_]+)\s*\(", code))
    ctype = {"const float*": L._P, "float*": L._P, "const double*": L._P, "double*": L._P, "const int32_t*": L._P, "int32_t*": L._P,
             "void*": L._P, "int64_t": L._i64, "int32_t": L._i32, "double": C.c_double, "size_t": C.c_size_t}
    for name, args in protos:
        args = [a.strip() for a in args.replace("\n", " ").split(",")]
        want = [] if args == ["void"] else [ctype[a.rsplit(" ", 1)[0]] for a in args]
        assert L.LOSS_PROTOTYPES[name][1] == want, name
    assert all(n.startswith("ktf_loss_") for n in L.LOSS_PROTOTYPES)
    lib = L.load()
    for name in L.LOSS_PROTOTYPES:
        assert hasattr(lib, name), name
    others = set(L.PROTOTYPES) | set(L.AUGMENT_PROTOTYPES) | set(L.RESAMPLE_PROTOTYPES) | set(L.GRAD_PROTOTYPES) | set(L.NORM_PROTOTYPES)
    assert not set(L.LOSS_PROTOTYPES) & others
    for other in ("ktf_hip.h", "ktf_augment.h", "ktf_resample.h", "ktf_grad.h", "ktf_norm.h"):
        assert "ktf_loss_" not in open(os.path.join(ROOT, "include", other)).read()
    assert len(L.PROTOTYPES) == 120 and lib.ktf_version() == 117
    assert lib.ktf_loss_slot_rows() == int(re.search(r"#define KTF_LOSS_SLOT_ROWS (\d+)", hdr).group(1)) >= 1
    assert float(re.search(r"#define KTF_LOSS_SIN2_FLOOR (\S+)", hdr).group(1)) == FLOOR == L.LOSS_SIN2_FLOOR == R.SIN2_FLOOR
    for name, val in (("SOFTMAX", L.LOSS_SOFTMAX), ("AM", L.LOSS_AM), ("AAM", L.LOSS_AAM)):
        assert int(re.search(rf"#define KTF_LOSS_{name} (\d+)", hdr).group(1)) == val == ktf.ops.LOSS_KINDS[name.lower()]


def _refused(rc, text):
    assert rc == -1, rc
    assert text in L.last_error(), L.last_error()
    with pytest.raises(ValueError):
        L.check(rc, "x")


def test_argument_checks_without_gpu():
    lib = L.load()
    raw = (C.c_float * 16384)()
    buf = C.c_void_p((C.addressof(raw) + 255) & ~255)      # stands for any aligned non-null device pointer: every refusal comes before a launch
    far = C.c_void_p(buf.value + 32768)                    # a second one that does not overlap B * ld floats at buf
    odd = C.c_void_p(buf.value + 4)
    B, N, D = 5, 12, 8
    need = lib.ktf_loss_workspace_bytes(B, N)
    assert need > 0
    inf, nan = float("inf"), float("nan")

    def fwd(z=buf, ldz=12, B=B, N=N, labels=buf, inv_x=buf, inv_w=buf, kind=2, margin=0.2, scale=30.0, loss=buf, pred=buf, lse=buf, ws=buf,
            ws_bytes=None):
        return lib.ktf_loss_margin_softmax_forward(z, ldz, B, N, labels, inv_x, inv_w, kind, margin, scale, loss, pred, lse, ws,
                                                   need if ws_bytes is None else ws_bytes, None)

    def bwd(z=buf, ldz=12, B=B, N=N, labels=buf, inv_x=buf, inv_w=buf, kind=2, margin=0.2, scale=30.0, lse=buf, gloss=None, dz=far, lddz=12,
            dinv_x=buf, dinv_w=buf, ws=buf, ws_bytes=None):
        return lib.ktf_loss_margin_softmax_backward(z, ldz, B, N, labels, inv_x, inv_w, kind, margin, scale, lse, gloss, dz, lddz, dinv_x,
                                                    dinv_w, ws, need if ws_bytes is None else ws_bytes, None)

    for name in ("z", "labels", "loss", "lse", "ws"):
        _refused(fwd(**{name: None}), "null")
    for name in ("z", "labels", "lse", "dz", "ws"):
        _refused(bwd(**{name: None}), "null")
    for fn, lds in ((fwd, ("ldz",)), (bwd, ("ldz", "lddz"))):
        plain = dict(inv_x=None, inv_w=None, **({"dinv_x": None, "dinv_w": None} if fn is bwd else {}))
        _refused(fn(inv_x=None), "go together")
        _refused(fn(inv_w=None), "go together")
        _refused(fn(kind=1, **plain), "cosine head")
        _refused(fn(kind=2, **plain), "cosine head")
        _refused(fn(kind=0, margin=0.1), "margin must be 0")
        _refused(fn(kind=0, margin=0.1, **plain), "margin must be 0")
        for bad in (0.0, -1.0, inf, nan):
            _refused(fn(scale=bad), "scale")
        for bad in (-0.1, inf, nan):
            _refused(fn(margin=bad), "margin")
            _refused(fn(kind=1, margin=bad), "margin")
        _refused(fn(margin=math.pi / 2), "pi / 2")
        _refused(fn(margin=2.0), "pi / 2")
        for bad in (-1, 3, 7):
            _refused(fn(kind=bad), "unknown kind")
        _refused(fn(B=-1), "negative size")
        _refused(fn(N=0), "below 1")
        _refused(fn(N=-4), "below 1")
        _refused(fn(B=1 << 31), "2^31")
        _refused(fn(N=1 << 31, **{ld: 1 << 31 for ld in lds}), "2^31")
        _refused(fn(B=1 << 30, N=1 << 30, **{ld: 1 << 30 for ld in lds}), "too large")
        for ld in lds:
            _refused(fn(**{ld: 11}), "leading dimension")
            _refused(fn(**{ld: 1 << 31}), "2^31")
        _refused(fn(ws_bytes=need - 1), "workspace")
        _refused(fn(ws=odd), "256-byte")
    _refused(bwd(dinv_x=None), "dinv_x")
    _refused(bwd(dinv_w=None), "dinv_x")
    _refused(bwd(kind=0, margin=0.0, inv_x=None, inv_w=None), "dinv_x")             # a plain head takes neither
    _refused(bwd(dz=buf, lddz=16), "overlaps z")                                     # in place only with the same leading dimension
    _refused(bwd(dz=odd), "overlaps z")
    _refused(bwd(dz=C.c_void_p(buf.value + 4 * ((B - 1) * 12 + N - 1))), "overlaps z")   # the last float of z
    _refused(bwd(z=C.c_void_p(far.value + 4 * (B * 12 - 1))), "overlaps z")          # the last float of dz
    for bad in ((-1, 4), (4, 0), (1 << 31, 4), (4, 1 << 31), (1 << 30, 1 << 30)):
        assert lib.ktf_loss_workspace_bytes(*bad) == -1

    def nrm(x=buf, ldx=8, rows=B, D=D, eps=1e-12, inv=buf):
        return lib.ktf_loss_row_inv_norm(x, ldx, rows, D, eps, inv, None)

    def nrb(x=buf, ldx=8, rows=B, D=D, eps=1e-12, inv=buf, ginv=buf, dx=far, lddx=8):
        return lib.ktf_loss_row_inv_norm_backward(x, ldx, rows, D, eps, inv, ginv, dx, lddx, None)

    for name in ("x", "inv"):
        _refused(nrm(**{name: None}), "null")
    for name in ("x", "inv", "ginv", "dx"):
        _refused(nrb(**{name: None}), "null")
    for fn, lds in ((nrm, ("ldx",)), (nrb, ("ldx", "lddx"))):
        _refused(fn(rows=-1), "negative size")
        _refused(fn(D=0), "below 1")
        _refused(fn(rows=1 << 31), "2^31")
        _refused(fn(D=1 << 31, **{ld: 1 << 31 for ld in lds}), "2^31")
        for ld in lds:
            _refused(fn(**{ld: 7}), "leading dimension")
        for bad in (0.0, -1e-12, inf, nan):
            _refused(fn(eps=bad), "eps")
    _refused(nrb(dx=buf), "overlaps x")
    _refused(nrb(dx=C.c_void_p(buf.value + 4 * ((B - 1) * 8 + D - 1))), "overlaps x")


def test_workspace_size_is_its_formula():
    lib = L.load()
    slot = lib.ktf_loss_slot_rows()
    hdr = open(os.path.join(ROOT, "include", "ktf_loss.h")).read()
    cols = int(re.search(r"#define KTF_LOSS_CHUNK_COLS (\d+)", hdr).group(1))
    al = lambda b: (b + 255) & ~255  # noqa: E731
    for B, N in [(0, 1), (0, 7323), (1, 1), (slot, 23), (slot + 1, 23), (5, cols), (5, cols + 1), (64, 7323), (512, 7324), (3 * slot - 2, 8192)]:
        want = al(max(-(-B // slot), 1) * N * 8) + al(-(-N // cols) * max(B, 1) * 8)
        assert lib.ktf_loss_workspace_bytes(B, N) == want > 0, (B, N)


# ----------------------------------------------------------------------------- ktf.autograd
def test_loss_functions_refuse_cpu_tensors():
    z, labels = torch.zeros((3, 5)), torch.tensor([0, 1, 2])
    with pytest.raises(ktf.KtfBackendError):
        A.row_inv_norm(torch.ones((3, 4)))
    with pytest.raises(ktf.KtfBackendError):
        A.margin_softmax_loss(z, labels)
    with pytest.raises(ktf.KtfBackendError):
        A.margin_softmax_loss(z, labels, "aam", 0.2, 30.0, torch.ones(3), torch.ones(5))
    head = A.ClassifierHead(4, 5, device="cpu")
    with pytest.raises(ktf.KtfBackendError):
        head(torch.ones((3, 4)), labels)
    with pytest.raises(ktf.KtfBackendError):
        head.cosines(torch.ones((3, 4)))


def test_margin_softmax_loss_value_errors_name_the_argument():
    z, labels, ix, iw = torch.zeros((3, 5)), torch.tensor([0, 1, 2]), torch.ones(3), torch.ones(5)
    bad = [("kind", dict(kind="arc")), ("margin", dict(kind="am", margin=-0.1, inv_norm_x=ix, inv_norm_w=iw)),
           ("margin", dict(kind="softmax", margin=0.1)), ("margin", dict(kind="aam", margin=1.6, inv_norm_x=ix, inv_norm_w=iw)),
           ("margin", dict(kind="am", margin=float("nan"), inv_norm_x=ix, inv_norm_w=iw)), ("scale", dict(scale=0.0)),
           ("scale", dict(scale=float("inf"))), ("inv_norm_x", dict(inv_norm_x=ix)), ("inv_norm_w", dict(inv_norm_w=iw)),
           ("inv_norm_x", dict(kind="aam", margin=0.2)), ("inv_norm_x", dict(inv_norm_x=torch.ones(4), inv_norm_w=iw)),
           ("inv_norm_w", dict(inv_norm_x=ix, inv_norm_w=torch.ones(3)))]
    for name, kw in bad:
        with pytest.raises(ValueError, match=name):
            A.margin_softmax_loss(z, labels, **kw)
    with pytest.raises(ValueError, match="labels"):
        A.margin_softmax_loss(z, torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="labels"):
        A.margin_softmax_loss(z, torch.tensor([0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="z"):
        A.margin_softmax_loss(torch.zeros(5), labels)
    with pytest.raises(ValueError, match="eps"):
        A.row_inv_norm(torch.ones((3, 4)), eps=0.0)
    with pytest.raises(ValueError, match="x"):
        A.row_inv_norm(torch.ones(4))


def test_classifier_head_arguments_and_parameters():
    cpu = torch.device("cpu")
    for name, kw in [("dim", dict(dim=0)), ("dim", dict(dim=2.5)), ("num_classes", dict(num_classes=0)), ("kind", dict(kind="arc")),
                     ("margin", dict(margin=-1.0)), ("margin", dict(kind="softmax", margin=0.2)), ("margin", dict(margin=1.6)),
                     ("scale", dict(scale=0.0)), ("bias", dict(bias=True)), ("bias", dict(kind="softmax", normalize=True, bias=True)),
                     ("normalize", dict(kind="am", normalize=False)), ("normalize", dict(normalize=1)), ("gemm", dict(gemm="fp8")),
                     ("eps", dict(eps=0.0))]:
        args = dict(dim=6, num_classes=9, device=cpu)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            A.ClassifierHead(**args)
    h = A.ClassifierHead(6, 9, device=cpu)
    assert (h.kind, h.margin, h.scale, h.normalize, h.gemm, h.bias) == ("aam", 0.2, 30.0, True, "f32", None)
    assert tuple(h.weight.shape) == (9, 6) and h.weight.dtype == torch.float32 and [n for n, _ in h.named_parameters()] == ["weight"]
    p = A.ClassifierHead(6, 9, kind="softmax", bias=True, gemm="bf16x3", device=cpu)
    assert (p.margin, p.scale, p.normalize) == (0.0, 1.0, False) and tuple(p.bias.shape) == (9,)
    assert [n for n, _ in p.named_parameters()] == ["weight", "bias"]
    c = A.ClassifierHead(6, 9, kind="softmax", normalize=True, device=cpu)
    assert (c.margin, c.scale, c.normalize) == (0.0, 30.0, True)
    # margin and scale are read at every call: a bad assignment is refused then, by name
    h.margin = 2.0
    with pytest.raises(ValueError, match="margin"):
        h(torch.ones((2, 6)), torch.tensor([0, 1]))
    h.margin, h.scale = 0.1, -1.0
    with pytest.raises(ValueError, match="scale"):
        h(torch.ones((2, 6)), torch.tensor([0, 1]))
    h.scale = 30.0
    with pytest.raises(ValueError, match="emb"):
        h(torch.ones((2, 5)), torch.tensor([0, 1]))
