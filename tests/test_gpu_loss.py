"""The classification head's loss kernels (include/ktf_loss.h) on the GPU against the fp64 oracle of tests/_loss_ref.py, and
ktf.autograd.row_inv_norm / margin_softmax_loss / ClassifierHead over them.

Bounds (u = 2^-24, the unit roundoff of fp32; every output is fp64 arithmetic rounded once, so u times the value is what the
rounding alone may cost and the bounds below leave a factor 2). The fp64 part, for inputs with |l| <= 64 and N <= 8192 (asserted):
the argument of an exponential is off by at most 4 * 2^-53 * 64, a sum of N terms by N 2^-53 relative, exp and log add an ulp each;
hence |lse - ref| <= 2^-38 (1 + |ref|) and p_j is relative-accurate to 2^-36, far below u.
    lse      |got - ref| <= 2^-38 (1 + |ref|)                                  (fp64)
    loss     |got - ref| <= 2 u (|lse| + |l_y|)
    dz       |got - ref| <= 2 u |gloss scale psi' inv_x inv_w| (p_j + [j = y])
    dinv_*   |got - ref| <= u |S| + 2^-36 sum |terms|                          (one rounding of the sum S, plus the fp64 part)
    inv      |got - ref| <= 2 u inv;        dx of the norm   |got - ref| <= 2 u |value|
    pred     equal to the oracle's where its two largest cosines differ by more than 2^-40 relative (always, on exact inputs)
A value below the normal range of fp32 is rounded to a multiple of 2^-149: every fp32 bound has that much added. The bounds of the
whole head (`head_reference`) are derived there. The worst ratios measured are in DESIGN.md section 7."""

import functools
import math
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
import _loss_ref as R  # noqa: E402
from _tdnn16_ref import X3_OPERANDS, bf16_rne  # noqa: E402
from test_loss_cpu import torch_inv_norm, torch_loss  # noqa: E402
from test_tdnn_grad_cpu import restated_pool, restated_tdnn  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TINY = 2.0 ** -149
DEV = "cuda:0"
NAN = float("nan")
EPS = 1e-12
# name -> (kind, margin, scale, cosine head)
HEADS = {"plain": ("softmax", 0.0, 1.0, False), "softmax": ("softmax", 0.0, 30.0, True), "am": ("am", 0.25, 30.0, True),
         "aam": ("aam", 0.3, 30.0, True)}
SIZES = [1, 2, 63, 64, 65, 257, 1000, 7323, 8192]


def _dev(a):
    return None if a is None else torch.as_tensor(np.array(a), device=DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _strided(values, extra, offset, fill=NAN):
    """A (B, N + extra) device view holding `values` in its first N columns and `fill` in the rest, starting `offset` floats into
    its allocation."""
    B, N = values.shape
    ld = N + extra
    flat = torch.full((B * ld + offset + 1,), fill, dtype=torch.float32, device=DEV)
    full = flat[offset:offset + B * ld].view(B, ld)
    full[:, :N] = torch.as_tensor(np.array(values, dtype=np.float32))
    return full


def run_loss(c, extra=0, offset=0, inplace=False, gloss="case", want_pred=True):
    """Both calls on fresh buffers whose outputs start as NaN, the workspace as NaN too. Returns numpy: loss, pred, lse, dz with
    its pad columns, dinv_x, dinv_w (None for a plain head)."""
    z = c["z"]
    B, N = z.shape
    kind, margin, scale, cosine = c["head"]
    zf = _strided(z, extra, offset)
    tl, ix, iw = _dev(c["labels"].astype(np.int32)), _dev(c["ix"]), _dev(c["iw"])
    gl = _dev(c["gloss"] if isinstance(gloss, str) else gloss)
    loss = torch.full((B,), NAN, dtype=torch.float32, device=DEV)
    pred = torch.full((B,), -7, dtype=torch.int32, device=DEV) if want_pred else None
    lse = torch.full((B,), NAN, dtype=torch.float64, device=DEV)
    ws = ops.loss_workspace(B, N, DEV)
    ws.fill_(0xFF)
    ops.loss_margin_softmax_forward(zf[:, :N], tl, ix, iw, kind, margin, scale, loss, pred, lse, ws)
    dzf = zf if inplace else _strided(np.full((B, N), NAN, np.float32), extra, offset)
    dix = torch.full((B,), NAN, dtype=torch.float32, device=DEV) if cosine else None
    diw = torch.full((N,), NAN, dtype=torch.float32, device=DEV) if cosine else None
    ops.loss_margin_softmax_backward(zf[:, :N], tl, ix, iw, kind, margin, scale, lse, gl, dzf, dix, diw, ws)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return dict(loss=host(loss), pred=host(pred), lse=host(lse), dz=host(dzf), dinv_x=host(dix), dinv_w=host(diw))


def make_case(head, z, labels, ix, iw, gloss):
    """The inputs (read-only from here on) and their oracle. head: a name of HEADS or such a tuple."""
    head = HEADS.get(head, head) if isinstance(head, str) else head
    kind, margin, scale, cosine = head
    z, labels = np.asarray(z, np.float32), np.asarray(labels)
    ix = np.asarray(ix, np.float32) if cosine else None
    iw = np.asarray(iw, np.float32) if cosine else None
    gloss = None if gloss is None else np.asarray(gloss, np.float32)
    f = R.forward(z, labels, ix, iw, kind, margin, scale)
    g = R.backward(z, labels, ix, iw, kind, margin, scale, f["lse"], gloss)
    assert np.abs(scale * f["c"]).max(initial=0.0) <= 64.0 and np.abs(f["ly"]).max(initial=0.0) <= 64.0 and z.shape[1] <= 8192
    for a in (z, labels, ix, iw, gloss):
        if a is not None:
            a.setflags(write=False)
    return dict(head=head, z=z, labels=labels, ix=ix, iw=iw, gloss=gloss, f=f, g=g)


def _labels(B, N, rng):
    """The corner labels first (0, N - 1, and the ignored -1 and N), random valid ones behind them."""
    return np.concatenate([[0, N - 1, -1, N], rng.integers(0, N, max(B - 4, 0))])[:B]


@functools.lru_cache(maxsize=None)
def gaussian(head, B, N):
    """A Gaussian batch of one head and shape and its oracle, computed once and shared by the tests that use it (read-only).
    Cosine heads: |c| <= 2.4 * 0.4 < 1; the plain one: logits with bias-like offsets per column, |l| <= 48."""
    rng = np.random.default_rng(1000 * B + N)
    if HEADS[head][3]:
        z = np.clip(rng.standard_normal((B, N)), -2.4, 2.4)
    else:
        z = np.clip(4.0 * rng.standard_normal((B, N)), -40.0, 40.0) + rng.uniform(-8.0, 8.0, N)[None, :]
    gloss = rng.standard_normal(B)
    if B > 4:
        gloss[4] = 0.0
    return make_case(head, z, _labels(B, N, rng), rng.uniform(0.2, 0.4, B), rng.uniform(0.5, 1.0, N), gloss)


def _ratio(err, bound, name):
    """Worst |err| / bound; where the bound is zero an exact zero is expected. fp32 outputs: 2^-149 on top (the module docstring)."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    live = bound > 0
    assert (err[~live] == 0).all(), name
    return float((err[live] / (bound[live] + TINY)).max()) if live.any() else 0.0


def check_against_oracle(got, c, tag):
    f, g = c["f"], c["g"]
    B, N = c["z"].shape
    assert not np.isnan(got["loss"]).any() and not np.isnan(got["lse"]).any() and not np.isnan(got["dz"]).any(), tag
    assert not got["dz"][:, N:].any(), tag                       # the pad columns are written as zero
    lse_err = np.abs(got["lse"] - f["lse"])
    assert (lse_err <= 2.0 ** -38 * (1 + np.abs(f["lse"]))).all(), (tag, lse_err.max(initial=0.0))
    ratios = {"lse": float((lse_err / (2.0 ** -38 * (1 + np.abs(f["lse"])))).max(initial=0.0))}
    ratios["loss"] = _ratio(np.abs(got["loss"] - f["loss"]), 2 * U * (np.abs(f["lse"]) + np.abs(f["ly"])) * f["valid"], "loss")
    ratios["dz"] = _ratio(np.abs(got["dz"][:, :N] - g["dz"]), 2 * U * g["dz_mag"], "dz")
    if c["ix"] is not None:
        for k in ("dinv_x", "dinv_w"):
            assert not np.isnan(got[k]).any(), (tag, k)
            ratios[k] = _ratio(np.abs(got[k] - g[k]), U * np.abs(g[k]) + 2.0 ** -36 * g[k + "_abs"], k)
    else:
        assert got["dinv_x"] is None and got["dinv_w"] is None
    print(f"{tag}: worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (tag, ratios)
    if got["pred"] is not None:
        sure = f["gap"] > 2.0 ** -40
        assert np.array_equal(got["pred"][sure], f["pred"][sure]), tag
        assert ((got["pred"] >= 0) & (got["pred"] < N)).all(), tag
    return ratios


def same_bits(a, b, tag):
    for k in a:
        assert (a[k] is None) == (b[k] is None), (tag, k)
        if a[k] is not None:
            assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), (tag, k)


def _cut(got, N):
    return dict(got, dz=got["dz"][:, :N])


# ----------------------------------------------------------------------------- rounding bounds: every width, stride and base
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("head", list(HEADS))
def test_gaussian_inputs_within_the_bounds_on_every_stride(head, N):
    """ld = N, N + 3, N + 4 with the base on and one float off a 16-byte boundary: rows start at every residue mod 4. One path
    (rule 8): the bits are the same."""
    B = ops.loss_slot_rows() + 1
    c = gaussian(head, B, N)
    base = run_loss(c)
    check_against_oracle(base, c, f"{head} B={B} N={N}")
    for extra, offset in ((0, 1), (3, 0), (3, 1), (4, 0), (4, 1)):
        other = run_loss(c, extra=extra, offset=offset)
        assert not other["dz"][:, N:].any()
        same_bits(_cut(base, N), _cut(other, N), f"{head} N={N} ld=N+{extra} offset={offset}")


def _batch_sizes():
    slot = 8                                                     # asserted against ktf_loss_slot_rows() in the test
    return [0, 1, 5, slot - 1, slot, slot + 1, 2 * slot + 3]


@pytest.mark.parametrize("B", _batch_sizes())
@pytest.mark.parametrize("head", ["plain", "aam"])
def test_batch_sizes_around_the_slots(head, B):
    """0, 1, 5, one less and one more than a slot, and three slots with a partial last one; two chunks of columns."""
    slot = ops.loss_slot_rows()
    assert _batch_sizes() == [0, 1, 5, slot - 1, slot, slot + 1, 2 * slot + 3]
    N = 257
    c = gaussian(head, B, N)
    got = run_loss(c, extra=3, offset=1)
    check_against_oracle(got, c, f"{head} B={B} N={N}")
    if B == 0:
        assert got["dz"].shape == (0, N + 3)
        if got["dinv_w"] is not None:
            assert got["dinv_w"].shape == (N,) and not got["dinv_w"].any()       # rule 9: the sum over no row


def test_ignored_rows_single_rows_and_gloss():
    slot = ops.loss_slot_rows()
    B, N = slot + 3, 65
    c = gaussian("aam", B, N)
    assert list(c["labels"][:4]) == [0, N - 1, -1, N] and c["gloss"][4] == 0.0
    got = run_loss(c)
    check_against_oracle(got, c, "labels 0, N - 1, -1, N")
    for b in (2, 3):
        assert got["loss"][b] == 0 and not got["dz"][b].any() and got["dinv_x"][b] == 0
    assert not got["dz"][4].any() and got["dinv_x"][4] == 0      # gloss = 0
    # NaN in the ignored rows' gloss, and no pred: the same bits
    poisoned = c["gloss"].copy()
    poisoned[[2, 3]] = NAN
    other = run_loss(c, gloss=poisoned, want_pred=False)
    assert other["pred"] is None
    same_bits(dict(got, pred=None), other, "NaN gloss of ignored rows")
    # gloss NULL = ones
    ones = make_case("aam", c["z"], c["labels"], c["ix"], c["iw"], np.ones(B))
    null = make_case("aam", c["z"], c["labels"], c["ix"], c["iw"], None)
    got_ones, got_null = run_loss(ones), run_loss(null)
    check_against_oracle(got_null, null, "gloss NULL")
    same_bits(got_ones, got_null, "gloss NULL against ones")
    # every row ignored
    none = make_case("aam", c["z"], np.where(np.arange(B) % 2, -1, N), c["ix"], c["iw"], c["gloss"])
    got_none = run_loss(none)
    check_against_oracle(got_none, none, "every row ignored")
    assert not got_none["loss"].any() and not got_none["dz"].any() and not got_none["dinv_x"].any() and not got_none["dinv_w"].any()
    assert np.array_equal(got_none["pred"], got["pred"])         # the prediction does not look at the label
    # one valid row, in the second slot
    labels = np.full(B, -1)
    labels[slot + 1] = 7
    one = make_case("aam", c["z"], labels, c["ix"], c["iw"], c["gloss"])
    got_one = run_loss(one)
    check_against_oracle(got_one, one, "one valid row")
    assert got_one["loss"][slot + 1] > 0 and np.count_nonzero(got_one["loss"]) == 1 and np.count_nonzero(got_one["dinv_x"]) == 1


def test_extreme_logits():
    """+64 and -64 in one row: every other probability underflows (exp(-128) is below the fp32 range: dz = 0 there), no NaN."""
    N = 70
    z = np.zeros((3, N), np.float32)
    z[0, 0], z[0, 1] = 64.0, -64.0
    z[1, 5], z[1, 6] = -64.0, 64.0
    z[2, :] = -64.0
    c = make_case("plain", z, [0, 5, 3], None, None, None)
    got = run_loss(c)
    check_against_oracle(got, c, "logits of +-64")
    assert np.isfinite(got["dz"]).all() and got["dz"][0, 1] == 0 and got["loss"][1] == 128.0 and got["pred"][1] == 6
    assert abs(got["loss"][2] - math.log(N)) <= 4 * U * 64 and got["pred"][2] == 0
    # a cosine head at scale 64: c = +-1
    zc = np.zeros((2, N), np.float32)
    zc[0, 0], zc[0, 1], zc[1, 2], zc[1, 3] = 1.0, -1.0, -1.0, 1.0
    cc = make_case(("am", 0.0, 64.0, True), zc, [0, 2], np.ones(2), np.ones(N), None)
    got = run_loss(cc)
    check_against_oracle(got, cc, "cosines of +-1 at scale 64")
    assert np.isfinite(got["dz"]).all() and np.isfinite(got["dinv_w"]).all()


def test_aam_targets_on_every_branch():
    """Target cosines on both sides of -cos m, on both sides of the sine floor, at +-1 and marginally above 1 (unit norms: c = z)."""
    kind, m, scale, _ = HEADS["aam"]
    cm = math.cos(m)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    up = f32(np.nextafter(np.float32(-cm), np.float32(1)))
    down = f32(np.nextafter(np.float32(-cm), np.float32(-1)))
    edge = math.sqrt(1.0 - R.SIN2_FLOOR)
    below_floor, above_floor = f32(np.nextafter(np.float32(edge), np.float32(2))), f32(np.nextafter(np.float32(edge), np.float32(0)))
    targets = [up, down, above_floor, below_floor, 1.0, -1.0, 1.0 + 2.0 ** -23, 0.3, -0.97]
    assert up > -cm > down and 1 - above_floor ** 2 > R.SIN2_FLOOR > 1 - below_floor ** 2
    B, N = len(targets), 130
    rng = np.random.default_rng(5)
    z = rng.uniform(-0.5, 0.5, (B, N)).astype(np.float32)
    labels = rng.integers(0, N, B)
    labels[0], labels[1] = 0, N - 1
    for b, t in enumerate(targets):
        z[b, labels[b]] = t
    c = make_case("aam", z, labels, np.ones(B), np.ones(N), rng.standard_normal(B))
    branch = [R.psi(z[b, labels[b]], kind, m)[1] for b in range(B)]
    assert branch[1] == 1.0 and branch[5] == 1.0 and branch[8] == 1.0 and branch[2] > 100 and branch[3] == branch[4] == branch[6] == cm
    got = run_loss(c)
    check_against_oracle(got, c, "aam branches")
    assert np.isfinite(got["dz"]).all() and np.isfinite(got["dinv_x"]).all() and np.isfinite(got["dinv_w"]).all()


@pytest.mark.parametrize("head", list(HEADS))
def test_a_single_class_gives_exact_zeros(head):
    B = 5
    rng = np.random.default_rng(9)
    c = make_case(head, rng.uniform(-0.9, 0.9, (B, 1)), [0, 0, -1, 1, 0], np.ones(B), np.ones(1), rng.standard_normal(B))
    for extra in (0, 3):
        got = run_loss(c, extra=extra)
        assert not got["loss"].any() and not got["dz"].any() and not got["pred"].any()
        check_against_oracle(got, c, f"{head} N=1")


def test_pred_on_exact_ties():
    """Integer logits and unit norms: the cosines are exact, equal maxima occur in every row, the lowest index wins; across threads,
    waves and chunks."""
    B, N = 6, 1000
    rng = np.random.default_rng(4)
    z = rng.integers(-3, 3, (B, N)).astype(np.float32)
    firsts = [0, 17, 255, 256, 511, 999]                          # thread 0, a lane, the last thread, the second round, the last column
    for b, j in enumerate(firsts):
        z[b, j:] = np.where(rng.random(N - j) < 0.3, 3.0, z[b, j:])
        z[b, j] = 3.0
        z[b, :j] = np.minimum(z[b, :j], 2.0)
    for head in ("plain", "softmax"):
        c = make_case(head, z / (1.0 if head == "plain" else 4.0), rng.integers(0, N, B), np.ones(B), np.ones(N), None)
        got = run_loss(c)
        assert list(got["pred"]) == firsts == list(c["f"]["pred"]), head
        check_against_oracle(got, c, f"ties {head}")


# ----------------------------------------------------------------------------- determinism, in place, columns that are not read
@pytest.mark.parametrize("head,N", [("aam", 7323), ("plain", 257), ("am", 64)])
def test_determinism_in_place_and_pad_columns(head, N):
    B = 2 * ops.loss_slot_rows() + 3
    c = gaussian(head, B, N)
    first, second = run_loss(c, extra=4), run_loss(c, extra=4)
    same_bits(first, second, "the same call twice")
    check_against_oracle(first, c, f"{head} B={B} N={N}")
    for extra, offset in ((0, 0), (3, 1), (4, 0)):                # _strided poisons z's pad columns with NaN: never read
        apart, inplace = run_loss(c, extra=extra, offset=offset), run_loss(c, extra=extra, offset=offset, inplace=True)
        assert not inplace["dz"][:, N:].any()                     # the NaN pad of z, now dz's, written as zero
        same_bits(apart, inplace, f"in place, ld=N+{extra}")
        same_bits(_cut(first, N), _cut(apart, N), f"ld=N+{extra} against ld=N+4")


# ----------------------------------------------------------------------------- the inverse norms
def run_norm(x, eps, ginv, extra=0, offset=0):
    rows, D = x.shape
    xf = _strided(x, extra, offset)
    inv = torch.full((rows,), NAN, dtype=torch.float32, device=DEV)
    dxf = _strided(np.full((rows, D), NAN, np.float32), extra, offset)
    ops.loss_row_inv_norm(xf[:, :D], eps, inv)
    ops.loss_row_inv_norm_backward(xf[:, :D], eps, inv, _dev(ginv), dxf)
    torch.cuda.synchronize()
    return dict(inv=inv.cpu().numpy(), dx=dxf.cpu().numpy())


@pytest.mark.parametrize("D", [1, 23, 512])
def test_inverse_norms(D):
    rows = 11                                                     # three workgroups of four rows, the last one partial
    rng = np.random.default_rng(D)
    x = rng.standard_normal((rows, D)).astype(np.float32)
    x[3] = 0.0                                                    # clamped by eps: inv = 1 / eps, dx = 0
    x[6] *= 1e-3
    x[7] = 1e-7 / math.sqrt(D)                                    # below eps = 1e-6: clamped too
    eps = 1e-6
    ginv = rng.standard_normal(rows).astype(np.float32)
    ginv[7] = NAN                                                 # a clamped row's ginv enters nothing
    n = R.inv_norm(x, eps)
    assert list(np.flatnonzero(n["clamped"])) == [3, 7]
    base = run_norm(x, eps, ginv)
    want_dx = R.inv_norm_backward(x, eps, base["inv"], np.nan_to_num(ginv))
    r_inv = _ratio(np.abs(base["inv"] - n["inv"]), 2 * U * n["inv"], "inv")
    r_dx = _ratio(np.abs(base["dx"] - want_dx), 2 * U * np.abs(want_dx), "dx")
    print(f"D={D}: worst |err| / bound: inv {r_inv:.3f}, dx {r_dx:.3f}")
    assert r_inv <= 1.0 and r_dx <= 1.0
    assert base["inv"][3] == np.float32(1.0 / eps) == base["inv"][7] and not base["dx"][3].any() and not base["dx"][7].any()
    for extra, offset in ((0, 1), (3, 0), (3, 1), (4, 0), (4, 1)):
        other = run_norm(x, eps, ginv, extra, offset)
        assert not other["dx"][:, D:].any()
        same_bits(base, dict(other, dx=other["dx"][:, :D]), f"D={D} ld=D+{extra} offset={offset}")
    empty = run_norm(np.zeros((0, D), np.float32), eps, np.zeros(0, np.float32))
    assert empty["inv"].shape == (0,) and empty["dx"].shape == (0, D)


# ----------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("head", ["plain", "aam"])
def test_autograd_functions_are_the_kernels(head):
    B, N = ops.loss_slot_rows() + 3, 257
    c = gaussian(head, B, N)
    kind, margin, scale, cosine = c["head"]
    want = run_loss(c)
    tz = _dev(c["z"]).requires_grad_(True)
    tix = _dev(c["ix"]).requires_grad_(True) if cosine else None
    tiw = _dev(c["iw"]).requires_grad_(True) if cosine else None
    loss, pred = A.margin_softmax_loss(tz, _dev(c["labels"]), kind, margin, scale, tix, tiw)         # int64 labels
    assert loss.shape == (B,) and pred.dtype == torch.int32 and not pred.requires_grad
    loss.backward(_dev(c["gloss"]))
    pairs = [(loss.detach(), "loss"), (pred, "pred"), (tz.grad, "dz")] + ([(tix.grad, "dinv_x"), (tiw.grad, "dinv_w")] if cosine else [])
    for got, k in pairs:
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want[k])), k
    # labels far outside int32 mark ignored rows
    far = _dev(c["labels"]).clone()
    far[0] = 2 ** 40
    again = A.margin_softmax_loss(tz.detach(), far, kind, margin, scale, tix.detach() if cosine else None, tiw.detach() if cosine else None)[0]
    assert again[0].item() == 0.0 and np.array_equal(_bits(again[1:].cpu().numpy()), _bits(want["loss"][1:]))

    rng = np.random.default_rng(3)
    x = rng.standard_normal((10, 23)).astype(np.float32)
    x[2] = 0.0
    ginv = rng.standard_normal(10).astype(np.float32)
    want_n = run_norm(x, EPS, ginv)
    tx = _dev(x).requires_grad_(True)
    inv = A.row_inv_norm(tx, EPS)
    inv.backward(_dev(ginv))
    assert np.array_equal(_bits(inv.detach().cpu().numpy()), _bits(want_n["inv"]))
    assert np.array_equal(_bits(tx.grad.cpu().numpy()), _bits(want_n["dx"]))


# ----------------------------------------------------------------------------- the whole head
def head_reference(x, w, labels, kind, margin, scale, mode, cosine=True, bias=None, cmax=0.55):
    """The fp64 restatement of ClassifierHead.forward (the mean loss of the valid rows; gradients with respect to emb and weight)
    on the operands `mode` multiplies, with a-priori bounds propagated from the GEMMs' and the loss kernels' own.

    GEMMs: |fp32 result - fp64| <= acc(n) S over n terms of magnitudes summing to S; acc(n) = (n + 2) u ("f32"; "bf16" on its bf16
    operands) or (3 n + 2) u 1.02 + (3 + 2^-6) 2^-16 ("bf16x3") -- tests/_tdnn_grad_ref.py, tests/_tdnn_grad16_ref.py. Forward:
    ez = acc(D) S. The inverse norms carry 2 u each (of the fp32 operands in every mode), so a cosine is off by
    dc = 4.01 u |c| + 1.01 |ix iw| ez and a logit by dl = scale P1 dc, P1 >= |psi'| on |c| <= cmax (asserted for the targets).
    lse is 1-Lipschitz in the largest logit error d_b of its row: |loss_b - ref| <= 2 d_b + the kernel's 2 u (|lse| + |l_y|).
    p_j moves by the factor exp(+-2 d_b): |p~ - p| <= p eta, eta = expm1(2 d_b); psi' moves by at most P2 dc_y, P2 >= |psi''|.
    Hence the error of dc_j = g s (p_j - [j=y]) psi'_j is at most Edc = g s (p eta P1_j + [j=y] (p + 1)(1 + eta) P2 dc_y) and that of
    dz at most Edz = 1.01 |ix iw| Edc + 4.01 u |dz| + 2.02 u dz_mag. The backward GEMMs multiply that dz ("bf16": rounded to bf16,
    the kernel's value and the reference's each within 2^-8 of their own: 2^-7 (|dz| + Edz) more): acc(n) (|dz| + Edz) |operand| + Edz |operand| summed. dinv_x / dinv_w (sums of dc z iw / dc z ix) take
    Edc, ez and 3.1 u per term (2 u of the norm, u of their rounding, the fp64 part); the norms' backward scales that by
    1.02 |inv^3 x| and adds 8.1 u of its own value (three factors inv, its rounding); autograd adds the two fp32 gradients: 1.01 u.
    A plain head (cosine=False, with `bias`): c = z = x . w + bias with one term more in the GEMM, no norms, and
    dbias = sum_b dz, an fp32 sum of B terms: (B + 2) u (|dz| + Edz) + Edz summed."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    B, D = x.shape
    N = w.shape[0]
    xq, wq = ((bf16_rne(x), bf16_rne(w)) if mode == "bf16" else (x, w))
    x64, w64, xq, wq = (a.astype(np.float64) for a in (x, w, xq, wq))
    acc = (lambda n: (3 * n + 2) * U * 1.02 + X3_OPERANDS) if mode == "bf16x3" else (lambda n: (n + 2) * U)
    z, ez = xq @ wq.T, acc(D) * (np.abs(xq) @ np.abs(wq).T)
    ix = iw = None
    if cosine:
        ix, iw = R.inv_norm(x64, EPS)["inv"], R.inv_norm(w64, EPS)["inv"]
    if bias is not None:
        b64 = np.asarray(bias, np.float32).astype(np.float64)
        z, ez = z + b64, acc(D + 1) * (np.abs(xq) @ np.abs(wq).T + np.abs(b64))
    f = R.forward(z, labels, ix, iw, kind, margin, scale)
    valid = f["valid"]
    nv = max(int(valid.sum()), 1)
    gl = np.full(B, 1.0 / nv)
    g = R.backward(z, labels, ix, iw, kind, margin, scale, f["lse"], gl)
    cm, sm = math.cos(margin), math.sin(margin)
    P1 = cm + sm * cmax / math.sqrt(1 - cmax * cmax) if kind == "aam" else 1.0
    P2 = sm / (1 - cmax * cmax) ** 1.5 if kind == "aam" else 0.0
    assert cmax < cm
    hot, slope, p = np.zeros((B, N)), np.ones((B, N)), np.zeros((B, N))
    for b in np.flatnonzero(valid):
        y = int(labels[b])
        assert kind != "aam" or abs(f["c"][b, y]) <= cmax - 1e-3, (b, f["c"][b, y])
        hot[b, y], slope[b, y] = 1.0, R.psi(f["c"][b, y], kind, margin)[1]
        l = scale * f["c"][b]
        l[y] = f["ly"][b]
        p[b] = np.exp(l - f["lse"][b])
    Aw = np.abs(ix)[:, None] * np.abs(iw)[None, :] if cosine else np.ones((B, N))
    dcos = (4.01 * U * np.abs(f["c"]) if cosine else 0.0) + 1.01 * Aw * ez
    d = (scale * P1 * dcos).max(axis=1)
    eta = np.expm1(2 * d)[:, None]
    loss = f["loss"].sum() / nv
    loss_bound = float(((2 * d + 2.02 * U * (np.abs(f["lse"]) + np.abs(f["ly"]))) * valid).sum() / nv + (B + 2) * U * 1.01 * abs(loss))
    gs = (gl * scale)[:, None] * valid[:, None]
    dc = gs * (p - hot) * slope
    dcos_y = (dcos * hot).sum(axis=1)[:, None]
    Edc = gs * (p * eta * np.where(hot > 0, P1, 1.0) + hot * (p + 1) * (1 + eta) * P2 * dcos_y)
    Edz = 1.01 * Aw * Edc + 4.01 * U * np.abs(g["dz"]) + 2.02 * U * g["dz_mag"] + TINY
    gz, Eg = g["dz"], Edz
    if mode == "bf16":
        gz = bf16_rne(g["dz"].astype(np.float32)).astype(np.float64)
        Eg = Edz + 2.0 ** -7 * (np.abs(g["dz"]) + Edz)
    gabs = np.abs(gz) + Eg
    dxg, dwg = gz @ wq, gz.T @ xq
    Edxg = acc(N) * (gabs @ np.abs(wq)) + Eg @ np.abs(wq)
    Edwg = acc(B) * (gabs.T @ np.abs(xq)) + Eg.T @ np.abs(xq)
    out = dict(loss=loss, loss_bound=loss_bound, pred=f["pred"], gap=f["gap"])
    if not cosine:
        return dict(out, dx=dxg, dw=dwg, dx_bound=Edxg, dw_bound=Edwg, db=gz.sum(0), db_bound=(B + 2) * U * gabs.sum(0) + Eg.sum(0))
    moved = Edc * (np.abs(z) + ez) + np.abs(dc) * ez
    Edix = 1.01 * (moved @ np.abs(iw)) + 3.1 * U * g["dinv_x_abs"]
    Ediw = 1.01 * (moved.T @ np.abs(ix)) + 3.1 * U * g["dinv_w_abs"]
    dxn, dwn = R.inv_norm_backward(x64, EPS, ix, g["dinv_x"]), R.inv_norm_backward(w64, EPS, iw, g["dinv_w"])
    Edxn = 1.02 * (np.abs(ix) ** 3 * Edix)[:, None] * np.abs(x64) + 8.1 * U * np.abs(dxn) + TINY
    Edwn = 1.02 * (np.abs(iw) ** 3 * Ediw)[:, None] * np.abs(w64) + 8.1 * U * np.abs(dwn) + TINY
    return dict(out, dx=dxg + dxn, dw=dwg + dwn,
                dx_bound=Edxg + Edxn + 1.01 * U * (np.abs(dxg) + np.abs(dxn)), dw_bound=Edwg + Edwn + 1.01 * U * (np.abs(dwg) + np.abs(dwn)))


@pytest.mark.parametrize("kind", ["aam", "am", "softmax"])
@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16x3"])
def test_classifier_head_against_the_restatement(mode, kind):
    B, D, N = 2 * ops.loss_slot_rows() + 3, 64, 300
    rng = np.random.default_rng(21)
    torch.manual_seed(21)
    x = rng.standard_normal((B, D)).astype(np.float32)
    labels = _labels(B, N, rng)
    head = A.ClassifierHead(D, N, kind=kind, gemm=mode, normalize=True, device=DEV)
    assert head.normalize and head.scale == 30.0 and head.margin == (0.0 if kind == "softmax" else 0.2)
    w = head.weight.detach().cpu().numpy()
    ref = head_reference(x, w, labels, kind, head.margin, head.scale, mode)
    emb = _dev(x).requires_grad_(True)
    loss, pred = head(emb, _dev(labels))
    loss.backward()
    ratios = {"loss": abs(loss.item() - ref["loss"]) / ref["loss_bound"],
              "demb": float((np.abs(emb.grad.cpu().numpy() - ref["dx"]) / ref["dx_bound"]).max()),
              "dweight": float((np.abs(head.weight.grad.cpu().numpy() - ref["dw"]) / ref["dw_bound"]).max())}
    print(f"ClassifierHead {kind} gemm={mode}: loss {loss.item():.6f}, worst |err| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    sure = ref["gap"] > 1e-3                                      # far beyond what the GEMM's error moves a cosine by
    assert np.array_equal(pred.cpu().numpy()[sure], ref["pred"][sure])
    with torch.no_grad():
        cos = head.cosines(emb)
    assert cos.shape == (B, N) and float(cos.abs().max()) <= 1.0 + 1e-5
    assert np.array_equal(cos.argmax(1).cpu().numpy()[sure], ref["pred"][sure])


def test_classifier_head_plain_with_bias_and_schedules():
    """The plain head is `cross_entropy` of the affine; margin and scale are read at every call; a batch without a valid row gives 0."""
    B, D, N = 9, 32, 70
    rng = np.random.default_rng(22)
    x, labels = rng.standard_normal((B, D)).astype(np.float32), rng.integers(0, N, B)
    labels[3] = -1
    head = A.ClassifierHead(D, N, kind="softmax", bias=True, device=DEV)
    with torch.no_grad():
        head.bias.copy_(_dev(rng.standard_normal(N).astype(np.float32)))
    emb = _dev(x).requires_grad_(True)
    loss, pred = head(emb, _dev(labels))
    loss.backward()
    p64 = [t.detach().cpu().double().requires_grad_(True) for t in (emb, head.weight, head.bias)]
    ce = torch.nn.functional.cross_entropy(p64[0] @ p64[1].T + p64[2], torch.as_tensor(labels), ignore_index=-1)
    ce.backward()
    ref = head_reference(x, head.weight.detach().cpu().numpy(), labels, "softmax", 0.0, 1.0, "f32", cosine=False,
                         bias=head.bias.detach().cpu().numpy())
    assert abs(ref["loss"] - ce.item()) <= 1e-12 * abs(ce.item())            # the restatement is torch's cross_entropy
    for k, want in zip(("dx", "dw", "db"), p64):
        assert np.abs(ref[k] - want.grad.numpy()).max() <= 1e-12
    ratios = {"loss": abs(loss.item() - ref["loss"]) / ref["loss_bound"]}
    for k, got in (("dx", emb.grad), ("dw", head.weight.grad), ("db", head.bias.grad)):
        ratios[k] = float((np.abs(got.cpu().numpy() - ref[k]) / ref[k + "_bound"]).max())
    print("ClassifierHead plain with bias: worst |err| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert not emb.grad[3].any()

    aam = A.ClassifierHead(D, N, device=DEV)
    with torch.no_grad():
        seen = []
        for aam.margin in (0.0, 0.1, 0.2):                        # a warm-up: one assignment per step
            seen.append(aam(emb, _dev(labels))[0].item())
        assert seen[0] < seen[1] < seen[2]
        aam.scale = 15.0
        assert aam(emb, _dev(labels))[0].item() != seen[2]
        none, pred = aam(emb, _dev(np.full(B, -1)))
        assert none.item() == 0.0 and pred.shape == (B,)


# ----------------------------------------------------------------------------- the network (that of test_gpu_tdnn_grad.py / test_gpu_norm.py)
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
    """8 utterances of 40-90 frames, 4 speakers: a speaker-dependent offset under unit noise."""
    rng = np.random.default_rng(seed)
    labels = np.arange(len(NET_LENS)) % CLASSES
    centres = rng.standard_normal((CLASSES, FEAT))
    feats = (rng.standard_normal((len(NET_LENS), max(NET_LENS), FEAT)) + centres[labels][:, None, :]).astype(np.float32)
    return feats, labels


def _restated_bn(x, lens, gamma, eps):
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


@pytest.mark.parametrize("N", [8, 1000])
def test_training_the_network_with_an_aam_head(N):
    """The five-GEMM network of test_gpu_tdnn_grad.py / test_gpu_norm.py (fused_norm=True) under an AAM ClassifierHead. First-step
    gradients against the fp64 restatement within the bound of those tests: per parameter tensor
    |got - ref| <= 14 * (n + 2) * 2^-24 * 8 * max|ref| with n = 8 * 90 rows; then 30 SGD steps."""
    seq = _stack()
    feats, labels = _problem()
    torch.manual_seed(5)
    net = A.TrainableSequential(seq, fused_norm=True).train()
    head = A.ClassifierHead(UNITS, N, kind="aam", margin=0.2, scale=16.0, device=DEV)
    tf_, tl, ty = torch.as_tensor(feats, device=DEV), torch.as_tensor(NET_LENS, device=DEV), torch.as_tensor(labels, device=DEV)

    loss, pred = head(net(tf_, tl), ty)
    loss.backward()
    first_acc = float((pred.cpu().numpy() == labels).mean())
    params = list(net.params) + [head.weight]
    ref_params = [p.detach().cpu().to(torch.float64).requires_grad_(True) for p in params]
    emb = _restated_net(seq, ref_params[:-1], torch.tensor(feats, dtype=torch.float64), NET_LENS)
    w64 = ref_params[-1]
    ref_loss = torch_loss(emb @ w64.T, torch.tensor(labels), torch_inv_norm(emb, EPS), torch_inv_norm(w64, EPS), "aam", 0.2, 16.0).mean()
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
    factor = 14 * (8 * 90 + 2) * U * 8
    worst = 0.0
    for i, (p, r) in enumerate(zip(params, ref_params)):
        err = float((p.grad.cpu().to(torch.float64) - r.grad).abs().max())
        scale = float(r.grad.abs().max())
        worst = max(worst, err / (factor * scale))
        print(f"parameter {i} {tuple(p.shape)}: max |err| {err:.3e}, max |ref| {scale:.3e}, bound {factor * scale:.3e}")
        assert err <= factor * scale, (i, err, factor * scale)
    print(f"N={N}: worst |err| / bound over the parameters {worst:.4f}")

    opt = torch.optim.SGD(list(net.parameters()) + list(head.parameters()), lr=0.05)
    losses = [loss.item()]
    for _ in range(30):
        opt.zero_grad()
        step_loss, pred = head(net(tf_, tl), ty)
        step_loss.backward()
        opt.step()
        losses.append(step_loss.item())
    last_acc = float((pred.cpu().numpy() == labels).mean())
    print(f"N={N}: loss first {losses[0]:.4f}, after 30 steps {losses[-1]:.4f}; accuracy {first_acc:.3f} -> {last_acc:.3f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert last_acc > first_acc

    # export is what it was: the layers hold the network's parameters bit for bit, the head is not part of the Sequential
    assert net.export() is seq
    it = iter(net.params)
    for l in seq.layers:
        if isinstance(l, ktf.layers.TDNN):
            kernel, bias = l.get_weights()
            assert np.array_equal(_bits(kernel[0].transpose(2, 0, 1)), _bits(next(it).detach().cpu().numpy()))
            assert np.array_equal(_bits(bias), _bits(next(it).detach().cpu().numpy()))
        elif isinstance(l, ktf.layers.BatchNorm):
            gamma = l.get_weights()[0]
            assert np.array_equal(_bits(gamma), _bits(next(it).detach().cpu().numpy()))
