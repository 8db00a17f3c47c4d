"""The head's loss kernels with sub-centres, the inter-top-k penalty and label smoothing (include/ktf_head.h) on the GPU against the
fp64 oracle of tests/_head_ref.py, and ktf.autograd.margin_softmax_loss / ClassifierHead over them.

Exact outputs: pred, sub_y and hard. The cosines are fp64 products of the fp32 inputs in a fixed order, which NumPy forms with the
same roundings, so the oracle's selection is the kernels' on every input: no tolerance, no "sure" rows.

Bounds, of the form tests/test_gpu_loss.py uses and derives (u = 2^-24; every output is fp64 arithmetic rounded once, the bounds leave
a factor 2; |l| <= 64 + scale * penalty and N <= 8192, asserted, keep the fp64 part below 2^-38 (1 + |lse|)):
    lse      |got - ref| <= 2^-38 (1 + |ref|)                                  (fp64)
    loss     |got - ref| <= 2 u (|lse| + (1 - e) |l_y| + e |mean l|)
    dz       |got - ref| <= 2 u |gloss scale psi' inv_x inv_w| (p_j + [j = y] + e ([j = y] + 1 / N))
    dinv_*   |got - ref| <= u |S| + 2^-36 sum |terms|
The columns of dz of the centres that were not selected, and dinv_w of a centre no row selected, are exactly 0 (their bound is 0).
The bounds of the whole head (`head_reference`) are those of test_gpu_loss.head_reference with the terms of H2 and H3 added."""

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

from kaldi_tflite_amd import autograd as A, ops  # noqa: E402
import _head_ref as H  # noqa: E402
import _loss_ref as R  # noqa: E402
from _tdnn16_ref import X3_OPERANDS, bf16_rne  # noqa: E402
import test_gpu_loss as T  # noqa: E402
from test_gpu_loss import DEV, EPS, NAN, TINY, U, _bits, _dev, _labels, _ratio, _strided, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
# name -> (kind, margin, scale, cosine head)
HEADS = T.HEADS
PEN = 0.06


def run_head(c, extra=0, offset=0, inplace=False, gloss="case", want_opt=True):
    """Both calls on fresh buffers whose outputs start as NaN (-7 for the integers), the workspace as 0xFF bytes. Returns numpy: loss,
    pred, sub_y, hard, lse, dz with its pad columns, dinv_x, dinv_w (None for a plain head)."""
    z, K, topk, pen, eps = c["z"], c["K"], c["topk"], c["pen"], c["eps"]
    B, NK = z.shape
    N = NK // K
    kind, margin, scale, cosine = c["head"]
    zf = _strided(z, extra, offset)
    tl, ix, iw = _dev(c["labels"].astype(np.int32)), _dev(c["ix"]), _dev(c["iw"])
    gl = _dev(c["gloss"] if isinstance(gloss, str) else gloss)
    loss = torch.full((B,), NAN, dtype=torch.float32, device=DEV)
    pred = torch.full((B,), -7, dtype=torch.int32, device=DEV) if want_opt else None
    sub_y = torch.full((B,), -7, dtype=torch.int32, device=DEV) if want_opt else None
    hard = torch.full((B, max(topk, 1)), -7, dtype=torch.int32, device=DEV) if (want_opt or topk) else None
    lse = torch.full((B,), NAN, dtype=torch.float64, device=DEV)
    ws = ops.head_workspace(B, N, K, DEV)
    ws.fill_(0xFF)
    ops.head_forward(zf[:, :NK], K, tl, ix, iw, kind, margin, scale, topk, pen, eps, loss, pred, lse, hard, sub_y, ws)
    dzf = zf if inplace else _strided(np.full((B, NK), NAN, np.float32), extra, offset)
    dix = torch.full((B,), NAN, dtype=torch.float32, device=DEV) if cosine else None
    diw = torch.full((NK,), NAN, dtype=torch.float32, device=DEV) if cosine else None
    ops.head_backward(zf[:, :NK], K, tl, ix, iw, kind, margin, scale, topk, pen, eps, lse, hard, gl, dzf, dix, diw, ws)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return dict(loss=host(loss), pred=host(pred), sub_y=host(sub_y), hard=host(hard), lse=host(lse), dz=host(dzf), dinv_x=host(dix),
                dinv_w=host(diw))


def make_case(head, K, topk, eps, z, labels, ix, iw, gloss, pen=None):
    """The inputs (read-only from here on) and their oracle. head: a name of HEADS or such a tuple; z (B, N * K) class-major."""
    head = HEADS.get(head, head) if isinstance(head, str) else head
    kind, margin, scale, cosine = head
    pen = (PEN if topk else 0.0) if pen is None else pen
    z, labels = np.asarray(z, np.float32), np.asarray(labels)
    ix = np.asarray(ix, np.float32) if cosine else None
    iw = np.asarray(iw, np.float32) if cosine else None
    gloss = None if gloss is None else np.asarray(gloss, np.float32)
    f = H.forward(z, labels, ix, iw, kind, margin, scale, K, topk, pen, eps)
    g = H.backward(z, labels, ix, iw, kind, margin, scale, K, topk, pen, eps, f["lse"], f["hard"], gloss)
    assert np.abs(scale * f["c"]).max(initial=0.0) <= 64.0 and np.abs(f["ly"]).max(initial=0.0) <= 64.0 and z.shape[1] // K <= 8192
    for a in (z, labels, ix, iw, gloss):
        if a is not None:
            a.setflags(write=False)
    return dict(head=head, K=K, topk=topk, pen=pen, eps=eps, z=z, labels=labels, ix=ix, iw=iw, gloss=gloss, f=f, g=g)


@functools.lru_cache(maxsize=None)
def gaussian(head, B, N, K, topk, eps):
    """A Gaussian batch and its oracle, computed once and shared by the tests that use it (read-only). Cosine heads: |c| < 1."""
    rng = np.random.default_rng(1000 * B + 10 * N + K)
    if HEADS[head][3]:
        z = np.clip(rng.standard_normal((B, N * K)), -2.4, 2.4)
    else:
        z = np.clip(4.0 * rng.standard_normal((B, N)), -40.0, 40.0) + rng.uniform(-8.0, 8.0, N)[None, :]
    gloss = rng.standard_normal(B)
    if B > 4:
        gloss[4] = 0.0
    return make_case(head, K, topk, eps, z, _labels(B, N, rng), rng.uniform(0.2, 0.4, B), rng.uniform(0.5, 1.0, N * K), gloss)


def check_against_oracle(got, c, tag):
    f, g = c["f"], c["g"]
    B, NK = c["z"].shape
    eps = c["eps"]
    assert not np.isnan(got["loss"]).any() and not np.isnan(got["lse"]).any() and not np.isnan(got["dz"]).any(), tag
    assert not got["dz"][:, NK:].any(), tag                      # the pad columns are written as zero
    for k in ("pred", "sub_y", "hard"):                          # exact, on every input
        if got[k] is not None:
            assert got[k].shape == f[k].shape and np.array_equal(got[k], f[k]), (tag, k, got[k], f[k])
    lse_err = np.abs(got["lse"] - f["lse"])
    print(f"{tag}: max lse error / bound {float((lse_err / (2.0 ** -38 * (1 + np.abs(f['lse'])))).max(initial=0.0)):.3f}")
    assert (lse_err <= 2.0 ** -38 * (1 + np.abs(f["lse"]))).all(), (tag, lse_err.max(initial=0.0))
    ratios = {}
    loss_bound = 2 * U * (np.abs(f["lse"]) + (1 - eps) * np.abs(f["ly"]) + eps * np.abs(f["lmean"])) * f["valid"]
    ratios["loss"] = _ratio(np.abs(got["loss"] - f["loss"]), loss_bound, "loss")
    ratios["dz"] = _ratio(np.abs(got["dz"][:, :NK] - g["dz"]), 2 * U * g["dz_mag"], "dz")        # a zero bound asks for an exact zero
    assert not got["dz"][:, :NK][:, ~g["selected"]].any(), tag
    if c["ix"] is not None:
        for k in ("dinv_x", "dinv_w"):
            assert not np.isnan(got[k]).any(), (tag, k)
            ratios[k] = _ratio(np.abs(got[k] - g[k]), U * np.abs(g[k]) + 2.0 ** -36 * g[k + "_abs"], k)
        assert not got["dinv_w"][~g["selected"]].any(), tag
    else:
        assert got["dinv_x"] is None and got["dinv_w"] is None
    print(f"{tag}: worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (tag, ratios)
    return ratios


def _cut(got, NK):
    return dict(got, dz=got["dz"][:, :NK])


def _switches(N, cosine):
    """(topk, smoothing) pairs: topk of 0, 1, 5, 64, N - 1 and N + 3 where allowed, both smoothings."""
    if not cosine:
        return [(0, 0.0), (0, 0.1)]
    ks = [k for k in (0, 1, 5, 64, N - 1, N + 3) if 0 <= k <= 64]
    return sorted({(k, (0.0, 0.1)[i % 2]) for i, k in enumerate(ks)} | {(0, 0.1), (5, 0.1)})


# ----------------------------------------------------------------------------- rounding bounds: every width, centre count, stride and base
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("head,K", [(h, K) for h in HEADS for K in (1, 2, 3) if K == 1 or HEADS[h][3]])     # K > 1: cosine heads (H7)
def test_gaussian_inputs_within_the_bounds_on_every_stride(head, K, N):
    """ld = NK, NK + 3, NK + 4 with the base on and one float off a 16-byte boundary. One path (H5): the bits are the same."""
    cosine = HEADS[head][3]
    B = ops.head_slot_rows() + 1
    for topk, eps in _switches(N, cosine):
        c = gaussian(head, B, N, K, topk, eps)
        base = run_head(c)
        tag = f"{head} B={B} N={N} K={K} topk={topk} e={eps}"
        check_against_oracle(base, c, tag)
        if (topk, eps) in ((0, 0.1), (5, 0.1), (64, 0.1)):
            for extra, offset in ((0, 1), (3, 0), (3, 1), (4, 0), (4, 1)):
                other = run_head(c, extra=extra, offset=offset)
                assert not other["dz"][:, N * K:].any()
                same_bits(_cut(base, N * K), _cut(other, N * K), f"{tag} ld=NK+{extra} offset={offset}")


@pytest.mark.parametrize("B", [0, 1, 7, 8, 9, 19])
@pytest.mark.parametrize("head,K,topk", [("plain", 1, 0), ("aam", 2, 5), ("am", 3, 64)])
def test_batch_sizes_around_the_slots(head, K, topk, B):
    assert ops.head_slot_rows() == 8
    N = 257
    c = gaussian(head, B, N, K, topk, 0.1)
    got = run_head(c, extra=3, offset=1)
    check_against_oracle(got, c, f"{head} B={B} N={N} K={K}")
    if B == 0:
        assert got["dz"].shape == (0, N * K + 3) and got["hard"].shape == (0, max(topk, 1))
        if got["dinv_w"] is not None:
            assert got["dinv_w"].shape == (N * K,) and not got["dinv_w"].any()       # H6: the sum over no row


def test_one_large_case():
    c = gaussian("aam", 19, 7323, 2, 5, 0.1)
    first, second = run_head(c, extra=4), run_head(c, extra=4)
    check_against_oracle(first, c, "aam B=19 N=7323 K=2")
    same_bits(first, second, "the same call twice")


# ----------------------------------------------------------------------------- bits
@pytest.mark.parametrize("head,N", [("plain", 257), ("softmax", 65), ("am", 1000), ("aam", 7323)])
def test_with_everything_off_the_outputs_are_those_of_the_plain_loss_kernels(head, N):
    """K = 1, topk = 0, smoothing = 0: every output equals the call of ktf_loss.h on the same inputs bit for bit (H5)."""
    B = 19
    old = T.gaussian(head, B, N)
    c = make_case(head, 1, 0, 0.0, old["z"], old["labels"], old["ix"], old["iw"], old["gloss"])
    for extra, offset, inplace in ((0, 0, False), (3, 1, False), (4, 0, True)):
        want = T.run_loss(old, extra=extra, offset=offset, inplace=inplace)
        got = run_head(c, extra=extra, offset=offset, inplace=inplace)
        assert (got["hard"] == -1).all() and np.array_equal(got["sub_y"], np.where(c["f"]["valid"], 0, -1))
        same_bits(want, {k: got[k] for k in want}, f"{head} N={N} ld=N+{extra} offset={offset} inplace={inplace}")
    check_against_oracle(got, c, f"{head} N={N} all off")


@pytest.mark.parametrize("head,N,K,topk", [("aam", 1000, 2, 5), ("plain", 257, 1, 0), ("am", 257, 3, 64), ("softmax", 64, 2, 1)])
def test_determinism_in_place_and_pad_columns(head, N, K, topk):
    B, NK = 19, N * K
    c = gaussian(head, B, N, K, topk, 0.1)
    first, second = run_head(c, extra=4), run_head(c, extra=4)
    same_bits(first, second, "the same call twice")
    check_against_oracle(first, c, f"{head} B={B} N={N} K={K}")
    for extra, offset in ((0, 0), (3, 1), (4, 0)):                # _strided poisons z's pad columns with NaN: never read
        apart, inplace = run_head(c, extra=extra, offset=offset), run_head(c, extra=extra, offset=offset, inplace=True)
        assert not inplace["dz"][:, NK:].any()                    # the NaN pad of z, now dz's, written as zero
        same_bits(apart, inplace, f"in place, ld=NK+{extra}")
        same_bits(_cut(first, NK), _cut(apart, NK), f"ld=NK+{extra} against ld=NK+4")
    # NaN in the gloss of the ignored rows, and none of the optional outputs: the same bits
    assert list(c["labels"][:4]) == [0, N - 1, -1, N]
    poisoned = c["gloss"].copy()
    poisoned[[2, 3]] = NAN
    other = run_head(c, extra=4, gloss=poisoned, want_opt=False)
    assert other["pred"] is None and other["sub_y"] is None
    keep = ("loss", "lse", "dz", "dinv_x", "dinv_w") + (("hard",) if topk else ())
    same_bits({k: first[k] for k in keep}, {k: other[k] for k in keep}, "NaN gloss of ignored rows")


# ----------------------------------------------------------------------------- exact selection
@pytest.mark.parametrize("K,topk", [(1, 5), (2, 1), (2, 64), (3, 5)])
def test_selection_on_exact_ties(K, topk):
    """Small integers over 4 with unit norms: exact cosines that repeat all over a row -- between the centres of a class, between
    classes at the top-k boundary, across the target, and rows whose target holds the largest cosine; duplicated columns besides."""
    B, N = 9, 1000
    rng = np.random.default_rng(40 + K)
    z = rng.integers(-3, 3, (B, N, K)).astype(np.float32)
    labels = rng.integers(0, N, B)
    labels[0], labels[1], labels[2] = 0, N - 1, 300
    z[0, 0, :] = 3.0                                              # the target holds the largest cosine, in every centre
    z[1] = np.minimum(z[1], 1.0)
    z[1, [5, 256, 257, 999], K - 1] = 2.0                         # the target among the four equal maxima, on both sides of a chunk edge
    z[2, 300, 0] = 2.0                                            # ties across the target: equal classes below and above it
    z[3, :, :] = z[3, :, :1]                                      # every centre of a class equal: the lowest k
    z[4] = 1.0                                                    # one value in the whole row
    z[5, 1::2] = z[5, 0::2]                                       # duplicated weight rows: z repeats class by class
    z[6, :, :] = -0.0
    z[6, ::3, 0] = 0.0                                            # +0 and -0 are equal
    z = z.reshape(B, N * K) / 4.0
    for head in ("softmax", "aam"):
        c = make_case(head, K, topk, 0.1, z, labels, np.ones(B), np.ones(N * K), rng.standard_normal(B))
        f = c["f"]
        assert f["pred"][0] == 0 and f["sub_y"][0] == 0 and 0 not in f["hard"][0]
        assert (np.sort(f["hard"][1][:3]) == [5, 256, 257]).all() if topk >= 3 else f["hard"][1][0] == 5
        assert list(f["hard"][4][:min(topk, 3)]) == [j for j in range(4) if j != labels[4]][:min(topk, 3)]
        assert (f["kstar"][3] == 0).all()
        got = run_head(c, extra=3, offset=1)
        check_against_oracle(got, c, f"ties {head} K={K} topk={topk}")


@pytest.mark.parametrize("topk", [5, 9, 64])
def test_selection_when_few_threads_hold_the_members(topk):
    """The forward kernel keeps four classes per thread in registers and reads a thread's classes again when more of them are
    members: classes 3, 259, 515, ... (one thread's, eleven of them) and 200, 456, ... hold the largest cosines, in mixed order and
    with equal values among them; row 2 has them all equal; in row 3 the target is one of them."""
    B, N, K = 4, 2600, 2
    rng = np.random.default_rng(50)
    z = rng.uniform(-0.5, 0.5, (B, N, K)).astype(np.float32)
    mine, other = np.arange(3, N, 256), np.arange(200, N, 256)
    assert len(mine) == 11 and len(other) == 10
    z[0, mine, 1] = 0.5 + rng.permutation(11) / 32.0
    z[1, mine, 0] = 0.5 + rng.integers(0, 3, 11) / 8.0
    z[1, other, 1] = 0.5 + rng.integers(0, 3, 10) / 8.0
    z[2, mine, 0], z[2, other, 0] = 0.75, 0.75
    z[3, mine, 1] = 0.5 + rng.permutation(11) / 32.0
    labels = np.array([0, N - 1, 7, 515])
    c = make_case("aam", K, topk, 0.1, z.reshape(B, N * K), labels, np.ones(B), np.ones(N * K), rng.standard_normal(B))
    f = c["f"]
    assert set(f["hard"][0][:min(topk, 11)]) <= set(mine) and list(f["hard"][2][:min(topk, 21)]) == sorted(set(mine) | set(other))[:min(topk, 21)]
    assert 515 not in f["hard"][3] and set(f["hard"][3][:min(topk, 10)]) <= set(mine)
    got = run_head(c, extra=3, offset=1)
    check_against_oracle(got, c, f"one thread's classes, topk={topk}")


# ----------------------------------------------------------------------------- corners
def test_ignored_rows_single_rows_and_gloss():
    B, N, K, topk, eps = 11, 65, 2, 5, 0.1
    c = gaussian("aam", B, N, K, topk, eps)
    assert list(c["labels"][:4]) == [0, N - 1, -1, N] and c["gloss"][4] == 0.0
    got = run_head(c)
    check_against_oracle(got, c, "labels 0, N - 1, -1, N")
    for b in (2, 3):
        assert got["loss"][b] == 0 and not got["dz"][b].any() and got["dinv_x"][b] == 0 and got["sub_y"][b] == -1 and (got["hard"][b] == -1).all()
    assert not got["dz"][4].any() and got["dinv_x"][4] == 0      # gloss = 0
    ones = make_case("aam", K, topk, eps, c["z"], c["labels"], c["ix"], c["iw"], np.ones(B))
    null = make_case("aam", K, topk, eps, c["z"], c["labels"], c["ix"], c["iw"], None)
    got_ones, got_null = run_head(ones), run_head(null)
    check_against_oracle(got_null, null, "gloss NULL")
    same_bits(got_ones, got_null, "gloss NULL against ones")
    none = make_case("aam", K, topk, eps, c["z"], np.where(np.arange(B) % 2, -1, N), c["ix"], c["iw"], c["gloss"])
    got_none = run_head(none)
    check_against_oracle(got_none, none, "every row ignored")
    assert not got_none["loss"].any() and not got_none["dz"].any() and not got_none["dinv_x"].any() and not got_none["dinv_w"].any()
    assert (got_none["hard"] == -1).all() and (got_none["sub_y"] == -1).all() and np.array_equal(got_none["pred"], got["pred"])
    labels = np.full(B, -1)
    labels[9] = 7                                                 # one valid row, in the second slot
    one = make_case("aam", K, topk, eps, c["z"], labels, c["ix"], c["iw"], c["gloss"])
    got_one = run_head(one)
    check_against_oracle(got_one, one, "one valid row")
    assert got_one["loss"][9] > 0 and np.count_nonzero(got_one["loss"]) == 1 and np.count_nonzero(got_one["dinv_x"]) == 1
    assert np.count_nonzero(got_one["dinv_w"]) == N == np.count_nonzero(got_one["dz"][9])      # one centre per class


@pytest.mark.parametrize("head", list(HEADS))
def test_a_single_class_gives_exact_zeros(head):
    B = 5
    rng = np.random.default_rng(9)
    cosine = HEADS[head][3]
    for K, topk in ((1, 0), (2, 3)) if cosine else ((1, 0),):
        c = make_case(head, K, topk, 0.1, rng.uniform(-0.9, 0.9, (B, K)), [0, 0, -1, 1, 0], np.ones(B), np.ones(K), rng.standard_normal(B))
        for extra in (0, 3):
            got = run_head(c, extra=extra)
            assert not got["loss"].any() and not got["dz"].any() and not got["pred"].any() and (got["hard"] == -1).all()
            check_against_oracle(got, c, f"{head} N=1 K={K}")


def test_extreme_logits():
    """+64 and -64 in one row, with smoothing: every other probability underflows, no NaN; a cosine head at scale 64 with c = +-1."""
    N = 70
    z = np.zeros((3, N), np.float32)
    z[0, 0], z[0, 1] = 64.0, -64.0
    z[1, 5], z[1, 6] = -64.0, 64.0
    z[2, :] = -64.0
    c = make_case("plain", 1, 0, 0.1, z, [0, 5, 3], None, None, None)
    got = run_head(c)
    check_against_oracle(got, c, "logits of +-64")
    assert np.isfinite(got["dz"]).all() and got["pred"][1] == 6 and got["pred"][2] == 0
    zc = np.zeros((2, N, 2), np.float32)
    zc[0, 0], zc[0, 1], zc[1, 2], zc[1, 3] = (1.0, -1.0), (-1.0, -1.0), (-1.0, -1.0), (0.5, 1.0)
    cc = make_case(("am", 0.0, 64.0, True), 2, 3, 0.1, zc.reshape(2, 2 * N), [0, 2], np.ones(2), np.ones(2 * N), None, pen=0.0)
    got = run_head(cc)
    check_against_oracle(got, cc, "cosines of +-1 at scale 64")
    assert np.isfinite(got["dz"]).all() and np.isfinite(got["dinv_w"]).all() and list(got["sub_y"]) == [0, 0]


def test_aam_targets_on_every_branch():
    """Target cosines on both sides of -cos m and of the sine floor, at +-1 and marginally above 1 (unit norms: c = z), held by the
    second of two centres; the first lies below it."""
    kind, m, scale, _ = HEADS["aam"]
    cm = math.cos(m)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    up, down = f32(np.nextafter(np.float32(-cm), np.float32(1))), f32(np.nextafter(np.float32(-cm), np.float32(-1)))
    edge = math.sqrt(1.0 - R.SIN2_FLOOR)
    below_floor, above_floor = f32(np.nextafter(np.float32(edge), np.float32(2))), f32(np.nextafter(np.float32(edge), np.float32(0)))
    targets = [up, down, above_floor, below_floor, 1.0, -1.0, 1.0 + 2.0 ** -23, 0.3, -0.97]
    B, N, K = len(targets), 130, 2
    rng = np.random.default_rng(5)
    z = rng.uniform(-0.5, 0.5, (B, N, K)).astype(np.float32)
    labels = rng.integers(0, N, B)
    labels[0], labels[1] = 0, N - 1
    for b, t in enumerate(targets):
        z[b, labels[b]] = (t - 0.25, t)
    c = make_case("aam", K, 5, 0.1, z.reshape(B, N * K), labels, np.ones(B), np.ones(N * K), rng.standard_normal(B))
    branch = [R.psi(t, kind, m)[1] for t in np.float32(targets)]
    assert branch[1] == 1.0 and branch[5] == 1.0 and branch[8] == 1.0 and branch[2] > 100 and branch[3] == branch[4] == branch[6] == cm
    assert (c["f"]["sub_y"] == 1).all()
    got = run_head(c)
    check_against_oracle(got, c, "aam branches")
    assert np.isfinite(got["dz"]).all() and np.isfinite(got["dinv_x"]).all() and np.isfinite(got["dinv_w"]).all()


# ----------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("head,K,topk,eps", [("plain", 1, 0, 0.1), ("aam", 2, 5, 0.1), ("am", 3, 0, 0.0), ("softmax", 1, 64, 0.0)])
def test_autograd_function_is_the_kernels(head, K, topk, eps):
    B, N = 11, 257
    c = gaussian(head, B, N, K, topk, eps)
    kind, margin, scale, cosine = c["head"]
    want = run_head(c)
    tz = _dev(c["z"]).requires_grad_(True)
    tix = _dev(c["ix"]).requires_grad_(True) if cosine else None
    tiw = _dev(c["iw"]).requires_grad_(True) if cosine else None
    loss, pred = A.margin_softmax_loss(tz, _dev(c["labels"]), kind, margin, scale, tix, tiw, sub_centers=K, top_k=topk, penalty=c["pen"],
                                       label_smoothing=eps)
    assert loss.shape == (B,) and pred.dtype == torch.int32 and not pred.requires_grad
    saved = [t for t in loss.grad_fn.saved_tensors if t is not None]
    assert sorted(t.numel() for t in saved if t.numel() >= B * N) == [B * N * K]          # of the logits' size: z alone
    loss.backward(_dev(c["gloss"]))
    pairs = [(loss.detach(), "loss"), (pred, "pred"), (tz.grad, "dz")] + ([(tix.grad, "dinv_x"), (tiw.grad, "dinv_w")] if cosine else [])
    for got, k in pairs:
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want[k])), k


def test_the_defaults_run_the_plain_loss_kernels():
    """A head built with the defaults: the same bits as the composition of the existing functions, and no call of ktf_head.h."""
    B, D, N = 11, 32, 70
    rng = np.random.default_rng(8)
    x, labels = rng.standard_normal((B, D)).astype(np.float32), _labels(B, N, rng)
    torch.manual_seed(8)
    head = A.ClassifierHead(D, N, device=DEV)
    assert (head.sub_centers, head.top_k, head.penalty, head.label_smoothing, head.center_counts) == (1, 0, 0.0, 0.0, None)
    calls = []
    real = ops.head_forward
    ops.head_forward = lambda *a, **k: calls.append(a) or real(*a, **k)
    try:
        emb = _dev(x).requires_grad_(True)
        loss, pred = head(emb, _dev(labels))
        loss.backward()
    finally:
        ops.head_forward = real
    assert not calls
    emb2, w2 = _dev(x).requires_grad_(True), head.weight.detach().clone().requires_grad_(True)
    z = A.tdnn_affine(emb2.unsqueeze(0), w2.unsqueeze(1), None, [0], gemm="f32").squeeze(0)
    per_row, pred2 = A._MarginSoftmax.apply(z, _dev(labels.astype(np.int32)), A.row_inv_norm(emb2, head.eps), A.row_inv_norm(w2, head.eps),
                                            "aam", 0.2, 30.0)
    valid = torch.tensor(int(((labels >= 0) & (labels < N)).sum()), device=DEV)     # a tensor, as in the head: the same division
    (per_row.sum() / valid).backward()
    for a, b in ((loss, per_row.sum() / valid), (pred, pred2), (emb.grad, emb2.grad), (head.weight.grad, w2.grad)):
        assert np.array_equal(_bits(a.detach().cpu().numpy()), _bits(b.detach().cpu().numpy()))


# ----------------------------------------------------------------------------- the whole head
def head_reference(x, w, labels, kind, margin, scale, mode, K, topk, pen, eps, cmax=0.55):
    """test_gpu_loss.head_reference for a cosine head with the switches of ktf_head.h: the fp64 restatement of
    ClassifierHead.forward on the operands `mode` multiplies, with the a-priori bounds derived there and these additions. Every
    centre's cosine is off by dcos = 4.01 u |c| + 1.01 |ix iw| ez; the restatement's selections (k* of every class, H_b) are the
    kernel's when the cosines they compare lie further apart than their errors' sum, which is asserted of the data. Then the loss
    is the same smooth function: a penalised logit carries the error of its cosine; lse, l_y and the mean logit are each 1-Lipschitz in
    the largest logit error d_b, so |loss_b - ref| <= (2 + 2 e) d_b + the kernel's 2 u (|lse| + (1 - e)|l_y| + e |mean|); the factor
    (p_j - [j=y]) + e ([j=y] - 1/N) moves as p_j does and stays below (p + 1) in magnitude, so Edc is as there; dz is zero off the
    selected centres in both."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    B, D = x.shape
    NK = w.shape[0]
    N = NK // K
    xq, wq = ((bf16_rne(x), bf16_rne(w)) if mode == "bf16" else (x, w))
    x64, w64, xq, wq = (a.astype(np.float64) for a in (x, w, xq, wq))
    acc = (lambda n: (3 * n + 2) * U * 1.02 + X3_OPERANDS) if mode == "bf16x3" else (lambda n: (n + 2) * U)
    z, ez = xq @ wq.T, acc(D) * (np.abs(xq) @ np.abs(wq).T)
    ix, iw = R.inv_norm(x64, EPS)["inv"], R.inv_norm(w64, EPS)["inv"]
    f = H.forward(z, labels, ix, iw, kind, margin, scale, K, topk, pen, eps)
    valid = f["valid"]
    nv = max(int(valid.sum()), 1)
    gl = np.full(B, 1.0 / nv)
    g = H.backward(z, labels, ix, iw, kind, margin, scale, K, topk, pen, eps, f["lse"], f["hard"], gl)
    Awk = np.abs(ix)[:, None] * np.abs(iw)[None, :]
    ck = (z * ix[:, None]) * iw[None, :]
    dcosk = 4.01 * U * np.abs(ck) + 1.01 * Awk * ez
    rows = np.arange(B)[:, None]
    cols = np.arange(N)[None, :] * K + f["kstar"]                 # (B, N): the selected centre of every class
    dcos, Aw = dcosk[rows, cols], Awk[rows, cols]
    # the selections are beyond the reach of the errors
    lo, hi = (ck - dcosk).reshape(B, N, K), (ck + dcosk).reshape(B, N, K)
    for k in range(K):
        rival = np.where(f["kstar"] == k, -np.inf, hi[:, :, k])
        assert (lo[rows, np.arange(N)[None, :], f["kstar"]] > rival).all(), "centres of a class too close for this test"
    for b in np.flatnonzero(valid):
        members = [j for j in f["hard"][b] if j >= 0]
        rest = [j for j in range(N) if j not in members and j != labels[b]]
        if members and rest:
            assert (f["c"][b, members] - dcos[b, members]).min() > (f["c"][b, rest] + dcos[b, rest]).max(), "top-k boundary too close"
    cm, sm = math.cos(margin), math.sin(margin)
    P1 = cm + sm * cmax / math.sqrt(1 - cmax * cmax) if kind == "aam" else 1.0
    P2 = sm / (1 - cmax * cmax) ** 1.5 if kind == "aam" else 0.0
    assert cmax < cm
    hot, slope, p = np.zeros((B, N)), np.ones((B, N)), np.zeros((B, N))
    for b in np.flatnonzero(valid):
        y = int(labels[b])
        assert kind != "aam" or abs(f["c"][b, y]) <= cmax - 1e-3, (b, f["c"][b, y])
        hot[b, y], slope[b, y] = 1.0, R.psi(f["c"][b, y], kind, margin)[1]
        p[b] = np.exp(f["l"][b] - f["lse"][b])
    d = (scale * P1 * dcos).max(axis=1)
    eta = np.expm1(2 * d)[:, None]
    loss = f["loss"].sum() / nv
    kernel = 2.02 * U * (np.abs(f["lse"]) + (1 - eps) * np.abs(f["ly"]) + eps * np.abs(f["lmean"]))
    loss_bound = float((((2 + 2 * eps) * d + kernel) * valid).sum() / nv + (B + 2) * U * 1.01 * abs(loss))
    gs = (gl * scale)[:, None] * valid[:, None]
    dc = gs * ((p - hot) + eps * (hot - 1.0 / N)) * slope
    dcos_y = (dcos * hot).sum(axis=1)[:, None]
    Edc_c = gs * (p * eta * np.where(hot > 0, P1, 1.0) + hot * (p + 1) * (1 + eta) * P2 * dcos_y)
    Edc, dcf = np.zeros((B, NK)), np.zeros((B, NK))
    Edc[rows, cols], dcf[rows, cols] = Edc_c, dc
    Edz = 1.01 * Awk * Edc + 4.01 * U * np.abs(g["dz"]) + 2.02 * U * g["dz_mag"] + TINY
    gz, Eg = g["dz"], Edz
    if mode == "bf16":
        gz = bf16_rne(g["dz"].astype(np.float32)).astype(np.float64)
        Eg = Edz + 2.0 ** -7 * (np.abs(g["dz"]) + Edz)
    gabs = np.abs(gz) + Eg
    dxg, dwg = gz @ wq, gz.T @ xq
    Edxg = acc(NK) * (gabs @ np.abs(wq)) + Eg @ np.abs(wq)
    Edwg = acc(B) * (gabs.T @ np.abs(xq)) + Eg.T @ np.abs(xq)
    moved = Edc * (np.abs(z) + ez) + np.abs(dcf) * ez
    Edix = 1.01 * (moved @ np.abs(iw)) + 3.1 * U * g["dinv_x_abs"]
    Ediw = 1.01 * (moved.T @ np.abs(ix)) + 3.1 * U * g["dinv_w_abs"]
    dxn, dwn = R.inv_norm_backward(x64, EPS, ix, g["dinv_x"]), R.inv_norm_backward(w64, EPS, iw, g["dinv_w"])
    Edxn = 1.02 * (np.abs(ix) ** 3 * Edix)[:, None] * np.abs(x64) + 8.1 * U * np.abs(dxn) + TINY
    Edwn = 1.02 * (np.abs(iw) ** 3 * Ediw)[:, None] * np.abs(w64) + 8.1 * U * np.abs(dwn) + TINY
    return dict(loss=loss, loss_bound=loss_bound, pred=f["pred"], sub_y=f["sub_y"], c=f["c"], dx=dxg + dxn, dw=dwg + dwn,
                dx_bound=Edxg + Edxn + 1.01 * U * (np.abs(dxg) + np.abs(dxn)), dw_bound=Edwg + Edwn + 1.01 * U * (np.abs(dwg) + np.abs(dwn)))


def head_problem(kind):
    """19 rows, 64 dimensions, 40 classes of 2 centres: weights and embeddings from the host, so the restatement's assertions about
    the data (head_reference) do not depend on the device."""
    B, D, N, K = 19, 64, 40, 2
    rng = np.random.default_rng(21)
    x = rng.standard_normal((B, D)).astype(np.float32)
    w = (rng.standard_normal((N * K, D)) * D ** -0.5).astype(np.float32)
    return x, w, _labels(B, N, rng), N, K


@pytest.mark.parametrize("kind", ["aam", "am", "softmax"])
@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16x3"])
def test_classifier_head_against_the_restatement(mode, kind):
    x, w, labels, N, K = head_problem(kind)
    B, D = x.shape
    head = A.ClassifierHead(D, N, kind=kind, gemm=mode, normalize=True, device=DEV, sub_centers=K, top_k=5, penalty=0.06, label_smoothing=0.1)
    with torch.no_grad():
        head.weight.copy_(_dev(w))
    ref = head_reference(x, w, labels, kind, head.margin, head.scale, mode, K, 5, 0.06, 0.1)
    emb = _dev(x).requires_grad_(True)
    loss, pred = head.train()(emb, _dev(labels))
    loss.backward()
    ratios = {"loss": abs(loss.item() - ref["loss"]) / ref["loss_bound"],
              "demb": float((np.abs(emb.grad.cpu().numpy() - ref["dx"]) / ref["dx_bound"]).max()),
              "dweight": float((np.abs(head.weight.grad.cpu().numpy() - ref["dw"]) / ref["dw_bound"]).max())}
    print(f"ClassifierHead {kind} gemm={mode} K={K}: loss {loss.item():.6f}, worst |err| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios
    top = np.sort(ref["c"], axis=1)
    sure = top[:, -1] - top[:, -2] > 1e-3                         # far beyond what the GEMM's error moves a cosine by
    assert np.array_equal(pred.cpu().numpy()[sure], ref["pred"][sure])
    counts = np.zeros((N, K), np.int64)
    for b in np.flatnonzero(ref["sub_y"] >= 0):
        counts[labels[b], ref["sub_y"][b]] += 1
    assert np.array_equal(head.center_counts.cpu().numpy(), counts)
    with torch.no_grad():
        cos = head.cosines(emb)
    assert cos.shape == (B, N) and float(cos.abs().max()) <= 1.0 + 1e-5
    assert float((cos.cpu().double() - torch.as_tensor(ref["c"])).abs().max()) <= 1e-4      # the classes' cosines: the largest centre's
    assert np.array_equal(cos.argmax(1).cpu().numpy()[sure], ref["pred"][sure])


def test_center_counts_and_dominant():
    """center_counts after a few steps is the host's count of the sub_y the kernels returned; evaluation mode does not count;
    dominant() keeps each class's most counted centre, the lowest among equal counts."""
    B, D, N, K = 19, 16, 6, 3
    rng = np.random.default_rng(31)
    torch.manual_seed(31)
    head = A.ClassifierHead(D, N, kind="am", sub_centers=K, label_smoothing=0.1, device=DEV).train()
    seen = []
    real = ops.head_forward

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append((a[2].cpu().numpy().copy(), out[4].cpu().numpy().copy()))       # labels (int32), sub_y
        return out
    ops.head_forward = spy
    try:
        for step in range(4):
            labels = rng.integers(-1, N + 1, B)
            head(_dev(rng.standard_normal((B, D)).astype(np.float32)), _dev(labels))
        counted = head.center_counts.cpu().numpy().copy()
        head.eval()(_dev(rng.standard_normal((B, D)).astype(np.float32)), _dev(rng.integers(0, N, B)))
    finally:
        ops.head_forward = real
    assert len(seen) == 5 and np.array_equal(head.center_counts.cpu().numpy(), counted)
    want = np.zeros((N, K), np.int64)
    for labels, sub_y in seen[:4]:
        assert ((sub_y >= 0) == ((labels >= 0) & (labels < N))).all() and (sub_y < K).all()
        for y, k in zip(labels, sub_y):
            if k >= 0:
                want[y, k] += 1
    assert np.array_equal(counted, want) and want.sum() > 0
    with torch.no_grad():
        head.center_counts[0] = 0                                 # a class no row selected: centre 0
        head.center_counts[1] = torch.tensor([2, 5, 5], device=DEV)
    counts = head.center_counts.cpu().numpy()
    best = [int(np.flatnonzero(r == r.max())[0]) for r in counts]
    assert best[0] == 0 and best[1] == 1
    small = head.dominant()
    assert small.sub_centers == 1 and small.center_counts is None and small.weight.is_cuda and small.label_smoothing == 0.1
    wk = head.weight.detach().cpu().numpy().reshape(N, K, D)
    assert np.array_equal(_bits(small.weight.detach().cpu().numpy()), _bits(np.stack([wk[j, best[j]] for j in range(N)])))
    loss, pred = small(_dev(rng.standard_normal((B, D)).astype(np.float32)), _dev(rng.integers(0, N, B)))
    assert np.isfinite(loss.item()) and pred.shape == (B,)


def test_training_the_network_with_a_sub_centre_aam_head():
    """The five-GEMM network of test_gpu_loss.py under an AAM head of 8 classes x 2 centres with the penalty and smoothing on:
    30 SGD steps lower the loss."""
    seq = T._stack()
    feats, labels = T._problem()
    torch.manual_seed(5)
    net = A.TrainableSequential(seq, fused_norm=True).train()
    head = A.ClassifierHead(T.UNITS, 8, kind="aam", margin=0.2, scale=16.0, device=DEV, sub_centers=2, top_k=3, penalty=0.06,
                            label_smoothing=0.1).train()
    tf_, tl, ty = torch.as_tensor(feats, device=DEV), torch.as_tensor(T.NET_LENS, device=DEV), torch.as_tensor(labels, device=DEV)
    opt = torch.optim.SGD(list(net.parameters()) + list(head.parameters()), lr=0.05)
    losses = []
    for _ in range(31):
        opt.zero_grad()
        step_loss, pred = head(net(tf_, tl), ty)
        step_loss.backward()
        opt.step()
        losses.append(step_loss.item())
    print(f"sub-centre AAM: loss first {losses[0]:.4f}, after 30 steps {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    assert int(head.center_counts.sum()) == 31 * len(labels) and not head.center_counts[4:].any()
