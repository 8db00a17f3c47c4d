"""The PLDA transform and scoring kernels on the MI355X at every dimension and tile edge (plda_common.h: plda_transform_row,
plda_score_tile in its four forms, wave_sum_as_256; pool_post.hip: ktf_plda_*, ktf_plda_score_*, ktf_plda_transform_n_*,
ktf_plda_score_n_*, ktf_plda_trials_*, ktf_spk_mean_f32; the cohort launcher of score_norm.hip), in both dtypes, against the
oracle of tests/_plda_score_ref.py.

Every element is compared, each with its own bound: |got - ref| <= (dim + k) u S for a score, S the magnitudes of its terms before
cancellation, and the transform's bound carried through the scale factor (the counts of k are in _plda_score_ref.py;
tests/test_plda_score_ref_cpu.py shows that a dropped dimension, a wrong count or a shifted psi breaks them by a factor of 10 or
more). The fp32 kernels are compared with the oracle in fp64, the fp64 kernels with the same expressions in long double. Where
two paths must agree, they agree bit for bit. Each test prints its worst err / bound before it asserts."""

import functools

import numpy as np
import pytest
import torch

import _plda_score_ref as P
import _verif_ref as V
from kaldi_tflite_amd import ops

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]
SHAPES = ((1, 1), (1, 65), (65, 1), (63, 64), (64, 64), (64, 65), (65, 129), (129, 65), (128, 128))


def npdt(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def prec(dtype):
    """The precision the reference is evaluated in: one the kernel's own roundings are large against."""
    return np.longdouble if dtype == torch.float64 else np.float64


def dev(a, dtype=None):
    t = torch.as_tensor(np.array(a, order="C"), device="cuda")      # (a copy: the shared references are read-only)
    return t if dtype is None else t.to(dtype)


def bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(dim, N, M, dtype):
    """Inputs of one scoring case and its references, computed once and shared: with the counts and with every count 1."""
    y, e, psi, n = P.score_inputs(dim, N, M, npdt(dtype))
    p = prec(dtype)
    ones = np.ones_like(n)
    host = frozen(y, e, psi, n, P.llr(y, e, psi, n, p), P.score_bound(P.llr_mags(y, e, psi, n, p), dim, npdt(dtype)),
                  P.llr(y, e, psi, ones, p), P.score_bound(P.llr_mags(y, e, psi, ones, p), dim, npdt(dtype)))
    return host + (dev(y), dev(e), dev(psi), dev(n, dtype))


def ratio(got, ref, bound):
    """Worst |got - ref| / bound over every element."""
    g = got.detach().cpu().numpy()
    assert g.shape == ref.shape and np.isfinite(g).all(), (g.shape, ref.shape)
    return float((np.abs(g.astype(ref.dtype) - ref) / bound).max())


def all_pairs(N, M, seed):
    """Every (class j, test i) pair once, shuffled."""
    j, i = np.meshgrid(np.arange(M, dtype=np.int32), np.arange(N, dtype=np.int32))
    pairs = np.stack([j.ravel(), i.ravel()], axis=1)
    return pairs[np.random.default_rng(seed).permutation(len(pairs))]


def check_three(dim, N, M, dtype, what):
    """ops.plda_score, ops.plda_score_n and ops.plda_trials (all N M pairs, shuffled) against the oracle; returns the blocks."""
    y, e, psi, n, ref_n, bound_n, ref_1, bound_1, dy, de, dpsi, dn = case(dim, N, M, dtype)
    s = ops.plda_score(dy, de, dpsi)
    sn = ops.plda_score_n(dy, de, dpsi, dn)
    pairs = all_pairs(N, M, dim + N)
    st = ops.plda_trials(dy, de, dpsi, dn, dev(pairs))
    r = ratio(s, ref_1, bound_1)
    rn = ratio(sn, ref_n, bound_n)
    rt = ratio(st, ref_n[pairs[:, 1], pairs[:, 0]], bound_n[pairs[:, 1], pairs[:, 0]])
    tag = "f64" if dtype == torch.float64 else "f32"
    print(f"plda edges {what} {tag} dim={dim} N={N} M={M}: worst err / bound plda_score {r:.4f}, plda_score_n {rn:.4f}, "
          f"plda_trials {rt:.4f}")
    assert r <= 1.0 and rn <= 1.0 and rt <= 1.0, (r, rn, rt)
    return s, sn


# ----------------------------------------------------------------------------- scores
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", P.DIMS)
def test_scores_at_every_dimension_edge(dtype, dim):
    N, M = 65, 67
    s, _ = check_three(dim, N, M, dtype, "dims")
    dy, de, dpsi = case(dim, N, M, dtype)[8:11]
    assert same_bits(ops.plda_score_n(dy, de, dpsi, torch.ones(M, dtype=dtype, device="cuda")), s)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,M", SHAPES)
@pytest.mark.parametrize("dim", [17, 257])
def test_scores_at_every_tile_shape(dtype, dim, N, M):
    s, sn = check_three(dim, N, M, dtype, "shapes")
    dy, de, dpsi, dn = case(dim, N, M, dtype)[8:]
    if N > 3 and M > 5:                                             # a sub-block scored on its own: the bits of that block
        assert same_bits(ops.plda_score(dy[3:], de[5:], dpsi), s[3:, 5:].contiguous())
        assert same_bits(ops.plda_score_n(dy[3:], de[5:], dpsi, dn[5:]), sn[3:, 5:].contiguous())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 15, 16, 17, 255, 256, 257])
@pytest.mark.parametrize("dim", [15, 17, 257])
def test_trial_lists(dtype, dim, T):
    N, M = 65, 67
    ref_n, bound_n = case(dim, N, M, dtype)[4:6]
    dy, de, dpsi, dn = case(dim, N, M, dtype)[8:]
    rng = np.random.default_rng([dim, T])
    pairs = np.stack([rng.integers(0, M, T), rng.integers(0, N, T)], axis=1).astype(np.int32)
    st = ops.plda_trials(dy, de, dpsi, dn, dev(pairs))
    r = ratio(st, ref_n[pairs[:, 1], pairs[:, 0]], bound_n[pairs[:, 1], pairs[:, 0]])
    print(f"plda edges trials {'f64' if dtype == torch.float64 else 'f32'} dim={dim} T={T}: worst err / bound plda_trials {r:.4f}")
    assert st.shape == (T,) and r <= 1.0
    perm = rng.permutation(T)
    assert same_bits(ops.plda_trials(dy, de, dpsi, dn, dev(pairs[perm])), st[dev(perm)])


# ----------------------------------------------------------------------------- transform
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("dim", P.DIMS)
def test_transform_at_every_dimension_edge(dtype, dim, B):
    x, A, offset, psi, n = P.transform_inputs(dim, B, npdt(dtype))
    dx, dA, doff, dpsi = dev(x), dev(A), dev(offset), dev(psi)
    p = prec(dtype)
    aug_x, aug_A = np.c_[x.astype(np.float64), np.ones(B)], np.c_[A.astype(np.float64), offset.astype(np.float64)]
    worst = {}
    for normalize in (False, True):
        for simple in (False, True):
            for cnt in (n, np.ones_like(n)):
                got = ops.plda_transform_n(dx, dA, doff, dpsi, dev(cnt, dtype), normalize, simple)
                ref = P.transform(x, A, offset, psi, cnt, normalize, simple, p)
                bound = P.transform_bound(x, A, offset, psi, cnt, normalize, simple, npdt(dtype), p)
                key = ("affine" if not normalize else "simple" if simple else "psi")
                worst[key] = max(worst.get(key, 0.0), ratio(got, ref, bound))
                if dtype == torch.float32:                          # and V.transform itself, a column of ones carrying the offset
                    v = V.transform(aug_x, 0.0, aug_A, psi, cnt, normalize, simple)
                    worst[key] = max(worst[key], ratio(got, v, bound))
    print(f"plda edges transform {'f64' if dtype == torch.float64 else 'f32'} dim={dim} B={B}: worst err / bound plda_transform_n "
          + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 63, 64, 65])
@pytest.mark.parametrize("dim", [15, 65, 257])
def test_plda_call_is_transform_then_score(dtype, dim, B):
    x, A, offset, psi, _ = P.transform_inputs(dim, B, npdt(dtype))
    dx, dA, doff, dpsi = dev(x), dev(A), dev(offset), dev(psi)
    ones = torch.ones(B, dtype=dtype, device="cuda")
    for simple in (False, True):
        scores, tr = ops.plda(dx, dA, doff, dpsi, True, simple)
        assert same_bits(tr, ops.plda_transform_n(dx, dA, doff, dpsi, ones, True, simple))
        assert scores.shape == (B, B) and same_bits(scores, ops.plda_score(tr, tr, dpsi))


# ----------------------------------------------------------------------------- cohort forms
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,C", [(1, 1), (1, 65), (65, 1), (64, 64), (65, 129)])
@pytest.mark.parametrize("dim", [17, 64, 257])
def test_cohort_forms_leave_the_score_block(dtype, dim, R, C):
    """Both roles (role 1 is the SWAP_STORE tile), with and without counts: the workspace's first R C elements are the (R, C)
    block of plda_score / plda_score_n, element by element, nothing is written past them or past the R statistics."""
    dy, de, dpsi, dn_c = case(dim, R, C, dtype)[8:]                 # rows, cohort, psi, counts of the cohort
    dn_r = dev(P.make_counts(R, np.random.default_rng([dim, R, C])), dtype)
    item = dy.element_size()
    need = ops.plda_cohort_workspace_bytes(R, C, dim, item)
    assert need == R * C * item
    for role in (0, 1):
        for counts in (None, dn_c if role == 0 else dn_r):
            if role == 0:
                want = ops.plda_score(dy, de, dpsi) if counts is None else ops.plda_score_n(dy, de, dpsi, counts)
            else:                                                   # the cohort scored as tests against the rows as classes
                want = (ops.plda_score(de, dy, dpsi) if counts is None else ops.plda_score_n(de, dy, dpsi, counts)).t().contiguous()
            for top_n in (None, 2):
                ws = torch.full((need + 256,), 0xFF, dtype=torch.uint8, device="cuda")
                mean = torch.full((R + 2,), float("nan"), dtype=torch.float64, device="cuda")
                std = torch.full((R + 2,), float("nan"), dtype=torch.float64, device="cuda")
                ops.plda_cohort_stats(dy, de, dpsi, counts, role, top_n, mean, std, ws)
                block = ws[:need].view(dtype).view(R, C)
                what = (role, counts is not None, top_n)
                assert same_bits(block, want), what
                assert bool((ws[need:] == 0xFF).all()), what
                wm, wsd = ops.topn_stats(block.clone(), top_n)
                assert same_bits(mean[:R], wm) and same_bits(std[:R], wsd), what
                assert bool(torch.isnan(mean[R:]).all()) and bool(torch.isnan(std[R:]).all()), what


# ----------------------------------------------------------------------------- speaker means
@pytest.mark.parametrize("D", [1, 255, 256, 257, 600])
def test_spk_mean_at_every_width(D):
    rng = np.random.default_rng(D)
    U = 45
    raw = (rng.standard_normal((U, D)) * 3).astype(np.float32)
    spk = [[3], [7, 7], rng.integers(0, U, 40).tolist(), [44, 0], [12, 3, 12, 12]]       # 1, 2 and 40 utterances, repeated indices
    assert len(set(spk[2])) < 40
    S = len(spk)
    want, wn = V.ivector_mean(raw, spk)
    offsets = dev(np.cumsum([0] + [len(u) for u in spk]).astype(np.int32))
    utts = dev(np.concatenate(spk).astype(np.int32))
    mbuf = torch.full((S * D + 7,), -7.5, dtype=torch.float32, device="cuda")
    nbuf = torch.full((S + 3,), -99, dtype=torch.int32, device="cuda")
    m, nu = ops.spk_mean(dev(raw), offsets, utts, S, means=mbuf[:S * D].view(S, D), num_utts=nbuf[:S])
    assert m.data_ptr() == mbuf.data_ptr() and nu.data_ptr() == nbuf.data_ptr()
    got = mbuf.cpu().numpy()
    assert np.array_equal(got[:S * D].view(np.int32), want.ravel().view(np.int32))
    assert np.all(got[S * D:] == -7.5)
    assert nbuf.cpu().numpy().tolist() == wn.tolist() + [-99] * 3
