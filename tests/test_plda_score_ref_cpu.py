"""The oracle and bounds of tests/_plda_score_ref.py, without a GPU: agreement with tests/_verif_ref.py where the two overlap, an
fp32 emulation of the score tile's arithmetic inside the score bound on every element of the inputs the GPU tests use, and
mutants of that emulation (a dropped dimension, counts taken as 1, counts or psi shifted by one) outside it by a factor of 10
or more: the evidence that tests/test_gpu_plda_score_edges.py would fail on a subtly wrong kernel."""

import numpy as np
import pytest

import _plda_score_ref as P
import _verif_ref as V

F32 = np.float32
SHAPES = ((1, 1), (1, 65), (65, 1), (63, 64), (64, 64), (64, 65), (65, 129), (129, 65), (128, 128))


# ----------------------------------------------------------------------------- the oracle against _verif_ref
@pytest.mark.parametrize("dim", [1, 17, 65, 257])
def test_llr_agrees_with_verif_ref(dim):
    y, e, psi, n = P.score_inputs(dim, 9, 11, np.float64)
    for cnt in (n, 1.0):
        want = V.llr(y, e, psi, cnt)
        S = P.llr_mags(y, e, psi, cnt)
        assert np.all(np.abs(P.llr(y, e, psi, cnt) - want) <= 1e-14 * S)
        wide = P.llr(y, e, psi, cnt, prec=np.longdouble)
        assert wide.dtype == np.longdouble and np.all(np.abs(wide - want) <= (dim + 12) * 2.0 ** -53 * S)
        assert np.all(S >= np.abs(want)) and S.shape == want.shape
    # the magnitudes, term by term, for one pair
    i, j = 4, 3
    k = n[j] * psi / (n[j] * psi + 1.0)
    var1 = 1.0 + psi / (n[j] * psi + 1.0)
    s = 0.5 * np.sum(np.abs(np.log(var1)) + (np.abs(y[i]) + np.abs(k * e[j])) ** 2 / var1 + np.log(1.0 + psi) + y[i] ** 2 / (1.0 + psi))
    assert P.llr_mags(y, e, psi, n)[i, j] == pytest.approx(s, rel=1e-13)


@pytest.mark.parametrize("dim", [1, 17, 65, 257])
@pytest.mark.parametrize("normalize,simple", [(False, False), (True, False), (True, True), (False, True)])
def test_transform_agrees_with_verif_ref(dim, normalize, simple):
    x, T, _, psi, n = P.transform_inputs(dim, 5, np.float64)
    mean = np.random.default_rng(dim).standard_normal(dim)
    offset = -T @ mean
    for cnt in (n, 1.0):
        want = V.transform(x, mean, T, psi, cnt, normalize, simple)
        got = P.transform(x, T, offset, psi, cnt, normalize, simple)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        # the affine form itself, exactly as V.transform evaluates it: a column of ones carries the offset
        aug = V.transform(np.c_[x, np.ones(len(x))], 0.0, np.c_[T, offset], psi, cnt, normalize, simple)
        assert np.abs(got - aug).max() <= 1e-13 * np.abs(want).max()
        b = P.transform_bound(x, T, offset, psi, cnt, normalize, simple, np.float32)
        assert b.shape == want.shape and np.all(b > 0)
    S, tot = P.transform_mags(x, T, offset, psi, n, simple)
    assert S[2, 0] == pytest.approx(np.sum(np.abs(T[0] * x[2])) + abs(offset[0]), rel=1e-13)
    y = x @ T.T + offset
    assert tot[2] == pytest.approx(np.sum(y[2] ** 2 / (1.0 if simple else psi + 1.0 / n[2])), rel=1e-12)


def test_input_rules():
    for dim in P.DIMS:
        for npdt in (np.float32, np.float64):
            y, e, psi, n = P.score_inputs(dim, 65, 67, npdt)
            assert psi.dtype == npdt and y.dtype == npdt and e.dtype == npdt
            assert dim < 8 or np.any(np.diff(psi) > 0) and np.any(np.diff(psi) < 0)            # not sorted
            edges = P.edge_dims(dim)
            assert dim - 1 in edges and all(0.5 <= psi[d] <= 30.0 for d in edges)
            if dim > 4:
                assert psi[1:4].tolist() == np.asarray(P.SPECIAL_PSI, npdt).tolist()
            else:
                assert psi.min() >= 0.05
            assert n[:3].tolist() == [1.0, 50.0, 2.0] and n.min() >= 1 and n.max() <= 50 and np.all(n == np.round(n))
            assert len(set(n[64:].tolist())) > 1 and n[64:67].tolist() != n[:3].tolist()    # the second tile's counts differ
    assert P.make_counts(1, np.random.default_rng(0)).tolist() == [1.0]


# ----------------------------------------------------------------------------- fp32 emulation of the tile, and its mutants
def emulate_terms(y, e, psi, n):
    """The per-dimension terms of plda_score_tile<float, PER_CLASS> in fp32, every operation rounded as the kernel rounds it
    (no fused multiply-add: one more rounding than the kernel may take)."""
    one = F32(1)
    y, e, psi = np.asarray(y, F32), np.asarray(e, F32), np.asarray(psi, F32)
    n = np.asarray(n, F32)[:, None]
    npsi = n * psi                                                  # (M, dim)
    ke = npsi * e / (npsi + one)
    w = one / (one + psi / (npsi + one))
    diff = y[:, None, :] - ke[None]
    q = diff * diff * w[None]                                       # (N, M, dim)
    l1 = np.log(one + psi / (npsi + one))                           # (M, dim)
    l2 = np.log(one + psi)                                          # (dim,)
    c = y * y * (one / (one + psi))                                 # (N, dim)
    for a in (q, l1, l2, c):
        assert a.dtype == F32
    return q, l1, l2, c


def emulate_score(terms, drop=None):
    q, l1, l2, c = terms
    if drop is not None:
        q, l1, l2, c = (np.delete(a, drop, axis=a.ndim - 1) for a in terms)
    half = F32(-0.5)
    s = half * (np.sum(l1, axis=1, dtype=F32)[None, :] + np.sum(q, axis=2, dtype=F32)) \
        - half * (np.sum(l2, dtype=F32) + np.sum(c, axis=1, dtype=F32))[:, None]
    assert s.dtype == F32
    return s


def oracle(y, e, psi, n, dim):
    return P.llr(y, e, psi, n), P.score_bound(P.llr_mags(y, e, psi, n), dim, F32)


def worst(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref) / bound).max())


@pytest.mark.parametrize("dim", P.DIMS)
def test_emulation_within_bound_and_mutants_outside(dim):
    y, e, psi, n = P.score_inputs(dim, 65, 67, F32)
    ref, bound = oracle(y, e, psi, n, dim)
    terms = emulate_terms(y, e, psi, n)
    r = worst(emulate_score(terms), ref, bound)
    ones = np.ones_like(n)
    ref1, bound1 = oracle(y, e, psi, ones, dim)
    r1 = worst(emulate_score(emulate_terms(y, e, psi, ones)), ref1, bound1)
    print(f"emulation dim={dim}: worst err / bound {r:.3f} with counts, {r1:.3f} without")
    assert r <= 1.0 and r1 <= 1.0
    mutants = {f"dropped d={d}": emulate_score(terms, drop=d) for d in P.edge_dims(dim)}
    mutants["counts all 1"] = emulate_score(emulate_terms(y, e, psi, ones))
    mutants["counts shifted by one class"] = emulate_score(emulate_terms(y, e, psi, np.roll(n, 1)))
    if dim > 1:
        mutants["psi shifted by one dimension"] = emulate_score(emulate_terms(y, e, np.roll(psi, 1), n))
    for name, got in mutants.items():
        m = worst(got, ref, bound)
        print(f"  mutant {name}: worst err / bound {m:.3g}")
        assert m >= 10.0, (dim, name, m)
    # the count-free form: a dropped dimension
    terms1 = emulate_terms(y, e, psi, ones)
    for d in P.edge_dims(dim):
        assert worst(emulate_score(terms1, drop=d), ref1, bound1) >= 10.0, (dim, d)


def emulate_transform(x, A, offset, psi, n, normalize, simple, drop=None):
    """plda_transform_row<float> in fp32; drop: a column of A the dot products leave out."""
    x, A, offset, psi = (np.asarray(a, F32) for a in (x, A, offset, psi))
    prod = A[None, :, :] * x[:, None, :]
    if drop is not None:
        prod = np.delete(prod, drop, axis=2)
    ys = np.sum(prod, axis=2, dtype=F32) + offset
    if not normalize:
        return ys
    dim = F32(x.shape[1])
    if simple:
        f = np.sqrt(dim) / np.sqrt(np.sum(ys * ys, axis=1, keepdims=True, dtype=F32))
    else:
        f = np.sqrt(dim / np.sum(ys * ys / (psi + F32(1) / np.asarray(n, F32)[:, None]), axis=1, keepdims=True, dtype=F32))
    assert f.dtype == F32
    return ys * f


@pytest.mark.parametrize("dim", P.DIMS)
def test_transform_emulation_within_bound_and_mutants_outside(dim):
    x, A, offset, psi, n = P.transform_inputs(dim, 5, F32)
    for normalize, simple in ((False, False), (True, False), (True, True)):
        ref = P.transform(x, A, offset, psi, n, normalize, simple)
        bound = P.transform_bound(x, A, offset, psi, n, normalize, simple, F32)
        r = worst(emulate_transform(x, A, offset, psi, n, normalize, simple), ref, bound)
        print(f"transform emulation dim={dim} normalize={normalize} simple={simple}: worst err / bound {r:.3f}")
        assert r <= 1.0
        for d in P.edge_dims(dim) if dim > 1 or not normalize else ():   # (dim 1: the length norm keeps the sign of y alone)
            assert worst(emulate_transform(x, A, offset, psi, n, normalize, simple, drop=d), ref, bound) >= 10.0, (dim, d)
        if normalize and not simple:
            assert worst(emulate_transform(x, A, offset, psi, np.ones_like(n), True, False), ref, bound) >= 10.0
            assert worst(emulate_transform(x, A, offset, psi, np.roll(n, 1), True, False), ref, bound) >= 10.0
            if dim > 1:
                assert worst(emulate_transform(x, A, offset, np.roll(psi, 1), n, True, False), ref, bound) >= 10.0


@pytest.mark.parametrize("dim", [17, 257])
@pytest.mark.parametrize("N,M", SHAPES)
def test_emulation_within_bound_at_every_shape(dim, N, M):
    y, e, psi, n = P.score_inputs(dim, N, M, F32)
    for cnt in (n, np.ones_like(n)):
        ref, bound = oracle(y, e, psi, cnt, dim)
        got = emulate_score(emulate_terms(y, e, psi, cnt))
        assert got.shape == (N, M) and worst(got, ref, bound) <= 1.0
