"""Score normalisation against a cohort on the MI355X: the top-N selection (ktf_topn_stats_*) on crafted rows against the NumPy
restatement (tests/_snorm_ref.py), its independence of where a row sits and of the run, PLDA.cohort_stats bit for bit against
ops.topn_stats of PLDA.score's block, against the fp64 restatement, its chunking, verification.score_normalized end to end, and
the refusals."""

import numpy as np
import pytest
import torch

import _snorm_ref as S
import _verif_ref as V
import test_gpu_verification as TV
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import ops

pytestmark = pytest.mark.gpu
Ls = ktf.layers
ver = ktf.verification
host, model, speakers, tol = TV.host, TV.model, TV.speakers, TV.tol
OFFSET = 1e8
KINDS = 8


def same_bits(a, b):
    return all(torch.equal(p.view(torch.int64), q.view(torch.int64)) for p, q in zip(a, b))


# ----------------------------------------------------------------------------- 1. selection on crafted matrices
def crafted(C, npdt, rows=65, seed=0):
    """(rows, C) in npdt, row r of kind r % KINDS, and the offset each row's deviation is measured from."""
    rng = np.random.default_rng(seed + C)
    x = np.empty((rows, C), npdt)
    off = np.zeros(rows)
    bits = np.uint64 if npdt == np.float64 else np.uint32
    for r in range(rows):
        kind = r % KINDS
        if kind == 0:                                              # random normals
            v = rng.standard_normal(C) * 10.0
        elif kind == 1:                                            # all equal
            v = np.full(C, [2.5, -7.25, 0.1][(r // KINDS) % 3])
        elif kind == 2:                                            # 40 % of the row is one value in the middle of the ranking
            v = np.where(rng.uniform(size=C) < 0.5, rng.uniform(1.0, 2.0, C), rng.uniform(-2.0, 0.0, C))
            v[rng.permutation(C)[:max(1, (4 * C) // 10)]] = 0.5
        elif kind == 3:                                            # 40 % of the row is its largest value: a small N cuts through it
            v = rng.uniform(-3.0, 3.0, C)
            v[rng.permutation(C)[:max(1, (4 * C) // 10)]] = 3.0
        elif kind == 4:                                            # mixed signs, many +0.0 and -0.0
            v = rng.standard_normal(C)
            z = rng.uniform(size=C)
            v[z < 0.3] = 0.0
            v[z < 0.15] = -0.0
        elif kind == 5:                                            # values that differ in the lowest mantissa byte only
            base = np.array([1.0 if (r // KINDS) % 2 == 0 else -1.0], npdt).view(bits)[0]
            v = (base + rng.integers(0, 256, C).astype(bits)).view(npdt)
        elif kind == 6:                                            # a common offset far above the spread: the centred variance
            v = OFFSET + rng.standard_normal(C)
            off[r] = OFFSET
        else:                                                      # wide dynamic range, both signs: every radix byte takes part
            v = rng.standard_normal(C) * np.exp(rng.uniform(-30.0, 30.0, C))
        x[r] = np.asarray(v, npdt)
    return x, off


def top_ns(C):
    return sorted(n for n in {1, 2, 7, C - 1, C, C + 5} if n >= 1 and (n <= C or n == C + 5))


def check_stats(got, x, off, n, what):
    """|mean - ref| <= 1e-12 max|row|, |std - ref| <= 1e-12 max|row - offset|; all-equal rows have std exactly 0."""
    x64 = np.asarray(x, np.float64)
    wm, ws = S.topn_stats(x64, n)
    gm, gs = host(got[0]), host(got[1])
    assert gm.shape == wm.shape and gs.shape == ws.shape
    em = np.abs(gm - wm) / np.maximum(np.abs(x64).max(axis=1), np.finfo(np.float64).tiny)
    es = np.abs(gs - ws) / np.maximum(np.abs(x64 - off[:x64.shape[0], None]).max(axis=1), np.finfo(np.float64).tiny)
    assert em.max() <= 1e-12, (what, n, int(em.argmax()), em.max())
    assert es.max() <= 1e-12, (what, n, int(es.argmax()), es.max())
    equal = np.all(x64 == x64[:, :1], axis=1)
    assert np.all(gs[equal] == 0.0) and np.all(gm[equal] == x64[equal, 0]), (what, n)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 5000])
def test_topn_stats_on_crafted_rows(C, dtype):
    npdt = np.float64 if dtype == torch.float64 else np.float32
    x, off = crafted(C, npdt)
    d = torch.as_tensor(x, device="cuda")
    for R in (1, 3, 65):
        for n in top_ns(C):
            got = ops.topn_stats(d[:R], n)
            assert got[0].dtype == torch.float64 and got[1].dtype == torch.float64 and got[0].shape == (R,)
            check_stats(got, x[:R], off, n, (C, R))
    check_stats(ops.topn_stats(d, None), x, off, None, (C, "None"))
    # rows inside a wider matrix (ld > C), read in place
    wide = torch.full((65, C + 11), 1e30, dtype=dtype, device="cuda")
    wide[:, 3:3 + C] = d
    for n in (top_ns(C)[0], top_ns(C)[-2]):
        got = ops.topn_stats(wide[:, 3:3 + C], n)
        check_stats(got, x, off, n, (C, "ld"))
        assert same_bits(got, ops.topn_stats(d, n))


def test_topn_stats_rows_starting_at_the_first_kinds_only():
    """R = 3 above takes kinds 0..2 only: every kind also as a matrix of its own single row (R = 1), in fp64 at the longest row that
    is staged in LDS (32 KiB) and the shortest that is read from global memory in every pass."""
    for C in (1000, 4096, 4097):
        x, off = crafted(C, np.float64, rows=KINDS, seed=5)
        d = torch.as_tensor(x, device="cuda")
        for r in range(KINDS):
            for n in (1, 7, C // 2, C - 1):
                check_stats(ops.topn_stats(d[r:r + 1], n), x[r:r + 1], off[r:r + 1], n, (C, "kind", r))


# ----------------------------------------------------------------------------- 2. independence and determinism
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("C", [257, 5000, 8192, 8193])            # rows staged in LDS (up to 32 KiB), and rows re-read from global memory
def test_row_result_independent_of_placement_and_run(C, dtype):
    rng = np.random.default_rng(C)
    row = torch.as_tensor(rng.standard_normal(C) * 3.0, device="cuda").to(dtype)
    row[::7] = row[3]                                              # ties
    for n in (2, 20, C - 1, None):
        alone = ops.topn_stats(row.reshape(1, C), n)
        assert same_bits(alone, ops.topn_stats(row.reshape(1, C), n))
        for R, at, ld in ((3, 2, C), (65, 40, C + 13), (65, 0, C + 1)):
            m = torch.as_tensor(rng.standard_normal((R, ld)), device="cuda").to(dtype)
            m[at, :C] = row
            got = ops.topn_stats(m[:, :C], n)
            assert same_bits((got[0][at:at + 1], got[1][at:at + 1]), alone), (n, R, at, ld)
            again = ops.topn_stats(m[:, :C], n)
            assert same_bits(got, again)


# ----------------------------------------------------------------------------- 3. / 4. the scores that are ranked
_setups = {}


def plda_setup(D, dtype):
    """A PLDA of dimension D, 70 transformed vectors and a cohort of 300 (its first 90 serve as the small cohort), and counts."""
    key = (D, dtype)
    if key not in _setups:
        mean, T, psi = model(D, seed=D + 1)
        layer = Ls.PLDA(D, mean, T, psi, dtype=dtype)
        rng = np.random.default_rng(D)
        v_tr = layer.transform(speakers(70, 1, D, seed=11))
        c_tr = layer.transform(speakers(300, 1, D, seed=12))
        _setups[key] = (layer, psi, v_tr, c_tr, rng.integers(1, 51, 70).astype(np.float64), rng.integers(1, 51, 300).astype(np.float64))
    return _setups[key]


def block(layer, v_tr, c_tr, role, n):
    """(R, C): row r holds the scores cohort_stats ranks for vector r, from PLDA.score."""
    if role == "test":
        return layer.score(v_tr, c_tr, enroll_num_examples=n)
    return layer.score(c_tr, v_tr, enroll_num_examples=n).t().contiguous()


@pytest.mark.parametrize("role", ["test", "enroll"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D", [128, 200])
def test_cohort_stats_rank_the_bits_of_plda_score(D, dtype, role):
    layer, psi, v_tr, c_all, n_v, n_c = plda_setup(D, dtype)
    for Cn in (90, 300):
        c_tr = c_all[:Cn]
        for counted in (True, False):
            n = None if not counted else (n_c[:Cn] if role == "test" else n_v)
            blk = block(layer, v_tr, c_tr, role, n)
            assert blk.shape == (70, Cn)
            for top_n in (2, 20, None):
                got = layer.cohort_stats(v_tr, c_tr, top_n=top_n, role=role, num_examples=n)
                assert got[0].shape == (70,) and got[0].dtype == torch.float64 and got[0].is_cuda
                assert same_bits(got, ops.topn_stats(blk, top_n)), (Cn, counted, top_n)


@pytest.mark.parametrize("role", ["test", "enroll"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("D", [128, 200])
def test_cohort_stats_match_restatement(D, dtype, role):
    """top_n = None only: with N < C a score that moves across the threshold within its tolerance changes the selected set."""
    layer, psi, v_tr, c_all, n_v, n_c = plda_setup(D, dtype)
    for Cn in (90, 300):
        c_tr = c_all[:Cn]
        for counted in (True, False):
            n = None if not counted else (n_c[:Cn] if role == "test" else n_v)
            one = 1.0 if n is None else n
            want = V.llr(host(v_tr), host(c_tr), psi, one) if role == "test" else V.llr(host(c_tr), host(v_tr), psi, one).T
            wm, ws = S.topn_stats(want, None)
            gm, gs = layer.cohort_stats(v_tr, c_tr, role=role, num_examples=n)
            bound = tol(dtype) * np.abs(want).max()
            assert np.abs(host(gm) - wm).max() <= bound and np.abs(host(gs) - ws).max() <= bound, (Cn, counted)


# ----------------------------------------------------------------------------- 5. chunking
@pytest.mark.parametrize("role", ["test", "enroll"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_cohort_stats_chunking_is_bit_identical(dtype, role):
    layer, psi, v_tr, c_all, n_v, n_c = plda_setup(128, dtype)
    c_tr = c_all[:90]
    row = 90 * v_tr.element_size()
    for n in (None, n_c[:90] if role == "test" else n_v):
        for top_n in (20, None):
            whole = layer.cohort_stats(v_tr, c_tr, top_n=top_n, role=role, num_examples=n)
            for limit in (25 * row + 7, 69 * row, row - 1, 1):     # chunks of 25, 25 and 20 rows; of 64 and 6 (whole tiles); of one row
                got = layer.cohort_stats(v_tr, c_tr, top_n=top_n, role=role, num_examples=n, workspace_limit=limit)
                assert same_bits(got, whole), (top_n, limit)


# ----------------------------------------------------------------------------- 6. end to end
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_score_normalized_end_to_end(dtype):
    D = 128
    mean, T, psi = model(D, seed=77)
    plda = Ls.PLDA(D, mean, T, psi, dtype=dtype)
    rng = np.random.default_rng(8)
    n_e = rng.integers(1, 9, 20).astype(np.float64)
    n_c = rng.integers(1, 30, 90).astype(np.float64)
    e_tr = plda.transform(speakers(20, 1, D, seed=21), num_examples=n_e)
    t_tr = plda.transform(speakers(40, 1, D, seed=22))
    cohort = torch.as_tensor(speakers(90, 1, D, seed=23), device="cuda")
    je = rng.integers(0, 12, 200)                                  # models repeat; models 12..19 occur in no trial
    it = rng.choice(np.arange(0, 40, 3), 200)                      # tests 1, 2, 4, 5, ... occur in no trial
    raw_want = plda.score_trials(t_tr, e_tr, je, it, enroll_num_examples=n_e)
    coh_plain, coh_n = plda.transform(cohort), plda.transform(cohort, num_examples=n_c)
    # the restatement on the device's own transformed vectors (their rounding is test_gpu_verification's subject)
    s_e = V.llr(host(coh_plain), host(e_tr), psi, n_e).T           # (models, cohort)
    s_t = V.llr(host(t_tr), host(coh_n), psi, n_c)                 # (tests, cohort)
    s_raw = V.llr(host(t_tr), host(e_tr), psi, n_e)[it, je]
    eps = tol(dtype) * max(np.abs(s_e).max(), np.abs(s_t).max(), np.abs(s_raw).max())     # the bound on a score, a mean and a std
    for sides in ("both", "enroll", "test"):
        es = S.topn_stats(s_e, None) if sides != "test" else None
        ts = S.topn_stats(s_t, None) if sides != "enroll" else None
        want = S.as_norm(s_raw, je, it, es, ts)
        for trials in ((je, it), (torch.as_tensor(je, device="cuda"), torch.as_tensor(it, device="cuda"))):
            got, raw = ver.score_normalized(plda, e_tr, t_tr, trials, cohort, enroll_num_examples=n_e, cohort_num_examples=n_c, sides=sides)
            assert got.shape == (200,) and got.dtype == torch.float64 and torch.equal(raw, raw_want)
            # z = (s - mu) / sd with s, mu and sd each within eps: |dz| <= (2 eps + |z| eps) / sd to first order; twice that covers
            # the higher orders (eps / sd << 1) and the arithmetic of the normalisation itself
            sd_min = min(p[1].min() for p in (es, ts) if p is not None)
            bound = 2.0 * eps * (2.0 + np.abs(want).max()) / sd_min
            assert np.abs(host(got) - want).max() <= bound, (sides, np.abs(host(got) - want).max(), bound)
    # adaptive: the statistics of every model / test (a row's bits do not depend on its neighbours) through the loop
    for top_n in (20, None):
        es = tuple(host(a) for a in plda.cohort_stats(e_tr, coh_plain, top_n=top_n, role="enroll", num_examples=n_e))
        ts = tuple(host(a) for a in plda.cohort_stats(t_tr, coh_n, top_n=top_n, role="test", num_examples=n_c))
        want = S.as_norm(host(raw_want), je, it, es, ts)
        got, raw = ver.score_normalized(plda, e_tr, t_tr, (je, it), cohort, top_n=top_n, enroll_num_examples=n_e, cohort_num_examples=n_c)
        assert torch.equal(raw, raw_want)
        assert np.abs(host(got) - want).max() <= 8 * np.finfo(np.float64).eps * np.abs(want).max()
        small = ver.score_normalized(plda, e_tr, t_tr, (je, it), cohort, top_n=top_n, enroll_num_examples=n_e, cohort_num_examples=n_c,
                                     workspace_limit=4096)[0]
        assert torch.equal(small, got)


def test_verification_score_with_and_without_cohort():
    ext, _ = TV.extractor("f32")
    mean, T, psi = model(128, seed=40)
    plda = Ls.PLDA(128, mean, T, psi)
    enroll = torch.as_tensor(TV.wavs(), device="cuda")
    test = torch.as_tensor(TV.synth.make_wav(3, 48000, seed=9), device="cuda")
    spk2utt = [[0, 1], [2], [3, 1, 0]]
    trials = (np.array([0, 1, 2, 0, 2]), np.array([0, 1, 2, 2, 0]))
    means, nu = ver.speaker_means(ext.embeddings(enroll), spk2utt)
    e_tr = plda.transform(ext.postprocess(means), num_examples=nu)
    y_tr = plda.transform(ext(test))
    today = plda.score_trials(y_tr, e_tr, trials[0], trials[1], enroll_num_examples=nu)
    assert torch.equal(ver.score(ext, plda, enroll, spk2utt, test, trials), today)
    cohort = torch.as_tensor(speakers(30, 1, 128, seed=3), device="cuda").to(torch.float32)
    n_c = np.arange(1, 31, dtype=np.float64)
    got = ver.score(ext, plda, enroll, spk2utt, test, trials, cohort=cohort, top_n=10, cohort_num_examples=n_c)
    want, raw = ver.score_normalized(plda, e_tr, y_tr, trials, cohort, top_n=10, enroll_num_examples=nu, cohort_num_examples=n_c)
    assert got.dtype == torch.float64 and torch.equal(got, want) and torch.equal(raw, today)


# ----------------------------------------------------------------------------- 7. refusals
def test_refusals():
    layer, psi, v_tr, c_all, n_v, n_c = plda_setup(128, torch.float64)
    c_tr = c_all[:90]
    for bad in (1, 0, -3, 2.0, True):
        with pytest.raises(ValueError):
            layer.cohort_stats(v_tr, c_tr, top_n=bad)
    with pytest.raises(ValueError):
        layer.cohort_stats(v_tr, c_tr[:, :100])                    # a cohort of the wrong dim
    with pytest.raises(ValueError):
        layer.cohort_stats(v_tr[:, :100], c_tr)
    with pytest.raises(ValueError):
        layer.cohort_stats(v_tr, c_tr.cpu())                       # cohort and vectors on different devices
    with pytest.raises(ValueError):
        layer.cohort_stats(v_tr.cpu(), c_tr)
    with pytest.raises(ValueError):
        layer.cohort_stats(v_tr[0], c_tr)                          # rank
    with pytest.raises(ValueError):
        layer.cohort_stats(v_tr, c_tr[:0])
    with pytest.raises(ValueError):
        layer.cohort_stats(v_tr, c_tr, role="model")
    zero = n_c[:90].copy()
    zero[4] = 0.0
    for bad in (zero, -1.0, n_c[:89], torch.as_tensor(zero, device="cuda")):
        with pytest.raises(ValueError):
            layer.cohort_stats(v_tr, c_tr, num_examples=bad)       # counts <= 0, or not one per cohort vector
    with pytest.raises(ValueError):
        layer.cohort_stats(v_tr, c_tr, role="enroll", num_examples=n_c[:90])      # the enroll side's counts belong to the rows
    with pytest.raises(ValueError):
        layer.cohort_stats(v_tr, c_tr, workspace_limit=0)
    x = torch.zeros((3, 5), dtype=torch.float64, device="cuda")
    for bad in (0, -1):
        with pytest.raises(ValueError):
            ops.topn_stats(x, bad)
    with pytest.raises(ValueError):
        ops.topn_stats(x.to(torch.float16), 2)
    e_tr = v_tr[:20]
    trials = (np.array([0, 1]), np.array([2, 3]))
    with pytest.raises(ValueError):
        ver.score_normalized(layer, e_tr, v_tr, trials, c_tr[:, :100])
    with pytest.raises(ValueError):
        ver.score_normalized(layer, e_tr, v_tr, trials, c_tr.cpu())
    with pytest.raises(ValueError):
        ver.score_normalized(layer, e_tr, v_tr, (np.array([0, 20]), np.array([2, 3])), c_tr)
    with pytest.raises(ValueError):
        ver.score_normalized(layer, e_tr, v_tr, trials, c_tr, top_n=1)
    # empty inputs launch nothing and return empty statistics
    m, s = layer.cohort_stats(v_tr[:0], c_tr, top_n=5)
    assert m.shape == (0,) and s.shape == (0,)
    m, s = ops.topn_stats(x[:0], 2)
    assert m.shape == (0,)
