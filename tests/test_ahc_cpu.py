"""CPU half of agglomerative clustering (Kaldi agglomerative-cluster): the two NumPy restatements agree with each other, with
hand-worked cases and with SciPy's average linkage; the C-ABI and ktf.diarization.agglomerative_cluster reject bad arguments
before anything reaches a GPU."""

import ctypes as C

import numpy as np
import pytest
import torch

import _ahc_ref as A
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L


def random_case(rng, i):
    n = int(rng.integers(1, 301)) if i % 4 else int(rng.integers(1, 40))
    dt = np.float32 if i % 2 else np.float64
    if i % 3 == 0:                                          # ties: small-integer costs
        s = rng.integers(-4, 5, (n, n)).astype(dt)
    else:
        s = rng.standard_normal((n, n)).astype(dt)
    if i % 7 == 0 and n > 2:                                # NaN / +-inf in the upper triangle
        k = max(1, n // 10)
        s[rng.integers(0, n, k), rng.integers(0, n, k)] = rng.choice([np.nan, np.inf, -np.inf], k)
    if i % 5 == 0:                                          # the lower triangle and the diagonal are never read
        s[np.tril_indices(n)] = np.nan
    if i % 2 == 0:
        kw = {"num_speakers": int(rng.integers(1, 6))}
        if i % 4 == 0:
            kw["max_spk_fraction"] = float(rng.choice([0.25, 0.4, 0.5, 0.75]))
    else:
        thr = float(rng.choice([-1.0, -0.25, 0.0, 0.5, 1.0, 2.0]))
        if i % 3 == 0:
            thr = float(rng.integers(-2, 3))                # integer costs: avg == threshold happens
        kw = {"threshold": thr}
    return s, kw, bool(i % 11 == 0)


def test_restatements_agree_on_random_cases():
    rng = np.random.default_rng(2024)
    merged_sizes, fraction_blocked = 0, 0
    for i in range(200):
        s, kw, rc = random_case(rng, i)
        want = A.ahc_kaldi(s, read_costs=rc, **kw)
        got = A.ahc_fast(s, read_costs=rc, **kw)
        assert got[1] == want[1] and np.array_equal(got[0], want[0]), (i, s.shape, s.dtype, kw)
        assert want[0].dtype == np.int32 and set(want[0].tolist()) == set(range(1, want[1] + 1))
        merged_sizes += want[1] < s.shape[0]
        if "max_spk_fraction" in kw and want[1] > kw["num_speakers"]:
            fraction_blocked += 1
    assert merged_sizes > 100 and fraction_blocked > 5, (merged_sizes, fraction_blocked)


@pytest.mark.parametrize("fn", [A.ahc_kaldi, A.ahc_fast])
def test_hand_cases(fn):
    for dt in (np.float32, np.float64):
        assert fn(np.zeros((1, 1), dt))[0].tolist() == [1]
        s = np.random.default_rng(1).standard_normal((6, 6)).astype(dt)
        assert fn(s, num_speakers=6)[0].tolist() == [1, 2, 3, 4, 5, 6]
        assert fn(s, num_speakers=9)[1] == 6
        # avg == threshold merges (<=), just above does not
        c = np.array([[0, 0.25], [0, 0]], dt)
        assert fn(c, threshold=0.25, read_costs=True)[1] == 1
        assert fn(c, threshold=float(np.nextafter(dt(0.25), dt(0))), read_costs=True)[1] == 2
        # NaN is never merged, not even in num_speakers mode; neither is +inf there
        for bad in (np.nan, np.inf):
            c = np.array([[0, bad], [0, 0]], dt)
            assert fn(c, num_speakers=1, read_costs=True)[1] == 2
        # label order: clusters never merged come first, in row order, then merged ones in the order of their last merge
        c = np.full((3, 3), 9.0, dt)
        c[1, 2] = 0.0
        assert fn(c, threshold=1.0, read_costs=True)[0].tolist() == [1, 2, 2]     # ids 1, 4
        c = np.full((3, 3), 9.0, dt)
        c[0, 1] = 0.0
        assert fn(c, threshold=1.0, read_costs=True)[0].tolist() == [2, 2, 1]     # ids 3, 4


@pytest.mark.parametrize("fn", [A.ahc_kaldi, A.ahc_fast])
def test_four_point_merge_order(fn):
    # costs (read_costs=True): C(3,4) = 0.1 is merged first -> id 5 = {3, 4}; then C(1,2) = 0.3 -> id 6 = {1, 2};
    # Sigma(5, 6) = 0.9 * 4 = 3.6, avg 0.9 > 0.5: stop. Final ids 5, 6 -> rows 3, 4 get label 1 and rows 1, 2 label 2.
    c = np.full((4, 4), 0.9)
    c[0, 1], c[2, 3] = 0.3, 0.1
    assert fn(c, threshold=0.5, read_costs=True)[0].tolist() == [2, 2, 1, 1]
    # with threshold 1.0 the two merge as well (id 7): one cluster
    assert fn(c, threshold=1.0, read_costs=True)[0].tolist() == [1, 1, 1, 1]
    # as scores (read_costs=False, Kaldi's default) the block is negated: scores -c give the same merges
    assert fn(-c, threshold=0.5)[0].tolist() == [2, 2, 1, 1]
    assert fn(-c)[1] == 4
    # max_spk_fraction 0.5: clusters of at most ceil(4 * 0.5) = 2 rows, so num_speakers=1 stops at two
    assert fn(-c, num_speakers=1, max_spk_fraction=0.5)[0].tolist() == [2, 2, 1, 1]
    # ties: equal costs merge the pair with the smallest (lo_id, hi_id) first
    t = np.ones((4, 4))
    assert fn(t, num_speakers=3, read_costs=True)[0].tolist() == [3, 3, 1, 2]        # (1, 2) -> id 5


def test_restatement_matches_scipy_average_linkage():
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    rng = np.random.default_rng(7)
    for n in (2, 5, 30, 120):
        for thr in (0.3, 0.8, 1.3):
            x = rng.standard_normal((n, 3))
            d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))      # tie-free, non-negative
            iu = np.triu_indices(n, 1)
            got, k = A.ahc_fast(d, threshold=thr, read_costs=True)
            if n > 1:
                ref = hier.fcluster(hier.linkage(d[iu], method="average"), t=thr, criterion="distance")
            else:
                ref = np.ones(1, int)
            assert k == len(set(ref.tolist()))
            # the same partition up to relabelling
            pairs = {(int(a), int(b)) for a, b in zip(got, ref)}
            assert len(pairs) == k, (n, thr)


def test_ahc_abi_argument_validation_without_gpu():
    lib = L.load()
    buf = (C.c_double * 64)()
    fbuf = (C.c_float * 64)()
    ibuf = (C.c_int32 * 16)()
    lens = (C.c_int32 * 3)(2, 3, 1)
    need = lib.ktf_ahc_workspace_bytes(lens, 3, 8)
    assert need > 0 and lib.ktf_ahc_workspace_bytes(lens, 3, 4) <= need
    big = (C.c_int32 * 2)(400, 6000)
    assert lib.ktf_ahc_workspace_bytes(big, 2, 4) < lib.ktf_ahc_workspace_bytes(big, 2, 8)

    def call(fn=lib.ktf_ahc_f64, s=buf, lengths=lens, dev=True, R=3, frac=1.0, labels=True, counts=True, ws=True,
             ws_bytes=need):
        return fn(s, lengths, ibuf if dev else None, R, 0, 0.0, None, frac, ibuf if labels else None,
                  ibuf if counts else None, buf if ws else None, ws_bytes, None)

    for kw, msg in [({"s": None}, "null argument"), ({"dev": False}, "null argument"), ({"labels": False}, "null argument"),
                    ({"counts": False}, "null argument"), ({"ws": False}, "null argument"), ({"lengths": None}, "null lengths"),
                    ({"R": 0}, "R = 0"), ({"R": 70000}, "R = 70000"),
                    ({"lengths": (C.c_int32 * 3)(2, 0, 1)}, "lengths[1] = 0"),
                    ({"lengths": (C.c_int32 * 3)(2, 3, 32768)}, "lengths[2] = 32768"),
                    ({"frac": 0.0}, "outside (0, 1]"), ({"frac": 1.5}, "outside (0, 1]"), ({"frac": -0.5}, "outside (0, 1]"),
                    ({"frac": float("nan")}, "outside (0, 1]"), ({"ws_bytes": need - 1}, "workspace of"),
                    ({"fn": lib.ktf_ahc_f32, "s": fbuf, "lengths": (C.c_int32 * 3)(-1, 3, 1)}, "lengths[0] = -1")]:
        assert call(**kw) == -1, kw
        assert msg in L.last_error(), (kw, L.last_error())
    assert lib.ktf_ahc_workspace_bytes((C.c_int32 * 2)(4, 40000), 2, 8) == -1 and "lengths[1]" in L.last_error()
    assert lib.ktf_ahc_workspace_bytes(lens, 3, 2) == -1 and "dtype_bytes" in L.last_error()
    assert lib.ktf_ahc_workspace_bytes(None, 3, 8) == -1


def _z(n=4, dtype=torch.float32):
    return torch.zeros((n, n), dtype=dtype)


@pytest.mark.parametrize("scores,kwargs,match", [
    ([], {}, "non-empty"),
    (np.zeros((4, 4), np.float32), {}, "tensor"),
    ([np.zeros((4, 4), np.float32)], {}, "torch tensor"),
    (torch.zeros((4, 3)), {}, "square"),
    (torch.zeros((0, 0)), {}, "square"),
    (torch.zeros((2, 2, 2)), {}, "square"),
    (torch.zeros((4, 4), dtype=torch.float16), {}, "float32 or all float64"),
    ([_z(), _z(3, torch.float64)], {}, "float32 or all float64"),
    (torch.zeros((4, 4), dtype=torch.int32), {}, "float32 or all float64"),
    (_z(), {"threshold": 0.5, "num_speakers": 2}, "not both"),
    (_z(), {"max_spk_fraction": 0.5}, "num_speakers only"),
    (_z(), {"num_speakers": 2, "max_spk_fraction": 0.0}, r"\(0, 1\]"),
    (_z(), {"num_speakers": 2, "max_spk_fraction": 1.5}, r"\(0, 1\]"),
    (_z(), {"num_speakers": 2, "max_spk_fraction": float("nan")}, r"\(0, 1\]"),
    (_z(), {"num_speakers": 0}, ">= 1"),
    (_z(), {"num_speakers": -3}, ">= 1"),
    (_z(), {"num_speakers": True}, "int or 1 ints"),
    (_z(), {"num_speakers": 2.0}, "int or 1 ints"),
    ([_z(), _z()], {"num_speakers": [2]}, "int or 2 ints"),
    ([_z(), _z()], {"num_speakers": [2, 1.5]}, "int or 2 ints"),
    (_z(), {"threshold": float("nan")}, "number"),
    (_z(), {"threshold": "0.5"}, "number"),
    (_z(), {"read_costs": 1}, "bool"),
    (_z(), {}, "on one GPU"),                         # a CPU tensor: there is no CPU path
])
def test_agglomerative_cluster_rejects_bad_arguments(scores, kwargs, match):
    with pytest.raises(ValueError, match=match):
        ktf.diarization.agglomerative_cluster(scores, **kwargs)


def test_agglomerative_cluster_rejects_blocks_above_the_limit():
    big = torch.empty((L.AHC_MAX_N + 1, L.AHC_MAX_N + 1), dtype=torch.float32, device="meta")
    with pytest.raises(ValueError, match="at most 32767"):
        ktf.diarization.agglomerative_cluster(big)
