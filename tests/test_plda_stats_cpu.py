"""The builders and oracles of tests/_plda_stats_ref.py, without a GPU: the mirrored constants are the source's, the case lists
reach every tile count, chunk count and edge that tests/test_gpu_plda_stats_dims.py claims, the integer cases are exact (the
np.longdouble oracle and the fp64 one give identical arrays), the fp64 oracle of the real-valued cases stays within a tenth of the
derived bound of the np.longdouble one, and the oracle's models at D = 65 / 150 / 200 move by less than a tenth of each tolerance
when the same rows come in another order."""

import os
import re

import numpy as np
import pytest

import _plda_stats_ref as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
wide = pytest.mark.skipif(np.finfo(LD).nmant <= 52, reason="np.longdouble is no wider than fp64 on this platform")


def source_constant(path, name):
    text = open(os.path.join(ROOT, path)).read()
    found = re.findall(r"(?:constexpr\s+int\s+|#define\s+)" + name + r"\s*=?\s*(\d+)", text)
    assert len(found) == 1, (path, name, found)
    return int(found[0])


def test_mirrored_constants_are_the_sources():
    hip = "kaldi-tflite_amd/csrc/plda_train.hip"
    for name in ("TILE", "KSTEP", "GRAM_MIN_ROWS", "GRAM_MAX_BLOCKS", "COLSUM_ROWS"):
        assert getattr(PS, name) == source_constant(hip, name), name
    assert PS.TRAIN_MAX_DIM == source_constant("include/ktf_hip.h", "KTF_TRAIN_MAX_DIM") == 1024
    text = open(os.path.join(ROOT, hip)).read()
    assert text.count("const int d = blockIdx.x * 256 + threadIdx.x;") == 2 and PS.COLSUM_COLS == 256
    assert "(rows + chunks - 1) / chunks" in text and "GRAM_MAX_BLOCKS / gram_tiles(D)" in text


def test_tile_map_walks_the_upper_triangle_row_by_row():
    for nt in (1, 2, 3, 4, 5, 16):
        got = [PS.tile_of(t, nt) for t in range(nt * (nt + 1) // 2)]
        assert got == [(i, j) for i in range(nt) for j in range(i, nt)]
    assert PS.gram_tiles(1024) == 136 and PS.gram_cap(1024) == 7 and PS.gram_cap(512) == 28 and PS.gram_cap(64) == 1024


def test_case_lists_reach_every_tile_count_chunk_count_and_edge():
    dims = PS.GRAM_DIMS + [PS.CAP_D]
    assert {PS.gram_tiles_1d(D) for D in dims} >= {1, 2, 3, 4, 5, 16}
    assert {D % PS.TILE for D in PS.GRAM_DIMS} >= {0, 1, 63} and any(D % PS.KSTEP for D in PS.GRAM_DIMS)
    assert {150, 200} <= set(PS.GRAM_DIMS) and max(dims) == PS.TRAIN_MAX_DIM
    assert {D % PS.TILE for D in PS.EM_DIMS} >= {0, 1, 63} and {D % PS.KSTEP for D in PS.EM_DIMS} >= {0, 1, 15}
    assert {S % PS.TILE for S in PS.EM_S} >= {0, 1, 63} and max(PS.EM_S) > 2 * PS.TILE
    # chunk counts 1, 2, 3, 4 by the row count and the capped value
    by_rows = {rows: PS.chunk_ranges(rows, PS.ROWS_D) for rows in PS.GRAM_ROWS}
    assert {len(c) for c in by_rows.values()} == {1, 2, 3, 4}
    assert [len(by_rows[r]) for r in (511, 512, 513, 1024, 1025, 1537)] == [1, 1, 2, 2, 3, 4]
    assert {r - PS.KSTEP for r in PS.GRAM_ROWS} >= {-1, 0, 1} and {r - PS.GRAM_MIN_ROWS for r in PS.GRAM_ROWS} >= {-1, 0, 1}
    for rows in PS.CAP_ROWS:
        wanted = -(-rows // PS.GRAM_MIN_ROWS)
        got = PS.chunk_ranges(rows, PS.CAP_D)
        assert wanted > len(got) == PS.gram_cap(PS.CAP_D) == 7
    assert PS.chunk_ranges(3585, 1024)[0] == (0, 513) and PS.chunk_ranges(3585, 1024)[-1] == (3078, 3585)
    every = list(by_rows.values()) + [PS.chunk_ranges(r, PS.CAP_D) for r in PS.CAP_ROWS] + [PS.chunk_ranges(PS.REAL_N, 200)]
    for ranges in every:                                     # the chunks tile the list, none is empty
        assert ranges[0][0] == 0 and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and all(r1 > r0 for r0, r1 in ranges)
    lens = [[r1 - r0 for r0, r1 in ranges] for ranges in every]
    assert any(n[0] % PS.KSTEP for n in lens if len(n) > 1)                      # a chunk whose row count is no multiple of 16
    assert any(n[-1] < n[0] for n in lens if len(n) > 1)                         # a last chunk shorter than the others
    assert any(n[-1] == n[0] for n in lens if len(n) > 1)                        # ... and one as long
    assert by_rows[1537] == [(0, 385), (385, 770), (770, 1155), (1155, 1537)]
    # the column-sum and class-mean kernels: D and the row count on both sides of 256
    assert {D - PS.COLSUM_COLS for D in PS.MEAN_DIMS} >= {-1, 0, 1} and {r - PS.COLSUM_ROWS for r in PS.MEAN_ROWS} >= {-1, 0, 1}
    assert max(PS.MEAN_DIMS) == max(PS.CLASS_DIMS) == PS.TRAIN_MAX_DIM and {1, 255, 256, 257} <= set(PS.CLASS_DIMS)
    assert {1, 2, 3, 7, 300} == set(PS.CLASS_COUNTS)
    # the workspace the host asks for is the larger of the two uses
    assert PS.workspace_bytes(4097, 1024) == 8 * 7 * 136 * 4096 and PS.workspace_bytes(513, 1) == 8 * 2 * 4096
    assert PS.workspace_bytes(2 ** 20 + 1, 1024) == 8 * 4097 * 1024          # beyond the cap the column sums need more


def test_the_library_sizes_its_workspace_by_the_restated_split():
    # a host function: the chunk cap and the chunk count by rows as the library computes them, without a GPU
    from kaldi_tflite_amd import ops
    cases = [(rows, PS.ROWS_D) for rows in PS.GRAM_ROWS] + [(rows, PS.CAP_D) for rows in PS.CAP_ROWS + [2 ** 20 + 1]]
    cases += [(PS.GRAM_DIM_LIST, D) for D in PS.GRAM_DIMS] + [(rows, D) for rows in PS.MEAN_ROWS for D in PS.MEAN_DIMS]
    for rows, D in cases + [(28 * 512 + 1, 512), (10 ** 6, 64), (10 ** 6, 65)]:
        assert ops._size("ktf_train_workspace_bytes", rows, D) == PS.workspace_bytes(rows, D), (rows, D)


@pytest.mark.parametrize("D", PS.ONE_ROW_DIMS)
def test_one_row_case_tells_the_two_halves_of_a_diagonal_tile_apart(D):
    for f64 in (False, True):
        y, c, w, want, differ = PS.one_row_case(D, f64)
        z = y[0].astype(np.float64) - c
        assert np.array_equal(want, want.T) and np.array_equal(np.triu(want), np.triu(np.outer(w[0] * z, z)))
        assert differ > 100                                  # pairs of one diagonal tile whose two orders round differently
        if np.finfo(LD).nmant > 52:                          # each element: within two roundings of the exact product
            exact = np.outer(w.astype(LD)[0] * z.astype(LD), z.astype(LD))
            assert np.all(np.abs(want - exact) <= 2.0 ** -51 * np.abs(exact))


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, LD), np.asarray(b, LD))


@wide
@pytest.mark.parametrize("D", PS.GRAM_DIMS)
def test_integer_gram_cases_over_d_are_exact(D):
    case = PS.gram_dim_case(D)                               # (asserts its exactness precondition)
    for form in PS.GRAM_FORMS:
        want = case["want"][form]
        args = PS.form_args(case, form)
        assert same(want, PS.gram(case["y"], dtype=LD, **args)) and np.array_equal(want, want.T)
        assert want[D - 1, D - 1] > 0 and np.array_equal(want * 2, np.round(want * 2))
    wants = [case["want"][f] for f in PS.GRAM_FORMS]
    assert all(not np.array_equal(a, b) for i, a in enumerate(wants) for b in wants[i + 1:])      # the forms differ


@wide
@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("rows", PS.GRAM_ROWS)
def test_integer_gram_cases_over_rows_are_exact(rows, with_idx):
    case = PS.gram_rows_case(rows, with_idx)
    y = case["y"][:case["N"]]
    assert same(case["want"], PS.gram(y, case["idx"], case["center"], case["weights"], dtype=LD))
    assert (case["idx"] is None) == (not with_idx) and (not with_idx or case["N"] < rows or rows == 1)
    assert not case["y"][case["N"]].any() and (case["idx"] is None or case["idx"].max() < case["N"])
    for k, (r0, r1) in enumerate(case["chunks"]):
        yk, ik = PS.only_chunk(case, k)
        alone = PS.gram(yk if ik is not None else yk[:rows], ik, None, case["weights"], dtype=LD)
        assert same(case["want_chunk"][k], alone)
        # a chunk left out or added twice changes G: no chunk's Gram vanishes
        assert case["want_chunk"][k][0, 0] > 0


@wide
@pytest.mark.parametrize("rows", PS.CAP_ROWS)
def test_integer_gram_cases_at_the_cap_are_exact(rows):
    case = PS.gram_cap_case(rows)
    y, c, w, want = case["y"], case["center"], case["weights"], case["want"]
    assert y.shape == (rows, PS.TRAIN_MAX_DIM) and np.array_equal(want, want.T)
    # np.longdouble on the columns at the tile edges (the whole matrix would take minutes); every element in another row order
    z = y.astype(LD) - c.astype(LD)
    probe = (w.astype(LD)[:, None] * z).T @ z[:, PS.CAP_PROBE]
    assert same(want[:, PS.CAP_PROBE], probe)
    order = np.random.default_rng(0).permutation(rows)
    assert np.array_equal(want, PS.gram(y[order], None, c, w[order]))


@wide
def test_integer_mean_and_projection_cases_are_exact():
    for rows in PS.MEAN_ROWS:
        for D in PS.MEAN_DIMS:
            y, want = PS.mean_case(rows, D)
            assert np.array_equal(y.astype(LD).sum(0), y.astype(np.float64).sum(0)) and want.shape == (D,)
            assert np.array_equal(want, y.astype(np.float64)[::-1].sum(0) * (1.0 / rows)) and y[rows - 1].all()
    for D in PS.CLASS_DIMS:
        x, offsets, utts, means, counts = PS.class_case(D)
        sums = np.stack([x[utts[offsets[s]:offsets[s + 1]]].astype(LD).sum(0) for s in range(len(counts))])
        assert counts.tolist() == PS.CLASS_COUNTS and np.array_equal(means, sums.astype(np.float64) / counts[:, None])
        assert utts.min() >= 0 and utts.max() < x.shape[0]
    for S in PS.EM_S:
        for D in PS.EM_DIMS:
            c = PS.em_case(S, D)
            y = (c["mu"].astype(LD) - c["mbar"].astype(LD)) @ c["P"].astype(LD).T
            assert np.array_equal(y, np.round(y)) and np.abs(y).max() < 2.0 ** 53
            nl = c["counts"][:, None] * c["lam"][None, :]
            assert np.array_equal(c["a"], (nl / (1 + nl)) * y.astype(np.float64)) and np.array_equal(c["b"], y.astype(np.float64) / (1 + nl))
            assert c["counts"].min() >= 1 and c["counts"].max() == PS.MAX_COUNT and (S == 1 or c["counts"].min() == 1)
            assert set(c["lam"].tolist()) <= set(PS.LAMBDAS.tolist()) and c["P"][:, D - 1].all()


@wide
@pytest.mark.parametrize("D", PS.REAL_DIMS)
def test_fp64_oracle_of_the_real_cases_is_within_a_tenth_of_the_bound(D):
    for f64 in (False, True):
        case = PS.real_gram_case(D, f64)
        assert case["y"].dtype == (np.float64 if f64 else np.float32) and 2.0 < np.linalg.norm(case["center"]) / np.sqrt(D) < 4.0
        for form in PS.REAL_FORMS:
            print(f"\ngram D={D} f64={f64} {form}: fp64 oracle - longdouble = {case['gap'][form]:.3f} of the bound")
            assert case["gap"][form] <= 0.1 and case["bound"][form].min() > 0
    em = PS.real_em_case(D)
    print(f"\nem D={D}: fp64 oracle - longdouble = {em['gap']:.3f} of the bound")
    assert em["gap"] <= 0.1


@pytest.mark.parametrize("D", PS.MODEL_DIMS)
def test_oracle_models_move_by_less_than_a_tenth_of_each_tolerance_under_a_permutation(D):
    a, b = PS.model_ref(D), PS.model_ref(D, permuted=True)
    (mean, T, psi), (mean2, T2, psi2) = a["plda"], b["plda"]
    e_mean = np.abs(mean - mean2).max() / np.abs(mean).max()
    e_psi = float((np.abs(psi - psi2) / psi).max())
    e_row = PS.row_err(T2, T)
    (enroll, test), n = PS.heldout(D)
    s, s2 = PS.plda_scores(a["plda"], enroll, test, n), PS.plda_scores(b["plda"], enroll, test, n)
    e_score = np.abs(s - s2).max() / np.abs(s).max()
    e_lda = max(PS.row_err(b["lda"][k], a["lda"][k]) for k in PS.MODEL_LDA)
    e_pca = max(PS.row_err(b["pca"][k], a["pca"][k]) for k in PS.MODEL_PCA)
    print(f"\nmodels D={D} under a permutation: mean {e_mean:.2e} psi {e_psi:.2e} rows {e_row:.2e} scores {e_score:.2e} "
          f"lda {e_lda:.2e} pca {e_pca:.2e}")
    assert e_mean <= 0.1 * PS.MEAN and e_psi <= 0.1 * PS.PSI and e_row <= 0.1 * PS.ROW_F64 and e_score <= 0.1 * PS.SCORE
    assert e_lda <= 0.1 * PS.ROW_F32 and e_pca <= 0.1 * PS.ROW_F32
    assert psi.min() > 0 and np.all(np.diff(psi) <= 0)
