"""The PLDA training statistics kernels (csrc/plda_train.hip) on the MI355X, called directly, at every tile, chunk and dimension
edge, against the fp64 oracle of tests/_plda_stats_ref.py. The integer cases must EQUAL the oracle (no tolerance: every partial sum
is exact in any order); the real-valued ones stay within a bound derived from the operation count, and repeat bit for bit. Every
call runs on a workspace filled with 0xFF bytes and writes into a buffer filled with NaN that is longer than the output: a tile or
chunk read before it is written, an element never written and a write beyond the output all show up. The estimators built on the
kernels are then compared with tests/_plda_train_ref.py at the dimensions recipes use (65, 150, 200) under the tolerances of
tests/test_gpu_plda_train.py. The measured worst cases are printed (run with -s) and recorded in DESIGN.md."""

import numpy as np
import pytest
import torch

import _plda_stats_ref as PS
from kaldi_tflite_amd import _lib as L
from kaldi_tflite_amd import ops
from kaldi_tflite_amd import training as tr

pytestmark = pytest.mark.gpu

PAD = PS.TILE * PS.TILE            # elements behind every output that must keep their poison
COUNT_POISON = -12345
F64 = {False: np.float32, True: np.float64}


def dev(a):
    return None if a is None else torch.as_tensor(np.array(a), device="cuda")     # a copy: the cached cases are read-only


def poisoned(n, dtype=torch.float64):
    return torch.full((n + PAD,), COUNT_POISON if dtype == torch.int32 else float("nan"), dtype=dtype, device="cuda")


def untouched(flat, n):
    tail = flat[n:]
    return bool((tail == COUNT_POISON).all() if flat.dtype == torch.int32 else torch.isnan(tail).all())


def workspace(rows, D):
    ws = ops.train_workspace(rows, D, "cuda")
    assert ws.numel() == PS.workspace_bytes(rows, D)
    return ws.fill_(0xFF)


def gram_t(y, idx=None, center=None, weights=None):
    """ktf_train_gram_f32 / _f64 on host arrays -> G (D, D) on the device, bit-symmetric, nothing written behind it."""
    y, idx, center, weights = dev(y), dev(idx), dev(center), dev(weights)
    N, D = y.shape
    rows = idx.numel() if idx is not None else N
    assert idx is None or (0 <= int(idx.min()) and int(idx.max()) < N)
    ws, flat = workspace(rows, D), poisoned(D * D)
    ops._call(ops._typed("ktf_train_gram", y), y.device, L.ptr(y), N, D, L.ptr(idx), rows, L.ptr(center), L.ptr(weights), L.ptr(flat),
              L.ptr(ws), ws.numel())
    G = flat[:D * D].view(D, D)
    assert untouched(flat, D * D)
    assert torch.equal(G, G.T)                               # (a NaN left over is unequal to itself)
    return G


def gram(y, **args):
    return gram_t(y, **args).cpu().numpy()


def colmean(y):
    y = dev(y)
    rows, D = y.shape
    ws, flat = workspace(rows, D), poisoned(D)
    ops._call(ops._typed("ktf_train_mean", y), y.device, L.ptr(y), rows, D, L.ptr(flat), L.ptr(ws), ws.numel())
    assert untouched(flat, D)
    return flat[:D].cpu().numpy()


def class_means(x, offsets, utts):
    x, offsets, utts = dev(x), dev(offsets), dev(utts)
    (N, D), S = x.shape, offsets.numel() - 1
    means, counts = poisoned(S * D), poisoned(S, torch.int32)
    ops._call("ktf_train_class_means", x.device, L.ptr(x), N, D, L.ptr(offsets), S, L.ptr(utts), utts.numel(), L.ptr(means), L.ptr(counts))
    assert untouched(means, S * D) and untouched(counts, S)
    return means[:S * D].view(S, D).cpu().numpy(), counts[:S].cpu().numpy()


def em_project_t(c):
    """-> (a, b) (S, D) on the device: the heads of buffers one tile of speakers and one tile of columns larger."""
    S, D = c["mu"].shape
    mu, mbar, P, lam, counts = (dev(c[k]) for k in ("mu", "mbar", "P", "lam", "counts"))
    a, b = (poisoned((S + PS.TILE) * (D + PS.TILE) - PAD) for _ in range(2))
    ops._call("ktf_plda_em_project", mu.device, L.ptr(mu), S, D, L.ptr(mbar), L.ptr(P), L.ptr(lam), L.ptr(counts), L.ptr(a), L.ptr(b))
    # with the row stride D a column d >= D of row s is column d - D of row s + 1: a write there lands in the next row (the
    # equality sees it) or, from the last row, behind the output, as a write to a row s >= S does
    assert untouched(a, S * D) and untouched(b, S * D)
    return a[:S * D].view(S, D), b[:S * D].view(S, D)


def as_input(y, f64):
    return np.asarray(y, F64[f64])


# ----------------------------------------------------------------------------- Gram: D against the tile
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("D", PS.GRAM_DIMS)
def test_gram_equals_the_oracle_at_every_d_edge(D, f64):
    case = PS.gram_dim_case(D)
    y = as_input(case["y"], f64)
    for form in PS.GRAM_FORMS:
        got = gram(y, **PS.form_args(case, form))
        assert np.array_equal(got, case["want"][form]), (form, np.argwhere(got != case["want"][form])[:4])


# ----------------------------------------------------------------------------- Gram: rows against the chunk split
@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("rows", PS.GRAM_ROWS)
def test_gram_equals_the_oracle_at_every_row_and_chunk_edge(rows, with_idx):
    case = PS.gram_rows_case(rows, with_idx)
    y = case["y"] if with_idx else case["y"][:rows]
    for f64 in (False, True):
        got = gram(as_input(y, f64), idx=case["idx"], center=case["center"], weights=case["weights"])
        assert np.array_equal(got, case["want"]), (f64, np.argwhere(got != case["want"])[:4])
    if len(case["chunks"]) > 1:
        for k, want in enumerate(case["want_chunk"]):       # one chunk's rows among zero rows: that chunk's own Gram
            yk, ik = PS.only_chunk(case, k)
            got = gram(yk if with_idx else yk[:rows], idx=ik, weights=case["weights"])
            assert np.array_equal(got, want), (k, case["chunks"][k])


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("D", PS.ONE_ROW_DIMS)
def test_gram_takes_both_halves_of_a_diagonal_tile_from_the_pair_with_i_below_j(D, f64):
    y, c, w, want, _ = PS.one_row_case(D, f64)
    got = gram(y, center=c, weights=w)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


# ----------------------------------------------------------------------------- Gram: the cap on chunks, the largest D
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("rows", PS.CAP_ROWS)
def test_gram_equals_the_oracle_at_the_chunk_cap_and_the_largest_d(rows, f64):
    case = PS.gram_cap_case(rows)
    got = gram(as_input(case["y"], f64), center=case["center"], weights=case["weights"])
    assert np.array_equal(got, case["want"]), np.argwhere(got != case["want"])[:4]


# ----------------------------------------------------------------------------- column means, class means
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("D", PS.MEAN_DIMS)
def test_column_means_equal_the_oracle(D, f64):
    for rows in PS.MEAN_ROWS:
        y, want = PS.mean_case(rows, D)
        got = colmean(as_input(y, f64))
        assert np.array_equal(got, want), (rows, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("D", PS.CLASS_DIMS)
def test_class_means_equal_the_oracle_on_a_slice_of_a_longer_list(D):
    x, offsets, utts, want, want_counts = PS.class_case(D)
    got, counts = class_means(x, offsets, utts)
    assert np.array_equal(counts, want_counts) and counts.dtype == np.int32
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


# ----------------------------------------------------------------------------- EM projection
@pytest.mark.parametrize("D", PS.EM_DIMS)
def test_em_projection_equals_the_oracle_and_stays_inside_s_and_d(D):
    for S in PS.EM_S:
        c = PS.em_case(S, D)
        a, b = (t.cpu().numpy() for t in em_project_t(c))
        assert np.array_equal(a, c["a"]), (S, np.argwhere(a != c["a"])[:4])
        assert np.array_equal(b, c["b"]), (S, np.argwhere(b != c["b"])[:4])


# ----------------------------------------------------------------------------- the wrappers hand the same arguments on
def test_the_ops_wrappers_give_the_same_bits():
    case = PS.gram_dim_case(150)
    y = dev(case["y"])
    args = {k: dev(v) for k, v in PS.form_args(case, "all").items()}
    ws = workspace(PS.GRAM_DIM_LIST, 150)
    assert np.array_equal(ops.train_gram(y, ws, **args).cpu().numpy(), case["want"]["all"])
    assert np.array_equal(ops.train_gram(y.double(), ws.fill_(0xFF), **args).cpu().numpy(), case["want"]["all"])
    rows_y, want = PS.mean_case(257, 257)
    assert np.array_equal(ops.train_mean(dev(rows_y), workspace(257, 257)).cpu().numpy(), want)
    x, offsets, utts, means, counts = PS.class_case(257)
    got, n = ops.train_class_means(dev(x), dev(offsets), dev(utts), len(counts))
    assert np.array_equal(got.cpu().numpy(), means) and np.array_equal(n.cpu().numpy(), counts)
    c = PS.em_case(65, 150)
    a, b = ops.plda_em_project(*(dev(c[k]) for k in ("mu", "mbar", "P", "lam", "counts")))
    assert np.array_equal(a.cpu().numpy(), c["a"]) and np.array_equal(b.cpu().numpy(), c["b"])


# ----------------------------------------------------------------------------- real-valued rows: the derived bounds
@pytest.mark.parametrize("D", PS.REAL_DIMS)
def test_real_valued_gram_and_projection_stay_within_the_derived_bounds(D):
    LD = np.longdouble
    for f64 in (False, True):
        case = PS.real_gram_case(D, f64)
        for form in PS.REAL_FORMS:
            args = PS.real_form_args(case, form)
            G, again = gram_t(case["y"], **args), gram_t(case["y"], **args)
            assert torch.equal(G, again)
            ratio = float((np.abs(G.cpu().numpy().astype(LD) - case["ref"][form]) / case["bound"][form]).max())
            print(f"\ngram D={D} {'f64' if f64 else 'f32'} {form}: worst err / bound {ratio:.4f}")
            assert ratio <= 1.0, (f64, form, ratio)
    c = PS.real_em_case(D)
    got, again = em_project_t(c), em_project_t(c)
    for name, g, g2, ref, bound in zip("ab", got, again, c["ref"], c["bound"]):
        assert torch.equal(g, g2)
        ratio = float((np.abs(g.cpu().numpy().astype(LD) - ref) / bound).max())
        print(f"\nem D={D} {name}: worst err / bound {ratio:.4f}")
        assert ratio <= 1.0, (name, ratio)


# ----------------------------------------------------------------------------- the estimators at the dimensions recipes use
@pytest.mark.parametrize("D", PS.MODEL_DIMS)
def test_compute_plda_matches_the_oracle_off_the_tile_edges(D):
    x, spk, *_ = PS.model_data(D)
    got = tr.compute_plda(dev(x), spk)
    mean, T, psi = PS.model_ref(D)["plda"]
    assert got.transformMat.dtype == np.float64 and got.transformMat.shape == (D, D)
    e_mean = np.abs(got.mean - mean).max() / np.abs(mean).max()
    e_psi = float((np.abs(got.psi - psi) / psi).max())
    e_row = PS.row_err(got.transformMat, T)
    (enroll, test), n = PS.heldout(D)
    s_ref = PS.plda_scores((mean, T, psi), enroll, test, n)
    e_score = np.abs(PS.plda_scores((got.mean, got.transformMat, got.psi), enroll, test, n) - s_ref).max() / np.abs(s_ref).max()
    print(f"\nplda D={D}: mean {e_mean:.2e} psi {e_psi:.2e} rows {e_row:.2e} scores {e_score:.2e}")
    assert e_mean <= PS.MEAN and e_psi <= PS.PSI and e_row <= PS.ROW_F64 and e_score <= PS.SCORE, (e_mean, e_psi, e_row, e_score)
    assert np.all(np.diff(got.psi) <= 0) and np.all(got.psi >= 0)


@pytest.mark.parametrize("D", PS.MODEL_DIMS)
def test_compute_lda_and_est_pca_match_the_oracle_off_the_tile_edges(D):
    x, spk, *_ = PS.model_data(D)
    xd, ref = dev(x), PS.model_ref(D)
    for f, quarter in PS.MODEL_LDA:
        dim = PS.lda_dim(D, quarter)
        got = tr.compute_lda(xd, spk, dim, total_covariance_factor=f)
        assert got.dtype == np.float32 and got.shape == (dim, D + 1)
        e = PS.row_err(got, ref["lda"][(f, quarter)])
        print(f"\nlda D={D} f={f} dim={dim}: rows {e:.2e}")
        assert e <= PS.ROW_F32, (f, dim, e)
    for half, m, v in PS.MODEL_PCA:
        want = ref["pca"][(half, m, v)]
        got = tr.est_pca(xd, PS.pca_dim(D, half), normalize_mean=m, normalize_variance=v)
        assert got.dtype == np.float32 and got.shape == want.shape
        e = PS.row_err(got, want)
        print(f"\npca D={D} mean={m} var={v} dim={want.shape[0]}: rows {e:.2e}")
        assert e <= PS.ROW_F32, (half, m, v, e)
