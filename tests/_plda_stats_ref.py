"""Case builders and the fp64 oracle for the PLDA training statistics kernels (csrc/plda_train.hip: class_stats_kernel, the two
column-sum kernels, gram_kernel<float|double> / gram_reduce_kernel, em_project_kernel) along the axes that choose their code
path: D against the 64-wide tile and the 16-wide LDS round, the row count against the chunk split, the speaker count against the
64-row tile. The oracles are plain NumPy; the integer cases are built so that every product and every partial sum in any order
is exactly representable in fp64 (the builders assert it), so that a kernel's output must EQUAL the oracle's whatever its
summation order: what is left is one correctly rounded division and one multiplication, stated here as the kernel states them.
Every builder is cached and returns read-only arrays.

Internal constants of the kernels, mirrored here because the library does not export them (tests/test_plda_stats_cpu.py checks
them against the source; a changed constant moves the edge, not the correctness of a test)."""

import functools

import numpy as np

import _plda_train_ref as R
from kaldi_tflite_amd import _lib as L
from test_gpu_plda_train import MEAN, PSI, ROW_F32, ROW_F64, SCORE, geom, row_err, spd  # noqa: F401 (the tolerances: for the tests)

TILE = 64                          # plda_train.hip:17, output tile of gram_kernel / em_project_kernel
KSTEP = 16                         # plda_train.hip:18, rows (gram) / summed index (projection) per LDS round
GRAM_MIN_ROWS = 512                # plda_train.hip:19, a chunk holds at least this many rows ...
GRAM_MAX_BLOCKS = 1024             # plda_train.hip:20, ... and tiles x chunks stays below this
COLSUM_ROWS = 256                  # plda_train.hip:21, rows per chunk of colsum_partial_kernel
COLSUM_COLS = 256                  # plda_train.hip:84, columns per workgroup of the column-sum and class-mean kernels
TRAIN_MAX_DIM = L.TRAIN_MAX_DIM    # include/ktf_hip.h KTF_TRAIN_MAX_DIM

U64 = 2.0 ** -53                   # unit roundoff of fp64
WEIGHTS = np.array([0.0, 0.5, 1.0, 2.0, 3.0])
LAMBDAS = np.array([0.0, 0.25, 0.5, 1.0, 2.0, 3.0])
MAX_COUNT = 300


# ------------------------------------------------------------------ the work split, restated
def gram_tiles_1d(D):
    return (D + TILE - 1) // TILE


def gram_tiles(D):
    t = gram_tiles_1d(D)
    return t * (t + 1) // 2


def gram_cap(D):
    return max(1, GRAM_MAX_BLOCKS // gram_tiles(D))


def gram_chunks(rows, D):
    by_rows = (rows + GRAM_MIN_ROWS - 1) // GRAM_MIN_ROWS
    return max(1, min(by_rows, gram_cap(D)))


def chunk_ranges(rows, D):
    """[(r0, r1)] of gram_kernel's chunks: per = ceil(rows / chunks) list positions each, the last one what is left."""
    chunks = gram_chunks(rows, D)
    per = (rows + chunks - 1) // chunks
    return [(c * per, min(c * per + per, rows)) for c in range(chunks)]


def tile_of(t, nt):
    """Upper-triangle tile t -> (ti, tj), ti <= tj, row by row: the kernel's loop."""
    ti = 0
    while t >= nt - ti:
        t -= nt - ti
        ti += 1
    return ti, ti + t


def workspace_bytes(rows, D):
    """ktf_train_workspace_bytes."""
    gram = gram_chunks(rows, D) * gram_tiles(D) * TILE * TILE
    cols = (rows + COLSUM_ROWS - 1) // COLSUM_ROWS * D
    return 8 * max(gram, cols)


# ------------------------------------------------------------------ the oracles
def gram(y, idx=None, center=None, weights=None, dtype=np.float64):
    """G = sum_r w_r (y[idx[r]] - c)(y[idx[r]] - c)^T, summed in `dtype`."""
    z = np.asarray(y).astype(dtype)
    if idx is not None:
        z = z[np.asarray(idx)]
    if center is not None:
        z = z - np.asarray(center).astype(dtype)
    wz = z if weights is None else np.asarray(weights).astype(dtype)[:, None] * z
    return wz.T @ z


def gram_magnitude(y, idx=None, center=None, weights=None):
    """sum_r |w_r| |y_ri - c_i| |y_rj - c_j| (fp64)."""
    z = np.asarray(y, np.float64)
    if idx is not None:
        z = z[np.asarray(idx)]
    if center is not None:
        z = z - np.asarray(center, np.float64)
    z = np.abs(z)
    wz = z if weights is None else np.abs(np.asarray(weights, np.float64))[:, None] * z
    return wz.T @ z


def colmean(y, dtype=np.float64):
    """sum * (1.0 / rows), the kernel's expression; the sum in `dtype`, the product in fp64 unless dtype is wider."""
    s = np.asarray(y).astype(dtype).sum(0)
    return _narrow(s, dtype) * (_one(dtype) / _narrow(np.asarray(y.shape[0]), dtype))


def class_means(x, offsets, utts, dtype=np.float64):
    """-> (means (S, D) = sum / count, counts (S,) int32) of the speakers of the CSR map; the sums in `dtype`, list order."""
    S = len(offsets) - 1
    x = np.asarray(x).astype(dtype)
    sums = np.stack([x[utts[offsets[s]:offsets[s + 1]]].sum(0) for s in range(S)])
    counts = np.diff(np.asarray(offsets)).astype(np.int32)
    return _narrow(sums, dtype) / _narrow(counts, dtype)[:, None], counts


def em_project(mu, mbar, P, lam, counts, dtype=np.float64):
    """y = (mu - mbar) P^T in `dtype`; a = (nl / den) * y, b = y / den with nl = n lam, den = 1 + nl, as the kernel states them."""
    y = (np.asarray(mu).astype(dtype) - np.asarray(mbar).astype(dtype)) @ np.asarray(P).astype(dtype).T
    y = _narrow(y, dtype)
    nl = _narrow(np.asarray(counts), dtype)[:, None] * _narrow(np.asarray(lam), dtype)[None, :]
    den = _one(dtype) + nl
    return (nl / den) * y, y / den


def em_magnitude(mu, mbar, P):
    """sum_k |mu_sk - mbar_k| |P_dk| (fp64)."""
    return np.abs(np.asarray(mu, np.float64) - np.asarray(mbar, np.float64)) @ np.abs(np.asarray(P, np.float64)).T


def _wide(dtype):
    return np.dtype(dtype).itemsize > 8


def _narrow(a, dtype):
    """The rounded steps run in fp64 (the integer cases: the sums are exact, so the cast is) unless a wider reference is asked for."""
    return np.asarray(a).astype(dtype if _wide(dtype) else np.float64)


def _one(dtype):
    return (np.dtype(dtype).type if _wide(dtype) else np.float64)(1.0)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def ints(rng, shape, dtype=np.float32, lim=4):
    return rng.integers(-lim, lim + 1, shape).astype(dtype)


def scrambled_idx(rng, N, rows):
    """`rows` list positions over [0, N): every row at least once while rows >= N, repeats, in scrambled order."""
    base = np.arange(N) if rows >= N else rng.choice(N, rows, replace=False)
    idx = np.concatenate([base, rng.integers(0, N, rows - len(base))])
    return rng.permutation(idx).astype(np.int32)


def assert_gram_exact(y, idx, center, weights):
    """Every term w (y_i - c_i)(y_j - c_j) is a multiple of 1/2 and the magnitudes of a whole element's terms sum to less than
    2^53 / 2: every partial sum in any order, fused or not, is exactly representable."""
    assert np.array_equal(y, np.round(y)) and (center is None or np.array_equal(center, np.round(center)))
    assert weights is None or np.array_equal(weights * 2, np.round(weights * 2))
    assert float(gram_magnitude(y, idx, center, weights).max()) * 2 < 2.0 ** 53


# ------------------------------------------------------------------ 1: Gram over D on integers
GRAM_DIMS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 150, 200, 257]
GRAM_FORMS = ["plain", "center", "weights", "all"]
GRAM_DIM_ROWS, GRAM_DIM_LIST = 40, 53


def form_args(case, form):
    """-> dict(idx, center, weights) of a form of gram_dim_case."""
    return dict(idx=case["idx"] if form == "all" else None, center=case["center"] if form in ("center", "all") else None,
                weights={"weights": case["w_rows"], "all": case["w_list"]}.get(form))


@functools.lru_cache(maxsize=None)
def gram_dim_case(D):
    """40 integer rows, a list of 53 positions -> dict(y, idx, center, w_rows, w_list, want = {form: G})."""
    rng = np.random.default_rng(21000 + D)
    N, rows = GRAM_DIM_ROWS, GRAM_DIM_LIST
    y = ints(rng, (N, D))
    y[y[:, D - 1] == 0, D - 1] = 3.0                         # the last dimension carries weight in every row
    case = dict(D=D, y=y, idx=scrambled_idx(rng, N, rows), center=ints(rng, D, np.float64, 3),
                w_rows=WEIGHTS[rng.integers(0, len(WEIGHTS), N)], w_list=WEIGHTS[rng.integers(0, len(WEIGHTS), rows)])
    assert rows > N and len(set(case["idx"].tolist())) == N and not np.array_equal(np.sort(case["idx"]), case["idx"])
    case["want"] = {}
    for form in GRAM_FORMS:
        args = form_args(case, form)
        assert_gram_exact(y, **args)
        case["want"][form] = frozen(gram(y, **args))
    frozen(*(case[k] for k in ("y", "idx", "center", "w_rows", "w_list")))
    return case


# ------------------------------------------------------------------ 2: Gram over rows and chunks at D = 17
ROWS_D = 17
GRAM_ROWS = [1, 15, 16, 17, 511, 512, 513, 1024, 1025, 1537]


@functools.lru_cache(maxsize=None)
def gram_rows_case(rows, with_idx):
    """-> dict(y (N + 1, 17): the last row is zero and no list names it, idx or None, center, weights, want (centre and weights),
    chunks = [(r0, r1)], want_chunk = [the Gram of chunk c's list positions alone, weights, no centre])."""
    D = ROWS_D
    rng = np.random.default_rng(22000 + 2 * rows + with_idx)
    N = max(1, rows // 2 + 3) if with_idx else rows
    y = np.concatenate([ints(rng, (N, D)), np.zeros((1, D), np.float32)])
    y[:N][y[:N, 0] == 0, 0] = 2.0                            # no row vanishes: a row left out or taken twice changes G[0, 0] ...
    idx = scrambled_idx(rng, N, rows) if with_idx else None
    w = WEIGHTS[rng.integers(1, len(WEIGHTS), rows)]         # ... for no weight is zero here
    c = ints(rng, D, np.float64, 3)
    assert_gram_exact(y[:N], idx, c, w)
    chunks = chunk_ranges(rows, D)
    pos = np.arange(rows) if idx is None else idx
    alone = [frozen(gram(y[pos[r0:r1]], None, None, w[r0:r1])) for r0, r1 in chunks]
    assert all(g[0, 0] > 0 for g in alone) and np.array_equal(sum(alone), gram(y[:N], idx, None, w))
    frozen(y, w, c)
    return dict(rows=rows, N=N, y=y, idx=None if idx is None else frozen(idx), center=c, weights=w,
                want=frozen(gram(y[:N], idx, c, w)), chunks=chunks, want_chunk=alone)


def only_chunk(case, k):
    """The inputs of gram_rows_case with every list position outside chunk k turned into a zero row -> (y, idx)."""
    r0, r1 = case["chunks"][k]
    inside = np.zeros(case["rows"], bool)
    inside[r0:r1] = True
    if case["idx"] is None:
        y = case["y"].copy()
        y[:case["rows"]][~inside] = 0
        return y, None
    return case["y"], np.where(inside, case["idx"], case["N"]).astype(np.int32)


# ------------------------------------------------------------------ 2b: which half of a diagonal tile an element comes from
ONE_ROW_DIMS = [65, 150]


@functools.lru_cache(maxsize=None)
def one_row_case(D, f64):
    """One real-valued row with a weight of 0.1 and a centre: nothing is summed, so an element is fl(fl(w fl(y_i - c_i)) fl(y_j - c_j))
    whatever the order or fusing of the additions, and NumPy computes just that. The weight sits on the first factor, so (i, j) and
    (j, i) of a diagonal tile round differently: G must hold, in both places, the value of the pair with i <= j.
    -> (y (1, D), center, weights (1,), want, the number of pairs i < j inside a diagonal tile whose two orders differ)."""
    rng = np.random.default_rng(22500 + 2 * D + f64)
    y = rng.standard_normal((1, D)).astype(np.float64 if f64 else np.float32)
    c, w = rng.standard_normal(D) * 3.0, np.array([0.1])
    z = y[0].astype(np.float64) - c
    both = np.outer(w[0] * z, z)
    want = np.triu(both) + np.triu(both, 1).T
    i, j = np.nonzero(np.triu(both != both.T, 1))
    differ = int(np.sum(i // TILE == j // TILE))
    return frozen(y, c, w, want) + (differ,)


# ------------------------------------------------------------------ 3: the cap on chunks at the largest D
CAP_D = TRAIN_MAX_DIM
CAP_ROWS = [7 * GRAM_MIN_ROWS + 1, 8 * GRAM_MIN_ROWS + 1]    # 3585: 8 chunks wanted, 7 given, per = 513; 4097: per = 586
CAP_PROBE = np.array([0, 1, 63, 64, 65, 511, 512, 959, 960, 1022, 1023])


@functools.lru_cache(maxsize=None)
def gram_cap_case(rows):
    """-> dict(y (rows, 1024) fp32, center, weights, want)."""
    D = CAP_D
    rng = np.random.default_rng(23000 + rows)
    y = ints(rng, (rows, D))
    c = ints(rng, D, np.float64, 3)
    w = WEIGHTS[rng.integers(0, len(WEIGHTS), rows)]
    assert float(np.abs(w).sum()) * 49 * 2 < 2.0 ** 53       # |y - c| <= 7
    return dict(rows=rows, y=frozen(y), center=frozen(c), weights=frozen(w), want=frozen(gram(y, None, c, w)))


# ------------------------------------------------------------------ 4: column means
MEAN_ROWS = [1, 255, 256, 257, 513]
MEAN_DIMS = [1, 255, 256, 257, 1024]


@functools.lru_cache(maxsize=None)
def mean_case(rows, D):
    rng = np.random.default_rng(24000 + 2000 * rows + D)
    y = ints(rng, (rows, D))
    y[rows - 1, y[rows - 1] == 0] = 1.0                      # the last row counts in every column
    assert rows * 4 < 2 ** 53
    return frozen(y), frozen(colmean(y))


# ------------------------------------------------------------------ 5: class means
CLASS_DIMS = [1, 255, 256, 257, 1024]
CLASS_COUNTS = [1, 300, 2, 7, 3, 1, 300]
CLASS_N, CLASS_LEAD, CLASS_TRAIL = 400, 5, 4


@functools.lru_cache(maxsize=None)
def class_case(D):
    """-> (x (400, D), offsets (S + 1) with offsets[0] = 5, utts: a longer list of which the map is a slice, means, counts)."""
    rng = np.random.default_rng(25000 + D)
    N = CLASS_N
    x = ints(rng, (N, D))
    lists = [rng.choice(N, n, replace=False) for n in CLASS_COUNTS]
    utts = np.concatenate([rng.integers(0, N, CLASS_LEAD)] + lists + [rng.integers(0, N, CLASS_TRAIL)]).astype(np.int32)
    offsets = (CLASS_LEAD + np.concatenate([[0], np.cumsum(CLASS_COUNTS)])).astype(np.int32)
    assert offsets[0] > 0 and offsets[-1] < len(utts) and len(set(lists[1]) & set(lists[6])) > 0
    assert any(np.any(np.diff(u) < 0) and np.ptp(u) > N // 2 for u in lists)         # scattered over x, not ascending
    assert MAX_COUNT * 4 < 2 ** 53 and max(CLASS_COUNTS) == MAX_COUNT
    means, counts = class_means(x, offsets, utts)
    return frozen(x, offsets, utts, means, counts)


# ------------------------------------------------------------------ 6: EM projection
EM_S = [1, 63, 64, 65, 130]
EM_DIMS = [1, 15, 16, 17, 63, 64, 65, 150]


@functools.lru_cache(maxsize=None)
def em_case(S, D):
    """-> dict(mu (S, D), mbar, P (D, D), lam, counts, a, b)."""
    rng = np.random.default_rng(26000 + 1000 * S + D)
    mu, mbar, P = ints(rng, (S, D), np.float64), ints(rng, D, np.float64, 3), ints(rng, (D, D), np.float64)
    P[P[:, D - 1] == 0, D - 1] = 1.0                         # the last summed index reaches every output
    lam = LAMBDAS[rng.integers(0, len(LAMBDAS), D)]
    lam[D - 1] = 0.25
    counts = rng.integers(1, MAX_COUNT + 1, S).astype(np.int32)
    counts[S - 1] = MAX_COUNT
    counts[0] = 1 if S > 1 else MAX_COUNT
    # y: integers below D * 7 * 4; n lam and 1 + n lam: multiples of 1/4 below 2^10
    assert float(em_magnitude(mu, mbar, P).max()) < 2.0 ** 53 and np.array_equal(lam * 4, np.round(lam * 4)) and MAX_COUNT * 3 + 1 < 2 ** 51
    a, b = em_project(mu, mbar, P, lam, counts)
    return dict(S=S, D=D, mu=frozen(mu), mbar=frozen(mbar), P=frozen(P), lam=frozen(lam), counts=frozen(counts), a=frozen(a), b=frozen(b))


# ------------------------------------------------------------------ 7: real-valued rows, derived bounds
REAL_DIMS = [65, 150, 200]
REAL_N, REAL_LIST = 1100, 1300                               # three chunks each, per = 367 and 434: no multiple of KSTEP
REAL_S = 130
REAL_FORMS = ["center", "all"]


def gram_bound(rows, magnitude):
    """|G - ref| <= (rows + 4) 2^-53 sum_r |w_r| |y_ri - c_i| |y_rj - c_j|: a dot product of `rows` terms in any order (rows - 1
    additions and one rounding of each product), the two subtractions and the weight."""
    return (rows + 4) * U64 * magnitude


def em_bound(D, scale, magnitude):
    """(D + 5) 2^-53 |scale| sum_k |mu_sk - mbar_k| |P_dk|, scale = nl / den for a and 1 / den for b: the dot product of D terms, the
    subtraction, n lam, 1 + n lam, the division and the product."""
    return (D + 5) * U64 * np.abs(scale) * magnitude


@functools.lru_cache(maxsize=None)
def real_gram_case(D, f64):
    """Standard-normal rows (fp32, or fp64 for the `_f64` instance), a centre of size 3
    -> dict(y, idx, center, weights, ref = {form: np.longdouble G}, bound = {form: E}, gap = {form: max (fp64 oracle - ref) / E})."""
    rng = np.random.default_rng(27000 + 2 * D + f64)
    y = rng.standard_normal((REAL_N, D)).astype(np.float64 if f64 else np.float32)
    case = dict(D=D, y=frozen(y), idx=frozen(scrambled_idx(rng, REAL_N, REAL_LIST)), center=frozen(rng.standard_normal(D) * 3.0),
                weights=frozen(rng.uniform(0.0, 2.0, REAL_LIST)), ref={}, bound={}, gap={})
    for form in REAL_FORMS:
        args = real_form_args(case, form)
        rows = REAL_LIST if form == "all" else REAL_N
        assert len(chunk_ranges(rows, D)) == 3 and (chunk_ranges(rows, D)[0][1] % KSTEP) != 0
        case["ref"][form] = frozen(gram(y, dtype=np.longdouble, **args))
        case["bound"][form] = frozen(gram_bound(rows, gram_magnitude(y, **args)))
        case["gap"][form] = float((np.abs(gram(y, **args) - case["ref"][form]) / case["bound"][form]).max())
    return case


def real_form_args(case, form):
    return dict(idx=case["idx"] if form == "all" else None, center=case["center"], weights=case["weights"] if form == "all" else None)


@functools.lru_cache(maxsize=None)
def real_em_case(D):
    """-> dict(mu, mbar, P, lam, counts, ref = (a, b) np.longdouble, bound = (Ea, Eb), gap = max (fp64 oracle - ref) / E)."""
    rng = np.random.default_rng(28000 + D)
    S = REAL_S
    mu, mbar, P = rng.standard_normal((S, D)), rng.standard_normal(D) * 3.0, rng.standard_normal((D, D)) / np.sqrt(D)
    lam = rng.uniform(0.01, 5.0, D)
    counts = rng.integers(1, MAX_COUNT + 1, S).astype(np.int32)
    ref = em_project(mu, mbar, P, lam, counts, np.longdouble)
    nl = counts[:, None] * lam[None, :]
    mag = em_magnitude(mu, mbar, P)
    bound = em_bound(D, nl / (1 + nl), mag), em_bound(D, 1 / (1 + nl), mag)
    got = em_project(mu, mbar, P, lam, counts)
    gap = max(float((np.abs(g - r) / e).max()) for g, r, e in zip(got, ref, bound))
    return dict(S=S, D=D, mu=frozen(mu), mbar=frozen(mbar), P=frozen(P), lam=frozen(lam), counts=frozen(counts),
                ref=frozen(*ref), bound=frozen(*bound), gap=gap)


# ------------------------------------------------------------------ 8: the estimators at the dimensions recipes use
MODEL_DIMS = [65, 150, 200]
MODEL_SPEAKERS = 300
MODEL_LDA = [(f, quarter) for f in (0.0, 0.1) for quarter in (True, False)]       # dim = D // 4 or D
MODEL_PCA = [(False, False, False), (False, True, True), (True, True, False), (True, False, True)]   # (dim = D // 2 or all, mean, variance)


@functools.lru_cache(maxsize=None)
def model_data(D, seed=1):
    """fp32 rows of a PLDA model: 300 speakers of 1 .. 8 rows, the generator and spectra of tests/test_gpu_plda_train.py
    -> (x, spk2utt, phi_w, phi_b)."""
    rng = np.random.default_rng(seed * 1000 + D)
    phi_b = spd(rng, geom(20.0, D, 0.985))
    phi_w = spd(rng, geom(2.0, D, 0.99))
    x, spk = R.sample_plda(rng, D, MODEL_SPEAKERS, 1, 8, phi_w, phi_b, rng.standard_normal(D) * 3.0)
    assert {len(u) for u in spk} == set(range(1, 9))
    return frozen(x.astype(np.float32)), spk, phi_w, phi_b


def lda_dim(D, quarter):
    return D // 4 if quarter else D


def pca_dim(D, half):
    return D // 2 if half else -1


@functools.lru_cache(maxsize=None)
def model_ref(D, permuted=False):
    """The oracle's models on model_data(D): dict(plda = (mean, T, psi), lda = {(f, quarter): A}, pca = {(half, mean, var): t});
    `permuted`: on the same rows with the speakers and every speaker's rows in another order."""
    x, spk, *_ = model_data(D)
    if permuted:
        rng = np.random.default_rng(3)
        spk = [list(rng.permutation(spk[s])) for s in rng.permutation(len(spk))]
    x = x.astype(np.float64)
    rows = x[np.random.default_rng(4).permutation(len(x))] if permuted else x        # est_pca takes no map: its rows move
    return dict(plda=R.compute_plda(x, spk),
                lda={(f, q): R.compute_lda(x, spk, lda_dim(D, q), total_covariance_factor=f) for f, q in MODEL_LDA},
                pca={(h, m, v): R.est_pca(rows, pca_dim(D, h), m, v) for h, m, v in MODEL_PCA})


@functools.lru_cache(maxsize=None)
def heldout(D, seed=5, S=60, per=3):
    """A held-out trial set of model_data(D)'s spectra: (enrollment means (S, D), test rows (S, D)), every class against every row."""
    _, _, phi_w, phi_b = model_data(D)
    x, spk = R.sample_plda(np.random.default_rng(seed), D, S, per + 1, per + 1, phi_w, phi_b, np.zeros(D))
    return frozen(np.stack([x[u[:per]].mean(0) for u in spk]), x[[u[per] for u in spk]]), per


def plda_scores(model, enroll, test, n):
    """Kaldi's Plda::LogLikelihoodRatio (no length normalisation) of every enrollment mean of n rows against every test row."""
    mean, T, psi = model
    e, t = (enroll - mean) @ T.T, (test - mean) @ T.T
    m = (n * psi / (n * psi + 1.0)) * e                                       # (S, D)
    v = 1.0 + psi / (n * psi + 1.0)
    given = -0.5 * (np.log(v).sum() + (((t[None] - m[:, None]) ** 2) / v).sum(-1))
    without = -0.5 * (np.log(1.0 + psi).sum() + ((t ** 2) / (1.0 + psi)).sum(-1))
    return given - without[None]
