"""Oracle, error bounds and input generator for the PLDA transform and scoring kernels (plda_common.h, the PLDA entry points of
pool_post.hip, the cohort launcher of score_norm.hip): tests/test_plda_score_ref_cpu.py and tests/test_gpu_plda_score_edges.py.

The formulas are those of tests/_verif_ref.py (V.llr, V.transform), evaluated in fp64 by default. `prec` selects the precision of
the evaluation: the fp64 kernels are held to a bound in units of 2^-53, which an fp64 reference would use up itself, so their
tests evaluate the same expressions in NumPy's long double (64-bit mantissa on x86; where long double is fp64 this is the fp64
oracle again).

Bounds. A kernel result is a sum of `dim` terms, each the outcome of a short chain of rounded operations. With u the unit
roundoff, S the sum of the terms' magnitudes before any cancellation and k the number of roundings on the longest chain of one
term, the first-order error of any order of summation is at most (dim + k) u S: dim - 1 additions of the sum (counted as dim)
and k roundings of relative size u on a term. The constants are counted below from the kernels' operations; they are not fitted.
"""

import numpy as np

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}

# Roundings on the chain of one quadratic term (y_i - k e_j)^2 / var1 of a score (plda_score_tile, plda_trials_kernel):
#   3  the staged k e_j = p * e / (p + 1): product, sum, quotient
#   4  the weight 1 / var1 = 1 / (1 + p / (p + 1)): sum, quotient, sum, quotient
#   3  the difference, the square, the product with the weight
#   2  the final combination: ld1 + a and the difference of the two halves (the factors -0.5 are exact)
# The other chains are shorter: log var1 (3 for the argument, 2 for a logarithm at its documented 1 ulp = 2 u, 2 for the final
# combination), log(1 + p) (1 + 2 + 2), y^2 / (1 + p) (square, sum, quotient, product, 2 for the final combination).
# The count forms compute n * p first. That product is exact for n = 1 and otherwise one rounding d, shared by the mean, which it
# moves by d / (n p + 1), and the variance, which it moves by less than d n p / (n p + 1): together less than one rounding of
# the term. The count forms are held to the same 12, the stricter figure.
K_SCORE = 12

# y_r = sum_c A_rc x_c + offset_r (plda_transform_row): one product per term, dim - 1 additions, the addition of the offset.
K_AFFINE = 2

# The scale factor of the length normalisation, relative, and the product that applies it. Per term of tot = sum v^2 / (p + 1 / n):
#   4  1 / n, p + 1 / n, v * v, the quotient            (simple_length_norm: 1, the square)
#   1  dim / tot                                          (simple_length_norm: 2 + 2 + 1, sqrt(dim), sqrt(tot), their quotient)
#   2  the square root at 1 ulp
#   1  y_r * f
# (the square root halves what reaches it; the counts leave that margin unused)
K_F = 8
K_F_SIMPLE = 7

# the dimensions at which the kernels change path: 16 lanes per trial, the 64-dimension LDS chunk and the 64-lane strides, the 256
# threads of the reductions (wave_sum_as_256: a second term per lane above 256, empty quarters below 193)
DIMS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 129, 255, 256, 257, 300, 513)
EDGE_DIMS = (0, 15, 16, 63, 64, 255, 256)
SPECIAL_PSI = (0.0, 1e-6, 1e4)


def edge_dims(dim):
    """The edge dimensions that exist at `dim`, dim - 1 among them."""
    return sorted({d for d in EDGE_DIMS + (dim - 1,) if 0 <= d < dim})


# ----------------------------------------------------------------------------- inputs
def make_counts(M, rng):
    """[1, 50, 2] followed by random integers in 1..50: classes of a second tile get other counts than the first tile's."""
    n = rng.integers(1, 51, size=M).astype(np.float64)
    n[:3] = [1.0, 50.0, 2.0][:M]
    return n


def make_psi(dim, npdt, rng):
    """Unsorted; in [0.5, 30] at every edge dimension (psi = 0 makes a dimension's two halves cancel exactly: a kernel that dropped
    it would pass); 0, 1e-6 and 1e4 at the interior positions 1, 2, 3 when dim > 4; rounded to npdt."""
    psi = rng.uniform(0.05, 30.0, dim)
    edges = edge_dims(dim)
    psi[edges] = rng.uniform(0.5, 30.0, len(edges))
    if dim > 4:
        psi[1:4] = SPECIAL_PSI
    return psi.astype(npdt)


def score_inputs(dim, N, M, npdt, seed=0):
    """(y (N, dim), e (M, dim), psi (dim), n (M)): standard normal vectors handed to the scoring entry points as they are, rounded
    to npdt before the oracle sees them; n in fp64 (integers: exact in either dtype)."""
    rng = np.random.default_rng([seed, dim, N, M])
    psi = make_psi(dim, npdt, rng)
    y = rng.standard_normal((N, dim)).astype(npdt)
    e = rng.standard_normal((M, dim)).astype(npdt)
    return y, e, psi, make_counts(M, rng)


def transform_inputs(dim, B, npdt, seed=0):
    """(x (B, dim), A (dim, dim), offset (dim), psi (dim), n (B)) rounded to npdt."""
    rng = np.random.default_rng([seed, dim, B, 7])
    psi = make_psi(dim, npdt, rng)
    A = (rng.standard_normal((dim, dim)) / np.sqrt(dim) + np.eye(dim)).astype(npdt)
    offset = rng.standard_normal(dim).astype(npdt)
    x = rng.standard_normal((B, dim)).astype(npdt)
    return x, A, offset, psi, make_counts(B, rng)


# ----------------------------------------------------------------------------- scores
def _class_terms(enroll_tr, psi, n, prec):
    e = np.asarray(enroll_tr, prec)
    psi = np.asarray(psi, prec)
    n = np.broadcast_to(np.asarray(n, prec), (e.shape[0],))[:, None]
    ke = n * psi / (n * psi + 1) * e                                # (M, dim)
    var1 = 1 + psi / (n * psi + 1)
    return ke, var1, psi


def llr(test_tr, enroll_tr, psi, n=1.0, prec=np.float64, rows=16):
    """V.llr: LogLikelihoodRatio(enroll_j, n_j, test_i) -> (N, M), in `prec`, `rows` test rows at a time."""
    y = np.asarray(test_tr, prec)
    ke, var1, psi = _class_terms(enroll_tr, psi, n, prec)
    ld1 = np.sum(np.log(var1), axis=1)                              # (M,)
    out = np.empty((y.shape[0], ke.shape[0]), prec)
    for r in range(0, y.shape[0], rows):
        yb = y[r:r + rows]
        given = -0.5 * (ld1[None, :] + np.sum((yb[:, None, :] - ke[None]) ** 2 / var1[None], axis=2))
        without = -0.5 * np.sum(np.log(1 + psi) + yb ** 2 / (1 + psi), axis=1)
        out[r:r + rows] = given - without[:, None]
    return out


def llr_mags(test_tr, enroll_tr, psi, n=1.0, prec=np.float64, rows=16):
    """S (N, M): half the sum over the dimensions of the magnitudes of every term of a score before cancellation,
    |log var1| + (|y_i| + |k_j e_j|)^2 / var1 + log(1 + psi) + y_i^2 / (1 + psi). The kernel rounds k e before it subtracts, so
    (y - k e)^2 does not bound what that rounding can move; (|y| + |k e|)^2 does."""
    y = np.abs(np.asarray(test_tr, prec))
    ke, var1, psi = _class_terms(enroll_tr, psi, n, prec)
    ke = np.abs(ke)
    l1 = np.sum(np.abs(np.log(var1)), axis=1)
    out = np.empty((y.shape[0], ke.shape[0]), prec)
    for r in range(0, y.shape[0], rows):
        yb = y[r:r + rows]
        q = np.sum((yb[:, None, :] + ke[None]) ** 2 / var1[None], axis=2)
        c = np.sum(np.log(1 + psi) + yb ** 2 / (1 + psi), axis=1)
        out[r:r + rows] = 0.5 * (l1[None, :] + q + c[:, None])
    return out


def score_bound(S, dim, npdt):
    """|got - ref| <= (dim + K_SCORE) u S, per element."""
    return (dim + K_SCORE) * U[np.dtype(npdt)] * S


# ----------------------------------------------------------------------------- transform
def _affine(x, A, offset, prec):
    return np.asarray(x, prec) @ np.asarray(A, prec).T + np.asarray(offset, prec)


def _denominators(y, psi, n, simple_length_norm, prec):
    if simple_length_norm:
        return np.ones_like(y)
    n = np.broadcast_to(np.asarray(n, prec), (y.shape[0],))[:, None]
    return np.asarray(psi, prec)[None, :] + 1 / n


def transform(x, A, offset, psi, n=1.0, normalize_length=True, simple_length_norm=False, prec=np.float64):
    """V.transform with the affine part as the kernels take it, y = A x + offset (V.transform(x, mean, T) with A = T and
    offset = -T mean), in `prec`."""
    y = _affine(x, A, offset, prec)
    if not normalize_length:
        return y
    tot = np.sum(y * y / _denominators(y, psi, n, simple_length_norm, prec), axis=1, keepdims=True)
    return y * np.sqrt(y.shape[1] / tot)


def transform_mags(x, A, offset, psi=None, n=1.0, simple_length_norm=False, prec=np.float64):
    """(S (B, dim), tot (B,)): S_r = sum_c |A_rc x_c| + |offset_r| for the affine part; the length normalisation's sum has
    non-negative terms only, so its magnitude is its value."""
    S = np.abs(np.asarray(x, prec)) @ np.abs(np.asarray(A, prec)).T + np.abs(np.asarray(offset, prec))
    if psi is None:
        return S, None
    y = _affine(x, A, offset, prec)
    return S, np.sum(y * y / _denominators(y, psi, n, simple_length_norm, prec), axis=1)


def transform_bound(x, A, offset, psi, n, normalize_length, simple_length_norm, npdt, prec=np.float64):
    """(B, dim) bound on |got - ref|. Affine part: E_r = (dim + K_AFFINE) u S_r. With the length normalisation out_r = y_r f:
    E_r f, plus |out_r| times the relative error of f. f has (dim + k_f) u of its own, and it is computed from the rounded y: an
    error E_r on y_r moves tot by 2 |y_r| E_r / den_r and f, an inverse square root of tot, by half of that relative to tot."""
    u = U[np.dtype(npdt)]
    dim = np.asarray(x).shape[1]
    S, _ = transform_mags(x, A, offset, prec=prec)
    E = (dim + K_AFFINE) * u * S
    if not normalize_length:
        return E
    y = _affine(x, A, offset, prec)
    den = _denominators(y, psi, n, simple_length_norm, prec)
    tot = np.sum(y * y / den, axis=1, keepdims=True)
    f = np.sqrt(dim / tot)
    rel_f = (dim + (K_F_SIMPLE if simple_length_norm else K_F)) * u + np.sum(np.abs(y) * E / den, axis=1, keepdims=True) / tot
    return f * E + np.abs(y) * f * rel_f
