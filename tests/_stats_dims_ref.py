"""Case builders for the GMM, full-covariance and i-vector statistics kernels along the three axes that choose their code path: the
feature dimension D (1 .. 128), the number of (frame, slot) pairs and the i-vector dimension S. The oracles are the existing fp64
restatements (_ubm_train_ref, _fgmm_ref, _ivector_ref, _ivector_train_ref); this module only builds inputs that reach a given
kernel instance or split and, for the integer cases, proves that every partial sum is exactly representable, so that the kernel's
output must EQUAL the oracle's whatever its summation order. Every builder is cached and returns read-only arrays.

Internal constants of the kernels, mirrored here because the library does not export them (the CPU test checks the cases against
them; a changed constant moves the edge, not the correctness of a test)."""

import functools
import types

import numpy as np

import _fgmm_ref as G
import _ivector_ref as R
import _ivector_train_ref as T
import _ubm_train_ref as U
from kaldi_tflite_amd import _lib as L

SEC_CH = 8192                      # gmm_bucket.h:11, pairs per chunk of the ordered scatter
SEC_CH_ANY = 32768                 # gmm_bucket.h:12, pairs per chunk of the unordered scatter
FG_ROWS = 512                      # fgmm.hip:20, rows of a bucket per quadratic-form workgroup
FG_TILE, FG_WAVES = 32, 4          # fgmm.hip:19 / :66, a wave's tile of rows and the waves that share an item
GKC = 2048                         # ivector_stages.h:8, K chunk of the fp64 GEMMs (K = I D for the linear term, I for the quadratic)
GT = 64                            # ivector_stages.hip:9, GEMM tile rows (one row per utterance)
IVS_WAVES, IVS_BATCH = 4, 8        # ivector_stages.hip:7-8, Gaussian owners per utterance; owned slots per run
NB = 32                            # ivector_stages.hip:12, Cholesky panel width
SEC_RB = 16                        # ivector_train.hip:22, bucket rows staged per step of the second-order kernel
IVP_FT, IVP_GT = 32, 256           # gmm_loglike.h:10-11, frames per workgroup and Gaussians per tile of the posterior kernel
ITEM_ROWS = L.GMM_ACC_ITEM_ROWS    # include/ktf_hip.h KTF_GMM_ACC_ITEM_ROWS, rows of a bucket per statistics item
MAX_D, MAX_N, MAX_S = L.IVECTOR_MAX_FEAT_DIM, L.IVECTOR_MAX_GSELECT, L.IVECTOR_MAX_DIM

D_EDGES = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 111, 112, 127, 128]


def gacc_nt(D):
    """gmm_train.hip gacc_nt: 16-wide tiles along z = [1, x] of gacc_full_kernel<NT>."""
    return (D + 1 + 15) // 16


def fg_nj(D):
    """fgmm.hip fg_dp(D) / 32: blocks of 32 output dimensions of fg_quad_kernel<NJ>."""
    return (D + 31) // 32


def gamma_group(D):
    """ivstats_kernel: a lane owns columns lane, lane + 64, lane + 128 of [x, gamma]; -> (group, lane) of the gamma column D."""
    return D // 64, D % 64


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def padded(x, pad=3):
    """x (F, D) -> a (F, D + pad) buffer whose pad columns hold NaN: the kernel is handed the first D columns with row stride
    D + pad, and a read beyond D turns the result NaN."""
    buf = np.full((x.shape[0], x.shape[1] + pad), np.nan, np.float32)
    buf[:, :x.shape[1]] = x
    return buf


def place_counts(rng, shape, counts, I):
    """A slot array of `shape` in which Gaussian g sits in exactly counts[g] slots at random places; the other slots hold -1 or an
    index >= I, about half each."""
    total = int(np.prod(shape))
    assert sum(counts) <= total
    flat = np.where(rng.random(total) < 0.5, -1, I + rng.integers(0, 4, total)).astype(np.int32)
    where = rng.permutation(total)[:sum(counts)]
    flat[where] = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    return flat.reshape(shape)


# ------------------------------------------------------------------ 1 / 8: gmm_acc on integers
ACC_POST = np.array([0.0, 0.25, 0.5, 1.0, 2.0], np.float32)


def assert_acc_exact(x, gauss, post, I):
    """Every term p, p x, p x_i x_j is a multiple of 1/4 and the magnitudes of a whole accumulator sum to less than 2^53 / 4: any
    order of fp64 additions (and the fused multiply-adds) gives the exact sum."""
    ok = (gauss >= 0) & (gauss < I)
    assert np.array_equal(x, np.round(x)) and np.array_equal(post * 4, np.round(post * 4))
    assert float(post[ok].sum()) * max(1.0, float(np.abs(x).max())) ** 2 * 4 < 2.0 ** 53


@functools.lru_cache(maxsize=None)
def acc_case(D):
    """I = 5, n = 3, F = 151; -> (x, gauss, post, {full: oracle})."""
    I, n, F = 5, 3, 151
    rng = np.random.default_rng(1000 + D)
    x = rng.integers(-4, 5, (F, D)).astype(np.float32)
    gauss = rng.integers(0, I - 1, (F, n)).astype(np.int32)              # Gaussian I - 1: nobody selects it
    gauss[rng.choice(F, 7, replace=False), rng.integers(0, n, 7)] = -1
    gauss[rng.choice(F, 5, replace=False), rng.integers(0, n, 5)] = I + rng.integers(0, 3, 5)
    post = ACC_POST[rng.integers(0, len(ACC_POST), (F, n))]
    assert (post == 0).any() and (gauss == -1).any() and (gauss >= I).any() and not (gauss == I - 1).any()
    assert_acc_exact(x, gauss, post, I)
    frozen(x, gauss, post)
    return x, gauss, post, {full: U.stats_on_pairs(x, gauss, post, I, full) for full in (False, True)}


ITEM_COUNTS = [ITEM_ROWS - 1, ITEM_ROWS, ITEM_ROWS + 1, 2 * ITEM_ROWS, 2 * ITEM_ROWS + 1, 0]


@functools.lru_cache(maxsize=None)
def acc_items_case():
    """D = 17, I = 6, the Gaussians' pair counts on the item edges, more pairs than one chunk of the ordered scatter."""
    D, I, n, F = 17, 6, 3, 2800
    rng = np.random.default_rng(1800)
    x = rng.integers(-4, 5, (F, D)).astype(np.float32)
    gauss = place_counts(rng, (F, n), ITEM_COUNTS, I)
    post = ACC_POST[rng.integers(0, len(ACC_POST), (F, n))]
    assert F * n > SEC_CH and np.bincount(gauss[(gauss >= 0) & (gauss < I)], minlength=I).tolist() == ITEM_COUNTS
    assert_acc_exact(x, gauss, post, I)
    frozen(x, gauss, post)
    return x, gauss, post, {full: U.stats_on_pairs(x, gauss, post, I, full) for full in (False, True)}


# ------------------------------------------------------------------ 2 / 3: one valid entry per list, integer models
def single_lists(rng, valid_g, n, I, empty=()):
    """(F, n) lists with the one valid entry valid_g[t] at slot t % n (a permuted slot order), -1 or an index >= I elsewhere; the
    frames in `empty` hold no valid entry."""
    F = len(valid_g)
    sel = np.where(rng.random((F, n)) < 0.5, -1, I + rng.integers(0, 4, (F, n))).astype(np.int32)
    slot = rng.permutation(F) % n
    keep = np.ones(F, bool)
    keep[list(empty)] = False
    sel[np.arange(F)[keep], slot[keep]] = np.asarray(valid_g, np.int32)[keep]
    return sel, slot


FG_EXACT_COUNTS = [10, 70, 16, 5]   # rows per Gaussian: Gaussian 1's waves see two full tiles, a partial one and an empty one


@functools.lru_cache(maxsize=None)
def fgmm_exact_case(D):
    """I = 4, n = 5, F = 3 * 32 + 5 -> (x, sel, slot, (gconst, means_invcovars, inv_covars) fp32, loglike (F) fp32)."""
    I, n, F = 4, 5, 3 * FG_TILE + 5
    assert sum(FG_EXACT_COUNTS) == F
    rng = np.random.default_rng(2000 + D)
    x = rng.integers(-3, 4, (F, D)).astype(np.float32)
    A = rng.integers(-1, 2, (I, D, D))
    ic = (np.triu(A) + np.swapaxes(np.triu(A, 1), 1, 2)).astype(np.float32)
    assert np.array_equal(ic, np.swapaxes(ic, 1, 2))
    mic = rng.integers(-3, 4, (I, D)).astype(np.float32)
    gc = rng.integers(-5, 6, I).astype(np.float32)
    valid_g = rng.permutation(np.repeat(np.arange(I), FG_EXACT_COUNTS))
    sel, slot = single_lists(rng, valid_g, n, I)
    # exactness: every term is a multiple of 1/2 and the magnitudes of a pair's terms sum to less than 2^23, so every partial sum
    # in any order (fused or not) is a multiple of 1/2 below 2^23: exactly representable in fp32
    ax = np.abs(x).astype(np.float64)
    mag = np.abs(gc)[valid_g] + np.einsum("fd,fd->f", ax, np.abs(mic)[valid_g]) + \
        0.5 * np.einsum("fd,fde,fe->f", ax, np.abs(ic).astype(np.float64)[valid_g], ax)
    assert mag.max() < 2.0 ** 23
    ll = G.loglikes_on(x, (gc, mic, ic), sel)
    assert np.array_equal(np.isfinite(ll).sum(1), np.ones(F)) and np.all(np.isfinite(ll[np.arange(F), slot]))
    want = ll[np.arange(F), slot]
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    return frozen(x, sel, slot, valid_g) + ((frozen(gc), frozen(mic), frozen(ic)), frozen(want.astype(np.float32)))


PRESELECT_CASES = [(D, n) for D in (1, 63, 64, 65, 127, 128) for n in (1, 64)]


@functools.lru_cache(maxsize=None)
def preselect_case(D, n):
    """an integer diagonal model, I = 6, F = 37, two frames with an empty list
    -> (x, sel, slot, model (gconsts, means_invvars, inv_vars), loglike (F) fp32, the empty frames)."""
    I, F, empty = 6, 37, (4, 30)
    rng = np.random.default_rng(3000 + 10 * D + n)
    x = rng.integers(-3, 4, (F, D)).astype(np.float32)
    model = types.SimpleNamespace(gconsts=rng.integers(-5, 6, I).astype(np.float32), means_invvars=rng.integers(-2, 3, (I, D)).astype(np.float32),
                                  inv_vars=rng.integers(1, 3, (I, D)).astype(np.float32), numGauss=I, featDim=D)
    valid_g = rng.integers(0, I, F)
    sel, slot = single_lists(rng, valid_g, n, I, empty)
    ax = np.abs(x).astype(np.float64)
    mag = np.abs(model.gconsts)[valid_g] + np.einsum("fd,fd->f", ax, np.abs(model.means_invvars)[valid_g]) + \
        0.5 * np.einsum("fd,fd->f", ax * ax, model.inv_vars[valid_g])
    assert mag.max() < 2.0 ** 23                               # multiples of 1/2 below 2^23: exact in fp32 in any order
    _, ll, valid = U.softmax_rows(U.on_list(U.diag_loglikes(x, model), sel))
    assert valid.sum() == F - len(empty) and not valid[list(empty)].any()
    assert np.array_equal(ll.astype(np.float32).astype(np.float64), ll)
    frozen(model.gconsts, model.means_invvars, model.inv_vars)
    return frozen(x, sel, slot) + (model, frozen(ll.astype(np.float32)), empty)


# ------------------------------------------------------------------ 4: ivector_post on integer log-likelihoods with ties
# (D, I, n, F): every D in {1, 64, 65, 127, 128}, I in {1, 40, 255, 256, 257, 513}, n in {1, 20, 63, 64}, F in {31, 32, 33} at
# least once; I < n in the second; D = 128 with n = 64 is the launch with the largest dynamic LDS
IVPOST_CASES = [(1, 1, 1, 31), (1, 40, 64, 32), (64, 255, 20, 33), (65, 256, 63, 31), (127, 257, 64, 32), (128, 513, 64, 33),
                (128, 40, 20, 32), (64, 513, 1, 31), (65, 257, 20, 33), (127, 256, 64, 31), (1, 513, 63, 32), (128, 255, 63, 33)]


def ivpost_twins(I):
    """(g, its exact copy): g and g + 256 on both sides of a tile boundary, the neighbours 255 / 256, and one pair inside a tile."""
    pairs = [(g, g + IVP_GT) for g in (0, 5, 100, 250) if g + IVP_GT < I]
    if I > IVP_GT:
        pairs.append((IVP_GT - 1, IVP_GT))
    if I > 2:
        pairs.append((1, 2))
    return pairs


@functools.lru_cache(maxsize=None)
def ivpost_case(k):
    """-> (x, W (2D, I), gconst, (gauss, post) of the oracle, info): x and W integers, so every log-likelihood is an integer that
    fp32 holds exactly in any summation order. Few mean coordinates are non-zero and few inverse variances differ from 2, so that
    few distinct values occur and ties abound; the last dimension's mean and inverse variance differ from Gaussian to Gaussian, so
    that the last x row and the last x^2 row of W (k = D - 1 and k = 2 D - 1) decide selections."""
    D, I, n, F = IVPOST_CASES[k]
    rng = np.random.default_rng(4000 + k)
    x = rng.integers(-2, 3, (F, D)).astype(np.float32)
    mi = np.zeros((I, D), np.float32)
    for g in range(I):
        dims = rng.choice(D, min(D, 2), replace=False)
        mi[g, dims] = rng.integers(-2, 3, len(dims))
    iv = np.full((I, D), 2.0, np.float32)                   # -iv / 2 stays an integer: inverse variances of 2 and 4
    for g in range(I):
        iv[g, rng.choice(D, min(D, 2), replace=False)] = 4.0
    mi[:, D - 1] = rng.integers(-2, 3, I)
    iv[:, D - 1] = rng.choice([2.0, 4.0], I)
    gc = rng.integers(-2, 1, I).astype(np.float32)
    for a, b in ivpost_twins(I):
        mi[b], iv[b], gc[b] = mi[a], iv[a], gc[a]
    W = np.ascontiguousarray(np.concatenate([mi.T, (np.float32(-0.5) * iv).T]))
    ax = np.abs(x).astype(np.float64)
    assert (np.abs(gc).max() + (ax @ np.abs(mi).T).max() + 0.5 * ((ax * ax) @ iv.T).max()) < 2.0 ** 23
    ll = R.loglikes(x, (gc, mi, iv))
    assert np.array_equal(ll, np.round(ll))
    keep = min(n, I)
    ties = straddle = 0
    if keep < I:
        for t in range(F):
            order = np.lexsort((np.arange(I), -ll[t]))
            if ll[t, order[keep - 1]] == ll[t, order[keep]]:
                ties += 1
                group = np.nonzero(ll[t] == ll[t, order[keep]])[0]
                straddle += int(group.min() // IVP_GT != group.max() // IVP_GT)
    g, p = R.posteriors(x, (gc, mi, iv), n, 0.0)
    return frozen(x, W, gc) + (frozen(g, p), dict(ties_at_cut=ties, ties_across_tiles=straddle, lds=ivpost_lds_bytes(D, keep)))


def ivpost_lds_bytes(D, keep):
    """ivector.hip ivpost_lds_bytes: [x, x^2] of 32 frames, the 32 x 257 tile, the sorted lists and their counts."""
    return 4 * (2 * D * IVP_FT + IVP_FT * (IVP_GT + 1) + 2 * IVP_FT * keep + IVP_FT)


# ------------------------------------------------------------------ 5: i-vector statistics at n = 64
# (D, I): I = 8 at every D (a wave owns two Gaussians, so a kind-(a) frame is 32 runs of two through the `dup` branch),
# and I = 40 at two D (ten Gaussians per wave: runs of IVS_BATCH distinct Gaussians, a second run in the same frame)
IVSTATS_CASES = [(D, 8) for D in (1, 63, 64, 65, 127, 128)] + [(64, 40), (127, 40)]
IVSTATS_LENS = [0, 1, 9, 30]
IVSTATS_S, IVSTATS_PRIOR = 5, 30.0
IVSTATS_SCALES = [dict(posterior_scale=1.0, acoustic_weight=0.5, max_count=3.0), dict(posterior_scale=1.0, acoustic_weight=0.5, max_count=0.0)]


def ivstats_frame(rng, kind, I, n):
    if kind == 0:                                            # (a) one wave owns every slot
        own = np.arange(int(rng.integers(0, IVS_WAVES)), I, IVS_WAVES)
        return own[rng.integers(0, len(own), n)]
    if kind == 1:                                            # (b) one Gaussian in slots 0, 1, 9 and 63
        g = rng.integers(0, I, n)
        rep = int(rng.integers(0, I))
        g[g == rep] = (rep + 1) % I
        g[[0, 1, 9, 63]] = rep
        return g
    if kind == 2:                                            # (c) -1 and indices >= I mixed in
        g = rng.integers(0, I, n)
        r = rng.random(n)
        g[r < 0.25] = -1
        g[r > 0.75] = I + rng.integers(0, 5, int((r > 0.75).sum()))
        return g
    return np.concatenate([rng.permutation(I)[:min(I, n)], np.full(max(0, n - I), -1)])   # (d) distinct Gaussians, then unused


@functools.lru_cache(maxsize=None)
def ivstats_case(k):
    """-> dict(x, gauss, post, off, sim (I D, S), U, want = [per scales: (B, S) i-vectors], gamma = the exact sum over the utterances
    with frames of the unscaled statistics, Y (I, D, S) = sum_u F_u w_u^T and ivector_sum = sum_u w_u of the unscaled statistics,
    w_u the posterior mean with the prior offset in its first coordinate, as ivector-extractor-acc-stats accumulates them)."""
    D, I = IVSTATS_CASES[k]
    n, S, lens = MAX_N, IVSTATS_S, IVSTATS_LENS
    rng = np.random.default_rng(5000 + k)
    _, (M, sig) = R.random_models(rng, I, D, S, prior_offset=IVSTATS_PRIOR)
    sim, Upk = R.derived(M, sig)
    F = sum(lens)
    x = (rng.standard_normal((F, D)) * 1.3).astype(np.float32)
    # the one-frame utterance is of kind (a); the others cycle through the four kinds
    kinds = [0] + [t % 4 for t in range(F - 1)]
    gauss = np.stack([ivstats_frame(rng, kd, I, n) for kd in kinds]).astype(np.int32)
    post = (2.0 ** -rng.integers(0, 5, (F, n))).astype(np.float32)
    assert n == 64 and all(k in kinds[1:10] and k in kinds[10:] for k in range(4))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    # a slot outside [0, I) is skipped with its weight (the kernel is handed the non-zero weight): the oracle, whose count for
    # max_count is the sum of all the weights it is given, sees a zero there
    ok = (gauss >= 0) & (gauss < I)
    listed = np.where(ok, post, np.float32(0))
    assert (post[~ok] > 0).all() and (~ok).sum() > F
    want = []
    for sc in IVSTATS_SCALES:
        rows = []
        for b in range(len(lens)):
            lo, hi = off[b], off[b + 1]
            rows.append(R.extract_packed(*R.stats(x[lo:hi], gauss[lo:hi], listed[lo:hi], I, **sc), sim, Upk, IVSTATS_PRIOR))
        want.append(np.array(rows))
    total = 0.5 * float(post[off[3]:][ok[off[3]:]].sum())
    assert IVSTATS_SCALES[0]["max_count"] < total                 # the longest utterance is scaled down
    gamma = np.zeros(I)                                           # powers of two between 2^-4 and 1, < 2^12 of them: exact
    np.add.at(gamma, gauss[ok], post[ok].astype(np.float64))
    Y, isum = np.zeros((I, D, S)), np.zeros(S)
    for b in range(len(lens)):
        lo, hi = off[b], off[b + 1]
        if hi > lo:
            gm, Fm = R.stats(x[lo:hi], gauss[lo:hi], listed[lo:hi], I)
            w = R.extract_packed(gm, Fm, sim, Upk, IVSTATS_PRIOR)
            w[0] += IVSTATS_PRIOR
            Y += Fm[:, :, None] * w[None, None, :]
            isum += w
    return dict(D=D, I=I, n=n, S=S, lens=lens, x=frozen(x), gauss=frozen(gauss), post=frozen(post), off=frozen(off),
                sim=frozen(np.ascontiguousarray(sim.reshape(I * D, S))), U=frozen(np.ascontiguousarray(Upk)), want=want, gamma=frozen(gamma),
                Y=frozen(Y), ivector_sum=frozen(isum))


def longest_run(gauss_row, I):
    """The most slots of one frame that one wave of ivstats_kernel owns, and whether a Gaussian repeats among them."""
    g = gauss_row[(gauss_row >= 0) & (gauss_row < I)]
    best, dup = 0, False
    for w in range(IVS_WAVES):
        own = g[g % IVS_WAVES == w]
        best = max(best, len(own))
        dup |= len(set(own.tolist())) < len(own)
    return best, dup


# ------------------------------------------------------------------ 6: second-order statistics on integers
SEC_DIMS = [1, 16, 17, 32, 33, 64, 127, 128]
SEC_LAYOUTS = [[0, 1, SEC_RB, SEC_RB + 1], [40, SEC_RB, 0, 1]]    # bucket sizes of the I = 4 Gaussians: 0, 1, 16, 17 and 40
SEC_SCALE, SEC_POISON = 0.5, 7.0


@functools.lru_cache(maxsize=None)
def sec_case(D, layout):
    """-> (x, gauss, post, Ssec (I, D, D) of the oracle without the poison)."""
    I, n, counts = 4, 2, SEC_LAYOUTS[layout]
    F = (sum(counts) + n - 1) // n + 4
    rng = np.random.default_rng(6000 + 10 * D + layout)
    x = rng.integers(-4, 5, (F, D)).astype(np.float32)
    x[x == 0] = 3.0                                          # no zero: a bucket of one row leaves a mark in every element
    gauss = place_counts(rng, (F, n), counts, I)
    post = (2.0 ** -rng.integers(0, 4, (F, n))).astype(np.float32)
    # terms are multiples of 2^-4 of magnitude <= 16; with the poison fewer than 2^12 of them: far below 2^53
    assert float(post.sum()) * SEC_SCALE * 16 * 16 + SEC_POISON * 16 < 2.0 ** 53
    M = np.full((I, D, 1), 0.1)
    acc = T.accumulate([(x, gauss, post)], M, np.tile(np.eye(D), (I, 1, 1)), 1.0, posterior_scale=SEC_SCALE)
    return frozen(x, gauss, post) + (frozen(acc["Ssec"]),)


# ------------------------------------------------------------------ 7: the ordered scatter
BUCKET_I = [1, 257, 8192]
BUCKET_N = 3
BUCKET_F = (3 * SEC_CH + 5 + BUCKET_N - 1) // BUCKET_N        # 3 * 8192 + 5 is no multiple of 3: the next frame count, 3 * 8192 + 6 pairs


@functools.lru_cache(maxsize=None)
def bucket_case(I):
    """-> (gauss (F, n), start (I + 1), the kept pairs in stable order by Gaussian)."""
    F, n = BUCKET_F, BUCKET_N
    rng = np.random.default_rng(7000 + I)
    heavy = I // 2
    g = rng.integers(0, I, F * n)
    g[rng.random(F * n) < 0.5] = heavy
    r = rng.random(F * n)
    g[r < 0.03] = -1
    g[r > 0.97] = I + rng.integers(0, 3, int((r > 0.97).sum()))
    g = g.astype(np.int32)
    ok = (g >= 0) & (g < I)
    start = np.concatenate([[0], np.cumsum(np.bincount(g[ok], minlength=I))]).astype(np.int32)
    order = np.argsort(np.where(ok, g, I), kind="stable")[:int(ok.sum())].astype(np.int32)
    return frozen(g.reshape(F, n), start, order)


# ------------------------------------------------------------------ 9: the unordered scatter
ANY_F, ANY_N, ANY_I, ANY_D, ANY_TAIL = 2341, 15, 5, 8, 2100


@functools.lru_cache(maxsize=None)
def unordered_case():
    """-> (x, sel, (gconst, means_invcovars, inv_covars) fp32, dense (F, I) posteriors of the oracle, 0 for a Gaussian not listed)."""
    F, n, I, D = ANY_F, ANY_N, ANY_I, ANY_D
    rng = np.random.default_rng(9000)
    stored, (mean, cov) = G.random_full_ubm(rng, I, D)
    x = G.draw_frames(rng, mean, cov, F)
    full = (G.gconsts(*stored).astype(np.float32), stored[1], stored[2])
    sel = np.where(rng.random((F, n)) < 0.5, -1, I + rng.integers(0, 4, (F, n))).astype(np.int32)
    for t in range(F):
        k = int(rng.integers(0, I))                          # Gaussian 0 and k of the others, at random slots
        slots = rng.choice(n, 1 + k, replace=False)
        sel[t, slots] = np.concatenate([[0], 1 + rng.choice(I - 1, k, replace=False)])
    assert np.all((sel == 0).sum(1) == 1) and F > FG_ROWS
    wg, wp, _ = G.posteriors(x, full, sel, 0.0)
    return frozen(x, sel) + (full, frozen(dense_posts(wg, wp, I)))


def dense_posts(g, p, I):
    """(F, n) slots -> (F, I): the posterior of every Gaussian, 0 where it is not listed (no Gaussian is listed twice)."""
    out = np.zeros((g.shape[0], I))
    f, s = np.nonzero(g >= 0)
    assert len(set(zip(f.tolist(), g[f, s].tolist()))) == len(f)
    out[f, g[f, s]] = p[f, s]
    return out


# ------------------------------------------------------------------ 10 / 11: the S axis, the batch axis and the K edges
S_EDGES = [1, NB - 1, NB, NB + 1, 2 * NB, 2 * NB + 1, MAX_S]
S_LENS, S_I, S_D, S_N, S_PRIOR = [0, 40, 7], 3, 4, 2, 30.0


def diag_reader(w, mi, iv):
    from kaldi_tflite_amd.io import KaldiDiagGmmReader
    g = KaldiDiagGmmReader.__new__(KaldiDiagGmmReader)
    g.path, g.binary, g.storedGconsts = None, True, None
    g.weights, g.means_invvars, g.inv_vars = w, mi, iv
    g.numGauss, g.featDim = mi.shape
    g.gconsts = g.computeGconsts()
    return g


@functools.lru_cache(maxsize=None)
def s_case(S):
    """-> dict(M, sig, ubm, utts = [(x, gauss, post)], ivectors (B, S) by extract_packed, dense = the same by extract_dense, acc = the
    totals of _ivector_train_ref.accumulate, objf)."""
    I, D, n = S_I, S_D, S_N
    rng = np.random.default_rng(10000 + S)
    (w, mi, iv), (M, sig) = R.random_models(rng, I, D, S, prior_offset=S_PRIOR)
    ubm = diag_reader(w, mi, iv)
    utts = []
    for T_u in S_LENS:
        x = (rng.standard_normal((T_u, D)) * 1.3 + rng.standard_normal(D) * 0.5).astype(np.float32)
        g, p = R.posteriors(x, (ubm.gconsts, mi, iv), n, 0.025) if T_u else (np.zeros((0, n), np.int32), np.zeros((0, n)))
        utts.append((x, g, p.astype(np.float32)))
    sim, Upk = R.derived(M, sig)
    st = [R.stats(x, g, p, I) for x, g, p in utts]
    packed = np.array([R.extract_packed(gm, Fm, sim, Upk, S_PRIOR) for gm, Fm in st])
    dense = np.array([R.extract_dense(gm, Fm, M, sig, S_PRIOR) for gm, Fm in st])
    acc = T.accumulate(utts, M, sig, S_PRIOR)
    return dict(S=S, M=M, sig=sig, ubm=ubm, utts=utts, ivectors=packed, dense=dense, acc=acc, objf=T.marginal_objf(utts, M, sig, S_PRIOR))


# (I, D): K = I D of the linear term on 2047, 2048, 2049; K = I of the quadratic term on 2049
K_CASES = [(23, 89), (16, 128), (683, 3), (2049, 1)]
K_B, K_T, K_S, K_N, K_PRIOR = GT + 1, 3, 9, 4, 30.0


@functools.lru_cache(maxsize=None)
def k_case(k):
    """B = 65 utterances of 3 frames -> dict(x, gauss, post, off, sim, U, want (B, S))."""
    I, D = K_CASES[k]
    B, Tu, S, n = K_B, K_T, K_S, K_N
    rng = np.random.default_rng(11000 + k)
    _, (M, sig) = R.random_models(rng, I, D, S, prior_offset=K_PRIOR)
    sim, Upk = R.derived(M, sig)
    F = B * Tu
    x = (rng.standard_normal((F, D)) * 1.3).astype(np.float32)
    gauss = np.full((F, n), -1, np.int32)
    post = np.zeros((F, n), np.float32)
    for t in range(F):
        m = int(rng.integers(1, min(n, I) + 1))
        gauss[t, :m] = rng.choice(I, m, replace=False)
        q = rng.uniform(0.01, 1.0, m)
        post[t, :m] = np.sort(q / q.sum())[::-1]
    gauss[0, 0] = I - 1                                      # the last row of K is used
    off = (np.arange(B + 1) * Tu).astype(np.int32)
    want = np.array([R.extract_packed(*R.stats(x[off[b]:off[b + 1]], gauss[off[b]:off[b + 1]], post[off[b]:off[b + 1]], I), sim, Upk, K_PRIOR)
                     for b in range(B)])
    return dict(I=I, D=D, S=S, n=n, B=B, x=frozen(x), gauss=frozen(gauss), post=frozen(post), off=frozen(off),
                sim=frozen(np.ascontiguousarray(sim.reshape(I * D, S))), U=frozen(np.ascontiguousarray(Upk)), want=frozen(want))


# ------------------------------------------------------------------ 12: real-valued full-covariance frames at the new instances
REAL_DIMS = [65, 96, 97, 128]
REAL_I, REAL_N, REAL_F = 12, 7, 200
EPS32 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def real_case(D, tied=False):
    """`tied`: every component gets component 0's covariance and the means move ten times closer, so that the listed Gaussians
    compete (on the plain random_full_ubm frames at these D one Gaussian takes the whole posterior).
    -> dict(x, sel, full = (gconst, mic, ic) fp32, ll (F) and dense (F, I) posteriors of the fp64 oracle, E (F) the running-error
    bound of a frame's log-likelihoods, gap_ll / gap_post: the distance of the oracle in float32 arithmetic from the fp64 one)."""
    from kaldi_tflite_amd.io import FullGmmModel
    I, n, F = REAL_I, REAL_N, REAL_F
    rng = np.random.default_rng(12000 + D)
    stored, (mean, cov) = G.random_full_ubm(rng, I, D)
    if tied:
        mean, cov, ic0 = mean * 0.1, np.repeat(cov[:1], I, 0), np.repeat(stored[2][:1], I, 0)
        stored = (stored[0], np.einsum("ide,ie->id", ic0.astype(np.float64), mean).astype(np.float32), ic0)
    comp = rng.integers(0, I, F)
    x = G.draw_frames(rng, mean, cov, F, comp=comp)
    model = FullGmmModel(*stored)
    gc, mic, ic = (np.ascontiguousarray(a, dtype=np.float32) for a in (model.gconsts, model.means_invcovars, model.inv_covars))
    sel = np.empty((F, n), np.int32)
    for t in range(F):                                       # the frame's own component and n - 1 others, in random order
        others = rng.choice(np.delete(np.arange(I), comp[t]), n - 1, replace=False)
        sel[t] = rng.permutation(np.concatenate([[comp[t]], others]))
    l64 = G.loglikes_on(x, (gc, mic, ic), sel)
    wg, wp, _ = G.posteriors(x, (gc, mic, ic), sel, 0.0)
    _, ll, _ = U.softmax_rows(l64)
    # E_t = (2 D + 4) 2^-24 max_slot(|gc| + sum |x_j||mic_j| + 1/2 sum |x_j||S_jk||x_k|)
    ax = np.abs(x).astype(np.float64)
    mag = np.abs(gc.astype(np.float64))[sel] + np.einsum("fd,fnd->fn", ax, np.abs(mic.astype(np.float64))[sel])
    for t in range(F):
        mag[t] += 0.5 * np.einsum("d,nde,e->n", ax[t], np.abs(ic.astype(np.float64))[sel[t]], ax[t])
    E = (2 * D + 4) * EPS32 * mag.max(1)
    m32 = types.SimpleNamespace(gconsts=gc, means_invcovars=mic, inv_covars=ic, numGauss=I)
    p32, l32, _ = U.softmax_rows(U.full_loglikes_on(x, m32, sel, np.float32))
    p64, _, _ = U.softmax_rows(l64)
    return dict(x=frozen(x), sel=frozen(sel), full=(gc, mic, ic), ll=frozen(ll), dense=frozen(dense_posts(wg, wp, I)), E=frozen(E),
                gap_ll=float(np.abs(l32.astype(np.float64) - ll).max()), gap_post=float(np.abs(p32.astype(np.float64) - p64).max()))
