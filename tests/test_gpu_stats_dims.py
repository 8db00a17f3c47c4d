"""The GMM, full-covariance and i-vector statistics kernels on the MI355X along the axes that choose their code path (DESIGN.md §7,
"GMM and i-vector kernels: every instance up to feature dim 128"): every gacc_full_kernel<NT> and fg_quad_kernel<NJ> instance, the
second and third column groups of the per-lane kernels, the chunk and item splits of the bucketing, the GEMM's second row tile and
K-chunk edges, and the Cholesky's panel edges. Cases and oracles: tests/_stats_dims_ref.py (tests/test_stats_dims_cpu.py checks
them without a GPU). Where the inputs are small integers the kernel's output must EQUAL the oracle's; the other bounds are the
project's existing ones (1e-8 of an fp64 array's largest magnitude, 1e-9 of the objective, 2e-5 of a posterior) or, for the
real-valued full-covariance frames at D > 64, the derived running-error bound stated at the test."""

import numpy as np
import pytest
import torch

import _stats_dims_ref as SD
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import ops
from kaldi_tflite_amd.io import IvecExtractorModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def d(a):
    return torch.as_tensor(np.array(a), device=DEV)          # a copy: the cached cases are read-only


def strided(x):
    """x (F, D) on the device as the first D columns of a (F, D + 3) buffer whose other columns hold NaN."""
    return d(SD.padded(x))[:, :x.shape[1]]


def zeros64(*shape):
    return torch.zeros(shape, dtype=torch.float64, device=DEV)


def host(*ts):
    out = tuple(t.cpu().numpy() for t in ts)
    return out if len(out) > 1 else out[0]


# ------------------------------------------------------------------ the D axis
def check_acc(x, gauss, post, want, I, full, unselected=None):
    D = x.shape[1]
    xd, gd, pd = strided(x), d(gauss), d(post)
    assert xd.stride(0) == D + 3
    acc = (zeros64(I), zeros64(I, D), zeros64(I, D, D) if full else zeros64(I, D))
    ops.gmm_acc(xd, gd, pd, *acc)
    occ, mean, sec = host(*acc)
    for name, got, w in zip(("occ", "mean_acc", "second_acc"), (occ, mean, sec), want):
        assert np.array_equal(got, w), (name, int((got != w).sum()), float(np.abs(got - w).max()))
    if full:
        assert np.array_equal(sec, np.swapaxes(sec, 1, 2))
    if unselected is not None:
        assert occ[unselected] == 0 and not mean[unselected].any() and not sec[unselected].any()
    ops.gmm_acc(xd, gd, pd, *acc)                            # a second call adds to the accumulators: exactly twice
    for got, w in zip(host(*acc), want):
        assert np.array_equal(got, 2 * w)


@pytest.mark.parametrize("full", [False, True], ids=["diag", "full"])
@pytest.mark.parametrize("D", SD.D_EDGES)
def test_gmm_acc_is_exact_on_integers(D, full):
    x, gauss, post, want = SD.acc_case(D)
    check_acc(x, gauss, post, want[full], 5, full, unselected=4)


@pytest.mark.parametrize("D", SD.D_EDGES)
def test_fgmm_quadratic_form_is_exact_on_integers(D):
    x, sel, slot, valid_g, (gc, mic, ic), want = SD.fgmm_exact_case(D)
    g, p, ll = host(*ops.fgmm_post_ll(strided(x), d(sel), d(mic), d(ic), d(gc), 0.0))
    bad = np.nonzero(ll != want)[0]
    assert bad.size == 0, (bad[:8], ll[bad[:8]], want[bad[:8]], valid_g[bad[:8]])
    assert np.array_equal(g[:, 0], valid_g) and np.all(p[:, 0] == 1.0)
    assert np.all(g[:, 1:] == -1) and np.all(p[:, 1:] == 0.0)


@pytest.mark.parametrize("D,n", SD.PRESELECT_CASES)
def test_preselect_is_exact_on_integers(D, n):
    x, sel, slot, model, want, empty = SD.preselect_case(D, n)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    post, ll = host(*ops.gmm_post_preselect(strided(x), d(sel), d(model.means_invvars), d(model.inv_vars), d(model.gconsts), cnt))
    assert np.array_equal(ll, want), (ll, want)
    F = len(want)
    expect = np.zeros((F, n), np.float32)
    keep = np.array([t not in empty for t in range(F)])
    expect[np.arange(F)[keep], slot[keep]] = 1.0
    assert np.array_equal(post, expect)
    assert int(cnt.item()) == F - len(empty)


@pytest.mark.parametrize("k", range(len(SD.IVPOST_CASES)), ids=[f"D{D}-I{I}-n{n}-F{F}" for D, I, n, F in SD.IVPOST_CASES])
def test_ivector_post_breaks_ties_by_the_lower_index(k):
    D, I, n, F = SD.IVPOST_CASES[k]
    x, W, gc, (wg, wp), info = SD.ivpost_case(k)
    g, p = host(*ops.ivector_post(d(x), d(W), d(gc), n, 0.0))
    assert g.shape == (F, n)
    bad = np.nonzero((g != wg).any(1))[0]
    assert bad.size == 0, (info, bad[:4], g[bad[:2]], wg[bad[:2]])
    err = float(np.abs(p - wp).max())
    print(f"ivector_post (D, I, n, F) = {SD.IVPOST_CASES[k]}: {info}, posterior deviation {err:.3e} (bound 2e-5)")
    assert err <= 2e-5
    assert np.all(p[g == -1] == 0) and np.all((g >= 0).sum(1) == min(n, I))


def run_extract(c, lo, hi, dtype=torch.float64, **scales):
    """ops.ivector_extract on utterances [lo, hi) of a case laid out as _stats_dims_ref lays it out."""
    off = c["off"]
    f0, f1 = int(off[lo]), int(off[hi])
    kw = dict(posterior_scale=1.0, acoustic_weight=1.0, max_count=0.0)
    kw.update(scales)
    return ops.ivector_extract(d(c["x"][f0:f1]), d(off[lo:hi + 1] - f0), d(c["gauss"][f0:f1]), d(c["post"][f0:f1]), kw["posterior_scale"],
                               kw["acoustic_weight"], kw["max_count"], d(c["sim"]), d(c["U"]), c["prior"], dtype)


@pytest.mark.parametrize("k", range(len(SD.IVSTATS_CASES)), ids=[f"D{D}-I{I}" for D, I in SD.IVSTATS_CASES])
def test_ivector_statistics_with_64_slots(k):
    c = dict(SD.ivstats_case(k), prior=SD.IVSTATS_PRIOR)
    I, D, S, B = c["I"], c["D"], c["S"], len(c["lens"])
    for sc, want in zip(SD.IVSTATS_SCALES, c["want"]):
        got = host(run_extract(c, 0, B, **sc))
        err = float(np.abs(got - want).max() / np.abs(want).max())
        print(f"ivector_extract (D, I) = ({D}, {I}), n = 64, max_count {sc['max_count']}: deviation {err:.3e} (bound 1e-8)")
        assert err <= 1e-8
        assert np.array_equal(got[0], np.zeros(S))           # the utterance without frames
    P = S * (S + 1) // 2
    gamma, Y, Rm, isum, iscat, totals = zeros64(I), zeros64(I * D, S), zeros64(I, P), zeros64(S), zeros64(P), zeros64(2)
    ops.ivector_acc_stats(d(c["x"]), d(c["off"]), d(c["gauss"]), d(c["post"]), 1.0, d(c["sim"]), d(c["U"]), c["prior"], gamma, Y, Rm,
                          isum, iscat, totals)
    assert np.array_equal(host(gamma), c["gamma"]), (host(gamma), c["gamma"])
    assert float(totals[0]) == B - 1                         # the empty utterance is not counted
    errs = {k: float(np.abs(got - c[k]).max() / np.abs(c[k]).max()) for k, got in (("Y", host(Y).reshape(I, D, S)), ("ivector_sum", host(isum)))}
    print(f"ivector_acc_stats (D, I) = ({D}, {I}), n = 64: deviations {errs} (bound 1e-8)")
    assert errs["Y"] <= 1e-8 and errs["ivector_sum"] <= 1e-8
    assert all(np.isfinite(host(t)).all() for t in (Rm, iscat, totals))       # (the second-order terms' values: the S test below)


@pytest.mark.parametrize("D", SD.SEC_DIMS)
def test_second_order_statistics_are_exact_on_integers(D):
    for layout, counts in enumerate(SD.SEC_LAYOUTS):
        x, gauss, post, want = SD.sec_case(D, layout)
        Ssec = torch.full((4, D, D), SD.SEC_POISON, dtype=torch.float64, device=DEV)
        ops.ivector_acc_second_order(d(x), d(gauss), d(post), SD.SEC_SCALE, Ssec)
        got = host(Ssec)
        assert np.array_equal(got, want + SD.SEC_POISON), (counts, int((got != want + SD.SEC_POISON).sum()))
        assert np.array_equal(got, np.swapaxes(got, 1, 2))
        assert np.all(got[counts.index(0)] == SD.SEC_POISON)  # the empty bucket's block is untouched


# ------------------------------------------------------------------ the pair-count axis
@pytest.mark.parametrize("I", SD.BUCKET_I)
def test_ordered_scatter_across_chunks(I):
    g, want_start, want_pairs = SD.bucket_case(I)
    start, pairs = host(*ops.vb_bucket(d(g), I))
    assert np.array_equal(start, want_start)
    assert np.array_equal(pairs[:start[I]], want_pairs)


@pytest.mark.parametrize("full", [False, True], ids=["diag", "full"])
def test_gmm_acc_across_chunks_and_item_edges(full):
    x, gauss, post, want = SD.acc_items_case()
    check_acc(x, gauss, post, want[full], 6, full, unselected=5)


def test_unordered_scatter_across_chunks():
    x, sel, (gc, mic, ic), want = SD.unordered_case()
    I = SD.ANY_I
    xd, cons = d(x), (d(mic), d(ic), d(gc))
    g, p = host(*ops.fgmm_post_ll(xd, d(sel), *cons, 0.0, want_loglike=False)[:2])
    got = SD.dense_posts(g, p, I)
    err = float(np.abs(got - want).max())
    print(f"fgmm_post_ll on {sel.size} pairs (unordered scatter, {SD.SEC_CH_ANY} per chunk): posterior deviation {err:.3e} (bound 2e-5)")
    assert err <= 2e-5
    assert np.all(p[g == -1] == 0) and np.all(g < I) and np.isfinite(p).all()
    listed = np.zeros((len(x), I), bool)
    f, s = np.nonzero((sel >= 0) & (sel < I))
    listed[f, sel[f, s]] = True
    assert not (got[~listed] != 0).any()                     # only listed Gaussians are kept ...
    assert np.all(got[want > 1e-30] > 0)                     # ... and every one fp32 does not flush to zero
    # the frames of the second chunk have the bits of a call in which they lie in the first
    t0 = SD.ANY_TAIL
    g2, p2 = host(*ops.fgmm_post_ll(xd[t0:], d(sel[t0:]), *cons, 0.0, want_loglike=False)[:2])
    assert np.array_equal(g2, g[t0:]) and np.array_equal(p2, p[t0:])


# ------------------------------------------------------------------ the S and batch axes
NAMES = ("gamma", "Y", "R", "ivector_sum", "ivector_scatter")


@pytest.mark.parametrize("S", SD.S_EDGES)
def test_extraction_and_statistics_at_the_panel_edges(S):
    c = SD.s_case(S)
    model = IvecExtractorModel(c["M"], c["sig"], SD.S_PRIOR)
    layer = ktf.layers.IvectorExtractor(model, c["ubm"], num_gselect=SD.S_N)
    Tm = max(SD.S_LENS)
    feats = np.zeros((len(SD.S_LENS), Tm, SD.S_D), np.float32)
    for b, (x, _, _) in enumerate(c["utts"]):
        feats[b, :x.shape[0]] = x
    args = (d(feats), d(np.concatenate([g for _, g, _ in c["utts"]])), d(np.concatenate([p for _, _, p in c["utts"]])), SD.S_LENS)
    got = host(layer.from_posteriors(*args, dtype=torch.float64))
    want = c["ivectors"]
    err = float(np.abs(got - want).max() / np.abs(want).max())
    assert np.array_equal(got[0], np.zeros(S))
    st = ktf.training.IvectorStats(model)
    chunks = layer.accumulate_from_posteriors(st, *args)
    h = st.host()
    acc = dict(c["acc"], R=SD.T.pack(c["acc"]["R"]))
    dev = {k: float(np.abs(h[k] - acc[k]).max() / np.abs(acc[k]).max()) for k in NAMES}
    rel = abs(st.objf() - c["objf"]) / abs(c["objf"])
    print(f"S = {S}: i-vectors {err:.3e} (bound 1e-8), statistics {dev} (bound 1e-8), objf {rel:.3e} (bound 1e-9), chunks {chunks}")
    assert err <= 1e-8
    assert h["num_ivectors"] == 2
    for k in NAMES:
        assert dev[k] <= 1e-8, (k, dev)
    assert rel <= 1e-9


@pytest.mark.parametrize("k", range(len(SD.K_CASES)), ids=[f"I{I}-D{D}" for I, D in SD.K_CASES])
def test_65_utterances_in_one_call_and_the_k_chunk_edges(k):
    c = dict(SD.k_case(k), prior=SD.K_PRIOR)
    B = c["B"]
    got = run_extract(c, 0, B)
    err = float(np.abs(host(got) - c["want"]).max() / np.abs(c["want"]).max())
    print(f"ivector_extract B = {B}, (I, D) = ({c['I']}, {c['D']}): deviation {err:.3e} (bound 1e-8)")
    assert err <= 1e-8
    alone = run_extract(c, B - 1, B)                         # utterance 64: the second row tile of the GEMMs
    assert torch.equal(alone[0], got[B - 1])


# ------------------------------------------------------------------ real-valued frames at the new full-covariance instances
@pytest.mark.parametrize("tied", [False, True], ids=["random", "tied"])
@pytest.mark.parametrize("D", SD.REAL_DIMS)
def test_fgmm_real_valued_frames_within_the_running_error_bound(D, tied):
    """No tolerance was ever measured for D > 60, so the bound is derived: a pair's log-likelihood is a sum of 1 + D + D^2 terms
    whose magnitudes add up to A = |gc| + sum |x_j||mic_j| + 1/2 sum |x_j||S_jk||x_k|, taken as D-term dot products (D roundings
    each) inside a D-term dot product and two more additions: at most (2 D + 4) roundings on any path, each below 2^-24 A. With
    E_t the largest such bound over the frame's slots, |loglike - oracle| <= E_t + 4 2^-24 |oracle| (max, exp, log, the sum) and
    |post - oracle| <= 2 E_t + 4 2^-24 (a posterior moves by at most twice the shift of the log-likelihoods). `tied`: the same
    frames' model with one shared covariance and close means, where several listed Gaussians share the posterior."""
    c = SD.real_case(D, tied)
    gc, mic, ic = c["full"]
    g, p, ll = host(*ops.fgmm_post_ll(d(c["x"]), d(c["sel"]), d(mic), d(ic), d(gc), 0.0))
    got = SD.dense_posts(g, p, SD.REAL_I)
    dl = np.abs(ll - c["ll"])
    dp = np.abs(got - c["dense"]).max(1)
    bl = c["E"] + 4 * SD.EPS32 * np.abs(c["ll"])
    bp = 2 * c["E"] + 4 * SD.EPS32
    print(f"fgmm_post_ll D = {D}{' tied' if tied else ''}: loglike deviation {dl.max():.3e} ({dl.max() / c['gap_ll']:.2f} x the fp32 oracle's {c['gap_ll']:.3e}; "
          f"{(dl / bl).max():.4f} of the bound), posterior deviation {dp.max():.3e} (fp32 oracle {c['gap_post']:.3e}; "
          f"{(dp / bp).max():.2e} of the bound)")
    assert np.all(dl <= bl)
    assert np.all(dp <= bp)
