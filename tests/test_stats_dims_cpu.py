"""The builders and oracles of tests/_stats_dims_ref.py, without a GPU: the D list reaches every kernel instance, the integer
cases are exact (the builders assert it; here every builder runs), the pair counts sit where the chunk and item constants put the
splits, and the i-vector oracle is well conditioned at every S."""

import numpy as np
import pytest

import _stats_dims_ref as SD


def test_d_edges_reach_every_instance():
    assert all(1 <= D <= SD.MAX_D for D in SD.D_EDGES) and SD.D_EDGES[-1] == SD.MAX_D
    assert {SD.gacc_nt(D) for D in SD.D_EDGES} == set(range(1, 10))          # gacc_full_kernel<1 .. 9>
    assert {SD.fg_nj(D) for D in SD.D_EDGES} == {1, 2, 3, 4}                   # fg_quad_kernel<1 .. 4>
    assert any(D > 64 for D in SD.D_EDGES)                                     # gacc_diag_kernel's second column, fg gather's second pass
    assert {SD.gamma_group(D)[0] for D in SD.D_EDGES} == {0, 1, 2}
    groups = {SD.gamma_group(D) for D, _ in SD.IVSTATS_CASES}
    assert {(0, 63), (1, 0), (1, 63), (2, 0)} <= groups                        # lane 63 of a group, lane 0 of the next
    assert {fg for fg in map(SD.fg_nj, SD.REAL_DIMS)} == {3, 4}
    # sec_acc_kernel prunes acc[a][c] by 16 a >= D: one block, the 16 / 17 edge, beyond 32, all eight
    assert {(D + 15) // 16 for D in SD.SEC_DIMS} >= {1, 2, 3, 4, 8}


@pytest.mark.parametrize("D", SD.D_EDGES)
def test_integer_cases_are_exact_and_feel_every_dimension(D):
    x, gauss, post, want = SD.acc_case(D)                    # (asserts its exactness precondition)
    assert x.shape == (151, D) and gauss.shape == (151, 3)
    for full in (False, True):
        occ, mean, sec = want[full]
        assert occ[4] == 0 and not mean[4].any() and not sec[4].any()
        assert all(np.array_equal(a, np.round(a * 4) / 4) for a in (occ, mean, sec))
        assert sec[:4, D - 1].any() and mean[:4, D - 1].any()                   # the last dimension carries weight
    assert np.array_equal(want[True][2], np.swapaxes(want[True][2], 1, 2))
    assert np.array_equal(np.einsum("idd->id", want[True][2]), want[False][2])
    x, sel, slot, valid_g, (gc, mic, ic), ll = SD.fgmm_exact_case(D)
    assert np.bincount(valid_g).tolist() == SD.FG_EXACT_COUNTS and len(set(slot.tolist())) == sel.shape[1]
    c = SD.FG_EXACT_COUNTS[1]                                # waves 0, 1 full, wave 2 partial, wave 3 empty
    assert 2 * SD.FG_TILE < c < 3 * SD.FG_TILE
    # a quadratic form without its last row and column, or without the last mean coordinate, gives another log-likelihood
    cut = (gc, mic, ic.copy())
    cut[2][:, D - 1, :] = 0
    cut[2][:, :, D - 1] = 0
    other = SD.G.loglikes_on(x, cut, sel)[np.arange(len(ll)), slot]
    assert ic[:, D - 1, :].any() and not np.array_equal(other.astype(np.float32), ll)


def test_preselect_and_second_order_builders():
    for D, n in SD.PRESELECT_CASES:
        x, sel, slot, model, ll, empty = SD.preselect_case(D, n)
        ok = (sel >= 0) & (sel < model.numGauss)
        assert np.array_equal(ok.sum(1), np.array([0 if t in empty else 1 for t in range(len(ll))]))
        assert all(ll[t] == 0 for t in empty) and sel.shape[1] == n
    assert {n for _, n in SD.PRESELECT_CASES} == {1, SD.MAX_N}
    sizes = set()
    for D in SD.SEC_DIMS:
        for k, counts in enumerate(SD.SEC_LAYOUTS):
            x, gauss, post, want = SD.sec_case(D, k)
            assert np.bincount(gauss[(gauss >= 0) & (gauss < 4)], minlength=4).tolist() == counts
            assert np.array_equal(want, np.swapaxes(want, 1, 2)) and np.array_equal(want, np.round(want * 16) / 16)
            assert all(want[g].any() == (c > 0) for g, c in enumerate(counts))
            sizes |= set(counts)
    assert sizes == {0, 1, SD.SEC_RB, SD.SEC_RB + 1, 40} and 40 > 2 * SD.SEC_RB


def test_ivector_post_cases_cover_the_values_and_hold_ties():
    Ds, Is, ns, Fs = (set(v) for v in zip(*SD.IVPOST_CASES))
    assert Ds == {1, 64, 65, 127, 128} and Is == {1, 40, 255, 256, 257, 513} and ns == {1, 20, 63, 64} and Fs == {31, 32, 33}
    assert any(I < n for _, I, n, _ in SD.IVPOST_CASES) and (SD.MAX_D, 513, SD.MAX_N, 33) in SD.IVPOST_CASES
    across = 0
    for k, (D, I, n, F) in enumerate(SD.IVPOST_CASES):
        x, W, gc, (g, p), info = SD.ivpost_case(k)
        assert W.shape == (2 * D, I) and g.shape == (F, n)
        assert np.all((g >= 0).sum(1) == min(n, I))
        if n < I:
            assert info["ties_at_cut"] >= 1, (k, info)
        across += info["ties_across_tiles"]
        print(f"ivector_post case {dict(zip('DInF', SD.IVPOST_CASES[k]))}: {info}")
        # both halves of W decide: without its last x row (k = D - 1) or its last x^2 row (k = 2 D - 1) the oracle selects other
        # Gaussians or gives other posteriors, and so it does without the whole x^2 half or its upper part (k >= D + D / 2)
        mi, iv = W[:D].T, -2.0 * W[D:].T
        if I > 1:
            for cut_mi, cut_iv in ((D - 1, None), (None, slice(D - 1, D)), (None, slice(0, D)), (None, slice(D // 2, D))):
                m2, v2 = mi.copy(), iv.copy()
                if cut_mi is not None:
                    m2[:, cut_mi] = 0
                if cut_iv is not None:
                    v2[:, cut_iv] = 0
                g2, p2 = SD.R.posteriors(x, (gc, m2, v2), n, 0.0)
                assert not np.array_equal(g2, g) or np.abs(p2 - p).max() > 1e-3, (k, cut_mi, cut_iv)
            assert len(np.unique(iv[:, D - 1])) == 2 and len(np.unique(iv)) == 2
    assert across >= 3
    assert max(SD.ivpost_case(k)[4]["lds"] for k in range(len(SD.IVPOST_CASES))) == SD.ivpost_lds_bytes(SD.MAX_D, SD.MAX_N) > 65536


def test_ivector_statistics_frames_reach_the_runs():
    for k, (D, I) in enumerate(SD.IVSTATS_CASES):
        c = SD.ivstats_case(k)
        runs = [SD.longest_run(row, I) for row in c["gauss"]]
        assert max(r for r, _ in runs) == SD.MAX_N                 # one wave owns all 64 slots of a frame
        assert any(d for _, d in runs)
        assert (c["gauss"] == -1).any() and (c["gauss"] >= I).any()
        assert np.array_equal(c["want"][0][0], np.zeros(c["S"])) and c["want"][0][1:].all()
        assert not np.array_equal(c["want"][0], c["want"][1])      # max_count changes the result
        if I > SD.IVS_WAVES * SD.IVS_BATCH:                         # more than IVS_BATCH distinct Gaussians of one wave in a frame
            assert max(len({g for g in row.tolist() if 0 <= g < I and g % SD.IVS_WAVES == 0}) for row in c["gauss"]) > SD.IVS_BATCH
    assert {I for _, I in SD.IVSTATS_CASES} == {8, 40} and {D for D, I in SD.IVSTATS_CASES if I == 8} == {1, 63, 64, 65, 127, 128}


def test_pair_counts_against_the_chunk_and_item_constants():
    n, F = SD.BUCKET_N, SD.BUCKET_F
    assert 3 * SD.SEC_CH + 5 <= F * n < 3 * SD.SEC_CH + 5 + n and SD.SEC_CH % n != 0      # four chunks; a frame straddles a boundary
    assert SD.BUCKET_I == [1, 257, 8192]
    for I in SD.BUCKET_I:
        g, start, order = SD.bucket_case(I)
        flat = g.reshape(-1)
        ok = (flat >= 0) & (flat < I)
        assert 0.02 < (flat == -1).mean() < 0.05 and 0.02 < (flat >= I).mean() < 0.05
        assert (flat == I // 2).sum() >= 0.45 * flat.size and start[I] == ok.sum() == len(order)
        assert np.all(np.diff(flat[order]) >= 0)
        same = np.diff(flat[order]) == 0
        assert np.all(np.diff(order)[same] > 0)                                            # pair order inside a bucket
        heavy = order[start[I // 2]:start[I // 2 + 1]]
        assert len(set((heavy // SD.SEC_CH).tolist())) == 4                                # its bucket has a share of every chunk
    x, gauss, post, _ = SD.acc_items_case()
    R = SD.ITEM_ROWS
    assert SD.ITEM_COUNTS == [R - 1, R, R + 1, 2 * R, 2 * R + 1, 0] and gauss.size > SD.SEC_CH
    assert SD.ANY_F * SD.ANY_N == 35115 > SD.SEC_CH_ANY and SD.SEC_CH_ANY % SD.ANY_N != 0
    assert SD.ANY_TAIL * SD.ANY_N < SD.SEC_CH_ANY                                          # the shorter call starts inside chunk 0
    x, sel, full, dense = SD.unordered_case()
    assert (sel == 0).sum() == SD.ANY_F > 4 * SD.FG_ROWS and dense.shape == (SD.ANY_F, SD.ANY_I)
    assert np.abs(dense.sum(1) - 1).max() < 1e-12
    assert [I * D for I, D in SD.K_CASES[:3]] == [SD.GKC - 1, SD.GKC, SD.GKC + 1] and SD.K_CASES[3] == (SD.GKC + 1, 1)
    assert SD.K_B == SD.GT + 1


@pytest.mark.parametrize("S", SD.S_EDGES)
def test_oracle_is_well_conditioned_at_every_s(S):
    assert SD.S_EDGES == [1, 31, 32, 33, 64, 65, 1024]
    c = SD.s_case(S)
    scale = np.abs(c["ivectors"]).max()
    rel = np.abs(c["ivectors"] - c["dense"]).max() / scale
    print(f"S = {S}: extract_packed against extract_dense {rel:.3e}")
    assert rel <= 1e-10
    assert np.array_equal(c["ivectors"][0], np.zeros(S)) and c["acc"]["num_ivectors"] == 2


def test_real_valued_cases_have_a_bound_above_the_float32_oracle():
    for D, tied in [(D, tied) for D in SD.REAL_DIMS for tied in (False, True)]:
        c = SD.real_case(D, tied)
        if tied:                                             # several Gaussians share the posterior in most frames
            assert (np.sort(c["dense"], axis=1)[:, -2] > 0.01).mean() > 0.5
        print(f"D = {D}{' tied' if tied else ''}: fp32 oracle gap loglike {c['gap_ll']:.3e}, posteriors {c['gap_post']:.3e}; E_t {c['E'].min():.3e} .. {c['E'].max():.3e}")
        assert c["gap_ll"] > 0 and np.all(c["E"] > 0)
        assert np.abs(c["dense"].sum(1) - 1).max() < 1e-12
    for k in range(len(SD.K_CASES)):
        c = SD.k_case(k)
        assert c["want"].shape == (SD.K_B, SD.K_S) and c["gauss"].max() == c["I"] - 1
