"""The shapes of test_gpu_augment_paths.py and test_gpu_resample_paths.py, without a GPU: each one selects the branch of
csrc/augment.hip or csrc/resample.hip it is there for. The helpers of tests/_augment_ref.py and tests/_resample_ref.py restate the
launchers' arithmetic (partition counts, early windows, the spectra's placement, the LDS budget, the `ordered` predicate, a tile's
span); the constants they mirror are read back from the sources here, so a changed AUG_J, KTF_AUG_DIRECT_TAPS, KTF_RS_TILE or LDS
budget fails this module instead of silently moving a GPU test off its branch."""

import os
import re

import numpy as np
import pytest

import _augment_ref as A
import _resample_ref as R
from kaldi_tflite_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ops.aug_partition()
T = ops.rs_tile()


def _source(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _const(text, pattern):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return int(found[0])


def test_mirrored_constants_are_the_sources():
    aug, fft, rs = (_source("kaldi-tflite_amd", "csrc", f) for f in ("augment.hip", "augment_fft.h", "resample.hip"))
    ha, hr = _source("include", "ktf_augment.h"), _source("include", "ktf_resample.h")
    assert _const(aug, r"constexpr int AUG_J = (\d+);") == A.AUG_J
    assert "constexpr int AUG_DIRECT = KTF_AUG_DIRECT_TAPS;" in aug and "if (Lh <= AUG_DIRECT)" in aug
    assert _const(ha, r"#define KTF_AUG_DIRECT_TAPS (\d+)") == A.DIRECT_TAPS
    assert _const(ha, r"#define KTF_AUG_PARTITION (\d+)") == P
    assert _const(fft, r"#define AUG_THREADS (\d+)") == A.AUG_THREADS
    assert "nearbyint(0.001 * (double)fs)" in aug and "nearbyint(0.05 * (double)fs)" in aug
    assert _const(rs, r"constexpr int RS_THREADS = (\d+);") == R.RS_THREADS
    assert (_const(rs, r"constexpr int RS_R = (\d+);"), _const(rs, r"constexpr int RS_J = (\d+);")) == (R.RS_R, R.RS_J)
    assert _const(rs, r"constexpr int RS_LDS_FLOATS = (\d+);") == R.RS_LDS_FLOATS
    assert _const(hr, r"#define KTF_RS_TILE (\d+)") == T
    assert _const(hr, r"#define KTF_RS_MAX_TAPS (\d+)") == R.MAX_TAPS
    assert _const(hr, r"#define KTF_RS_MAX_SPAN (\d+)") == R.MAX_SPAN
    assert _const(hr, r"#define KTF_RS_MAX_TABLE_FLOATS \(1 << (\d+)\)") == 16 and R.MAX_TABLE_FLOATS == 1 << 16


# ----------------------------------------------------------------------------- augmentation
def test_long_rirs_outrun_the_blocks_of_a_workgroup():
    ns, Ls = A.long_shapes(P)
    assert [A.blocks_of(L, P) for L in Ls] == [5, 5, 10, 13] and all(A.conv_path(L) == "transform" for L in Ls)
    beyond = far = edited = 0
    for n in ns:
        for L in Ls:
            groups = A.conv_groups(n, L, P)
            assert groups[0]["pend"] == A.AUG_J < groups[0]["np"]                # every RIR has more partitions than AUG_J
            beyond += sum(g["j0"] >= A.AUG_J and g["np"] > g["j0"] + A.AUG_J for g in groups)
            far += sum(g["slides"] > A.AUG_J - 1 for g in groups)
            edited += sum(g["pend"] != min(g["np"], A.AUG_J) for g in groups)      # where pend = min(np, AUG_J) would stop early
    assert beyond >= 4 and far >= 16 and edited >= 16, (beyond, far, edited)
    # the smallest shape of each kind: one sample against five partitions already has a second workgroup that slides four times
    small = A.conv_groups(ns[0], Ls[0], P)
    assert [(g["j0"], g["pend"], g["slides"]) for g in small] == [(0, 4, 3), (4, 5, 4)]
    assert any(g["j0"] >= A.AUG_J and g["np"] > g["j0"] + A.AUG_J for g in A.conv_groups(ns[0], Ls[2], P))
    # what test_gpu_augment.py's longest RIR (3 P + 5) reaches: no window slides more than AUG_J - 1 times
    for n in (1, P - 1, P, P + 1, 2 * P + 17):
        assert all(g["slides"] <= A.AUG_J - 1 and g["np"] <= A.AUG_J for g in A.conv_groups(n, 3 * P + 5, P))


def _windows(bank, fs):
    """[(L, k, s0, s1)] of a [(L, peak)] bank: the early window only depends on the peak's place."""
    out = []
    for L, k in bank:
        h = np.zeros(L)
        h[k] = 1.0
        assert A.early_window(h, fs)[0] == k
        out.append((L,) + A.early_window(h, fs))
    return out


def test_wide_early_bank_has_three_early_partitions():
    assert [A.early_partitions(fs, P) for fs in (8000, 16000, 44100, 48000)] == [1, 1, 3, 3]
    assert [sum(A.early_taps(fs)) for fs in (16000, 44100, 48000)] == [816, 2249, 2448]
    bank = A.wide_early_bank(P)
    lengths = [L for L, _ in bank]
    assert len(bank) >= 4 and len(set(lengths)) == len(bank) and (3 * P + 5, 100) in bank and (5000, 2500) in bank
    for fs, early in ((48000, [148, 2448, 2448, 49, 64]), (44100, [144, 2249, 2249, 45, 64])):
        win = _windows(bank, fs)
        assert [s1 - s0 for _, _, s0, s1 in win] == early
        assert [A.blocks_of(e, P) for e in early] == [1, 3, 3, 1, 1]
        # (full path, early path) per RIR: the RIR with its peak on the last tap splits, the 64-tap one is all time domain
        paths = [(A.conv_path(L), A.conv_path(s1 - s0)) for L, _, s0, s1 in win]
        assert paths == [("transform", "transform")] * 3 + [("transform", "direct"), ("direct", "direct")]
        assert win[0][3] == win[0][0] and win[3][1] == win[3][0] - 1            # clipped by the RIR's end; the peak on the last tap
        # the early spectra of RIR r > 0 lie npe = 3 partitions apart; with npe = 1 those of RIRs 1 and 2 would overlap
        slots = A.spectra_slots(lengths, fs, P)
        full_end = sum(lengths) // P + len(bank)
        assert all(slots[r][0] + A.blocks_of(lengths[r], P) <= (slots[r + 1][0] if r + 1 < len(bank) else full_end) for r in range(len(bank)))
        assert [e0 - full_end for _, e0 in slots] == [0, 3, 6, 9, 12]
        assert slots[1][1] + A.blocks_of(early[1], P) == slots[2][1] and A.blocks_of(early[1], P) > 1
    # the grid of the early launch: with the whole bank in the batch the early rows end before the full ones (nye < ny); a row
    # alone with a RIR shorter than the window has ny < nye
    for n in A.early_ns(P):
        ny, nye, gx = A.early_grid(n, max(lengths), 48000, P)
        assert nye < ny and gx == -(-nye // A.AUG_J)
    assert A.early_grid(1, 1500, 48000, P)[:2] == (2, 3) and A.early_grid(1, A.DIRECT_TAPS, 48000, P)[:2] == (1, 3)
    # more early blocks than one workgroup owns: the early launch has a second workgroup per row
    assert A.early_grid(2 * P + 17, max(lengths), 48000, P)[1] > A.AUG_J


def test_edge_early_bank_sits_on_the_time_domain_limit():
    win = _windows(A.edge_early_bank(P), 16000)
    D = A.DIRECT_TAPS
    assert [s1 - s0 for _, _, s0, s1 in win] == [D, D + 1, 116, 300, D]
    assert [(A.conv_path(L), A.conv_path(s1 - s0)) for L, _, s0, s1 in win] == \
        [("transform", "direct"), ("transform", "transform"), ("transform", "transform"), ("transform", "transform"), ("direct", "direct")]
    assert all(s1 == L for L, _, _, s1 in win)                                   # every window is cut by the RIR's end
    assert all(L > P for L, *_ in win[:2]) and [(s0, s1 == L) for L, _, s0, s1 in win[3:]] == [(0, True), (0, True)]
    assert A.early_partitions(16000, P) == 1


def test_tie_cases_split_the_maximum_over_lanes_and_waves():
    kinds = set()
    for L, peaks in A.TIE_CASES:
        h = A.rir_with_peaks(np.random.default_rng(L + peaks[0]), L, peaks)
        assert int(np.argmax(h)) == min(peaks) and sorted(np.flatnonzero(h == h.max()).tolist()) == sorted(peaks) and max(peaks) < L
        (t0, w0), (t1, w1) = A.peak_owner(min(peaks)), A.peak_owner(sorted(peaks)[1])
        if t0 == t1:
            kinds.add("one thread")
        elif w0 == w1:
            kinds.add("one wave, lower index in the higher lane" if t0 > t1 else "one wave, lower index in the lower lane")
        else:
            kinds.add("two waves, lower index in the later wave" if w0 > w1 else "two waves, lower index in the earlier wave")
    assert kinds >= {"one thread", "one wave, lower index in the higher lane", "one wave, lower index in the lower lane",
                     "two waves, lower index in the later wave"}
    assert A.peak_owner(300) == (44, 0) and A.peak_owner(45) == (45, 0) and A.peak_owner(70)[1] == 1 and A.peak_owner(260) == (4, 0)


# ----------------------------------------------------------------------------- resampling
def _plan(fi, fo, zeros, cutoff):
    return ops.rs_plan(fi, fo, R.default_cutoff(fi, fo) if cutoff is None else cutoff, zeros)


def _all_tiles(iu, ou, first, taps):
    return [t for n in R.rows_for(iu, ou, T) if n for t in R.tiles_of(-(-n * ou // iu), first, taps, iu, ou, T)]


def test_global_table_plans_exceed_the_lds_budget():
    shapes = {}
    parities = set()
    for fi, fo, zeros, cutoff in R.GLOBAL_TABLE_PLANS:
        iu, ou, first, taps, w = _plan(fi, fo, zeros, cutoff)                   # (ktf_rs_plan_sizes accepted it)
        budget = R.lds_budget(first, taps, iu, ou, T)
        assert budget["floats"] > R.RS_LDS_FLOATS and not budget["wlds"] and not budget["refused"] and R.is_ordered(first, taps, iu)
        assert budget["span_floats"] + T <= R.RS_LDS_FLOATS                     # what the launch asks for without the table
        six = _plan(fi, fo, 6, cutoff)
        assert R.lds_budget(six[2], six[3], iu, ou, T)["wlds"]
        shapes[(fi, fo, zeros)] = (ou, iu, int(taps.max()))
        if iu % 2 == 0:
            for t in _all_tiles(iu, ou, first, taps):
                parities |= t["parities"]
    assert shapes[(44100, 16000, 16)] == (160, 441, 90) and shapes[(48000, 44100, 48)] == (147, 160, 106)
    assert shapes[(8000, 11025, 16)][:2] == (441, 320) and shapes[(44100, 8000, 12)][2] == 134
    assert parities == {0, 1}                                                   # the pair path with and without the single first tap
    assert any(iu % 2 for _, iu, _ in shapes.values())                          # and rs_taps<false>


def test_wide_ou_plans_put_tiles_inside_and_across_units():
    for fi, fo, zeros, cutoff in R.WIDE_OU_PLANS:
        iu, ou, first, taps, w = _plan(fi, fo, zeros, cutoff)
        assert ou == fo // np.gcd(fi, fo) and ou in (441, 1031) and R.lds_budget(first, taps, iu, ou, T)["wlds"]
        tiles = _all_tiles(iu, ou, first, taps)
        inside = [t for t in tiles if t["u_last"] == t["u_first"]]
        across = [t for t in tiles if t["u_last"] > t["u_first"]]
        assert inside and across
        if ou > T:
            # a tile never holds a whole unit: one that straddles two begins at a later phase than it ends on (i0 > i1)
            assert all(t["u_last"] == t["u_first"] + 1 and t["s0"] - t["u_first"] * ou > t["s_end"] - t["u_last"] * ou for t in across)
            assert any(t["s_end"] - t["s0"] == T - 1 for t in inside) and any(t["s_end"] - t["s0"] == T - 1 for t in across)
        else:
            assert 2 * ou < T and any(t["u_last"] - t["u_first"] >= 2 for t in across)
    assert max(fo // np.gcd(fi, fo) for fi, fo, *_ in R.WIDE_OU_PLANS) > T


def test_tap_extremes():
    few = set()
    for fi, fo, zeros, cutoff in R.FEW_TAPS_PLANS:
        iu, ou, first, taps, w = _plan(fi, fo, zeros, cutoff)
        assert cutoff == 0.5 * min(fi, fo) and zeros == 1 and int(taps.max()) <= R.RS_J       # the read-ahead loop runs at most once
        assert int(taps.min()) < R.RS_J
        few |= set(taps.tolist())
        if iu % 2 == 0:
            odd = [t for t in _all_tiles(iu, ou, first, taps) if 1 in t["parities"]]
            assert odd and int(taps.min()) - 1 < R.RS_J                         # one odd tap first, then fewer than RS_J left
    assert few == {2, 3, 4} and {fi // np.gcd(fi, fo) % 2 for fi, fo, *_ in R.FEW_TAPS_PLANS} == {0, 1}
    widest = []
    for fi, fo, zeros, cutoff in R.MOST_TAPS_PLANS:
        iu, ou, first, taps, w = _plan(fi, fo, zeros, cutoff)
        assert R.lds_budget(first, taps, iu, ou, T)["wlds"]
        widest.append(int(taps.max()))
    assert widest == [R.MAX_TAPS - 1, R.MAX_TAPS]
    with pytest.raises(ValueError, match="taps"):
        _plan(48000, 8000, 22, None)                                            # 267: with one phase the count is odd, 255 is its limit
    # the table's copy loop (i += di, j += dj, one carry): all three forms of the step, and a thread that takes more than one
    assert R.table_copy_steps(R.MAX_TAPS - 1, 1)[:2] == (1, 1) and R.table_copy_steps(R.MAX_TAPS, 2) == (1, 0, 2)
    iu, ou, first, taps, w = R.one_tap_plan()
    assert int(taps.max()) == 1 and R.table_copy_steps(1, ou) == (R.RS_THREADS, 0, 2) and ou > R.RS_THREADS and iu % 2 == 0
    budget = R.lds_budget(first, taps, iu, ou, T)
    assert R.is_ordered(first, taps, iu) and budget["wlds"] and not budget["refused"] and first.min() == 0 and first.max() == iu - 1
    assert {p for t in _all_tiles(iu, ou, first, taps) for p in t["parities"]} == {0, 1}


def test_unordered_plan_fails_the_predicate_only():
    iu, ou, first, taps, w = _plan(16000, 17600, 6, None)
    assert (iu, ou) == (10, 11) and R.is_ordered(first, taps, iu)
    phase = ou // 2
    f2, t2, w2 = R.unordered_plan(first, taps, w, phase)
    assert not R.is_ordered(f2, t2, iu) and f2[phase] < f2[phase - 1]
    assert f2[phase] == first[phase] - 3 and t2[phase] == taps[phase] + 3 and not w2[phase, :3].any()
    assert np.array_equal(w2[phase, 3:t2[phase]], w[phase, :taps[phase]])
    keep = np.arange(ou) != phase
    assert np.array_equal(f2[keep], first[keep]) and np.array_equal(t2[keep], taps[keep]) and np.array_equal(w2[keep, :w.shape[1]], w[keep])
    budget = R.lds_budget(f2, t2, iu, ou, T)
    assert budget["wlds"] and not budget["refused"]
    # the same sums: the oracle on both plans agrees to the bit (the added products are exact zeros)
    x = (np.random.default_rng(9).standard_normal(500) * 3000).astype(np.float32)
    m = R.num_out(x.size, 16000, 17600)
    assert np.array_equal(R.resample64(x, first, taps, w, iu, ou, m)[0], R.resample64(x, f2, t2, w2, iu, ou, m)[0])
    # the unordered span covers every phase's reads in every tile, and differs from the span the ordered branch would take
    for t in R.tiles_of(2 * T + 17, f2, t2, iu, ou, T):
        assert t["lo"] == f2.min() + t["u_first"] * iu and t["hi"] == (f2 + t2).max() + t["u_last"] * iu
