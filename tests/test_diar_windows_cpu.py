"""Sliding-window extraction for diarization, host side (no GPU): the window rule against the reference's subsegment names of
librispeech_2.wav, hand-worked boundary cases, the count formula, the RTTM rule (make_rttm.py) and argument validation -- for the
package's helpers and for the NumPy restatement (tests/_diar_ref.py) the GPU tests compare against."""

import os

import numpy as np
import pytest
import torch

import _diar_ref as R
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import models as Mo

D = ktf.diarization
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHIFT = 0.01


def fixture_windows():
    names = open(os.path.join(GOLDEN, "subsegments_librispeech_2.txt")).read().split()
    return [(int(n.split("-")[1]), int(n.split("-")[2])) for n in names]


def test_window_rule_reproduces_the_reference_subsegments():
    want = fixture_windows()
    assert len(want) == 29 and want[0] == (0, 150) and want[-1] == (2100, 2248)
    W, P, M = Mo.window_frames(SHIFT, 1.5, 0.75, 0.5)
    assert (W, P, M) == (150, 75, 50)
    # one segment over the whole recording: unclamped (22.48 s) the names themselves, clamped to the 2246 frames the last end moves
    assert R.window_rule(0, 2248, W, P, M) == want
    assert R.window_rule(0, 2246, W, P, M) == want[:-1] + [(2100, 2246)]
    segs = Mo.caller_segments([[(0.0, 22.48)]], [2246], SHIFT)
    assert segs == [[(0, 2246)]]


@pytest.mark.parametrize("W,P,M", [(150, 75, 50), (150, 150, 0), (10, 3, 4), (1, 1, 0), (7, 2, 0)])
def test_count_formula_matches_the_loop(W, P, M):
    for L in range(1, 400):
        ws = R.window_rule(100, 100 + L, W, P, M)
        assert len(ws) == Mo.window_count(L, W, P, M) == R.window_count(L, W, P, M)
        assert all(1 <= b - a <= W + M for a, b in ws)
        assert ws[0][0] == 100 and ws[-1][1] == 100 + L


def test_window_rule_boundaries():
    """Hand-worked cases, for the restatement and for the package's count (the device tables: tests/test_gpu_diar_windows.py)."""
    W, P, M = 150, 75, 50
    for L, n in ((1, 1), (200, 1), (201, 2), (150, 1), (2246, 29)):
        assert Mo.window_count(L, W, P, M) == n
    for L, n in ((300, 7), (171, 3), (120, 1), (121, 2)):
        assert Mo.window_count(L, 100, 30, 20 if L != 171 else 40) == n
    assert R.window_rule(5, 6, W, P, M) == [(5, 6)]                                     # L = 1
    assert R.window_rule(0, 200, W, P, M) == [(0, 200)]                                 # L = W + M: one window of W + M frames
    assert R.window_rule(0, 201, W, P, M) == [(0, 150), (75, 201)]                      # L = W + M + 1
    assert R.window_rule(0, 150, W, P, M) == [(0, 150)]
    # P does not divide L - W: the remainder joins the last window
    assert R.window_rule(0, 300, 100, 30, 20) == [(0, 100), (30, 130), (60, 160), (90, 190), (120, 220), (150, 250), (180, 300)]
    assert R.window_rule(0, 171, 100, 30, 40) == [(0, 100), (30, 130), (60, 171)]


def test_frame_conversion_and_caller_segments():
    assert Mo.seconds_to_frames(1.5, SHIFT) == 150 and Mo.seconds_to_frames(0.755, SHIFT) == 76 and Mo.seconds_to_frames(0.004, SHIFT) == 0
    segs = Mo.caller_segments([[(0.0, 1.0), (1.0, 2.5), (3.0, 99.0)], []], [500, 10], SHIFT)
    assert segs == [[(0, 100), (100, 250), (300, 500)], []]
    assert segs[0] == R.caller_segments([(0.0, 1.0), (1.0, 2.5), (3.0, 99.0)], 500, SHIFT)


@pytest.mark.parametrize("pairs,why", [
    ([(1.0, 0.5)], "ends before"),
    ([(0.0, 1.0), (0.5, 2.0)], "overlaps"),
    ([(2.0, 3.0), (0.0, 1.0)], "overlaps"),
    ([(0.0, 0.001)], "empty"),
    ([(6.0, 7.0)], "empty"),                          # starts behind the recording's end: empty after the clamp
    ([(0.0,)], "pair"),
    ([(0.0, float("nan"))], "pair"),
])
def test_caller_segments_are_validated(pairs, why):
    with pytest.raises(ValueError, match=why):
        Mo.caller_segments([pairs], [500], SHIFT)
    with pytest.raises(ValueError, match="list of 2"):
        Mo.caller_segments([[(0.0, 1.0)]], [500, 10], SHIFT)


@pytest.mark.parametrize("window,period,min_segment", [
    (0.0, 0.75, 0.5), (-1.0, 0.5, 0.5), (1.5, 0.0, 0.5), (1.5, 2.0, 0.5), (1.5, 0.75, -0.1), (1.5, 0.001, 0.5),
    (float("inf"), 0.75, 0.5), ("1.5", 0.75, 0.5), (True, 0.75, 0.5), (1.5, None, 0.5)])
def test_window_arguments_are_validated(window, period, min_segment):
    with pytest.raises(ValueError):
        Mo.window_frames(SHIFT, window, period, min_segment)


def test_recordings_on_different_devices_are_refused():
    a, b = torch.zeros(4), torch.zeros(4, device="meta")
    with pytest.raises(ValueError, match="one GPU"):
        Mo._one_device([(a[None], 0, 0), (b[None], 0, 1)])
    assert Mo._one_device([(a[None], 0, 0), (a[None], 0, 1)]) == a.device


class _Res:
    def __init__(self, wins, lengths, shift=SHIFT):
        self.windows = torch.as_tensor(np.asarray(wins, np.int32).reshape(-1, 3))
        self.lengths = lengths
        self.frame_shift = shift


def test_rttm_midpoints_merging_gaps_and_format():
    wins = [(0, 0, 150), (0, 75, 225), (0, 150, 300), (0, 400, 550), (0, 475, 600)]
    labels = torch.tensor([1, 1, 2, 2, 2], dtype=torch.int32)
    lines = D.rttm(_Res(wins, [5]), labels, reco_ids=["a"])
    # [0,150) [75,225): boundary 112.5; [112.5,225) [150,300): 187.5; merged 1 = [0, 187.5), 2 = [187.5, 300); gap to 400 kept
    assert lines == ["SPEAKER a 1 0.000 1.875 <NA> <NA> 1 <NA> <NA>",
                     "SPEAKER a 1 1.875 1.125 <NA> <NA> 2 <NA> <NA>",
                     "SPEAKER a 1 4.000 2.000 <NA> <NA> 2 <NA> <NA>"]
    assert R.rttm_pieces([0, 75, 150, 400, 475], [150, 225, 300, 550, 600], [1, 1, 2, 2, 2]) == \
        [(0, 187.5, 1), (187.5, 300, 2), (400, 600, 2)]


def test_rttm_chained_midpoint_and_channel():
    # three windows overlapping in a chain: the middle one's start moves first, then its end
    st, en, lab = [0, 10, 12], [20, 30, 40], [1, 2, 3]
    assert D.rttm_pieces(st, en, lab) == R.rttm_pieces(st, en, lab) == [(0, 15, 1), (15, 21, 2), (21, 40, 3)]
    lines = D.rttm(_Res([(0, a, b) for a, b in zip(st, en)], [3]), [torch.tensor(lab)], channel=2)
    assert lines[1] == "SPEAKER reco0 2 0.150 0.060 <NA> <NA> 2 <NA> <NA>"


def test_rttm_recordings_labels_and_order():
    wins = [(0, 75, 225), (0, 0, 150), (2, 0, 100)]           # recording 1 has no window; recording 0's windows out of order
    lab = [torch.tensor([3, 3]), torch.tensor([1])]
    lines = D.rttm(_Res(wins, [2, 0, 1]), lab, reco_ids=["x", "y", "z"])
    assert lines == ["SPEAKER x 1 0.000 2.250 <NA> <NA> 3 <NA> <NA>", "SPEAKER z 1 0.000 1.000 <NA> <NA> 1 <NA> <NA>"]
    for r in (R.rttm_line("x", 0, 225, 3, SHIFT), R.rttm_line("z", 0, 100, 1, SHIFT)):
        assert r in lines
    with pytest.raises(ValueError):
        D.rttm(_Res(wins, [2, 0, 1]), torch.tensor([1, 2]))
    with pytest.raises(ValueError):
        D.rttm(_Res(wins, [2, 0, 1]), torch.tensor([1, 2, 3]), reco_ids=["a"])


def test_rttm_pieces_random_against_restatement():
    rng = np.random.default_rng(7)
    for _ in range(200):
        n = int(rng.integers(1, 12))
        st = np.sort(rng.integers(0, 500, n))
        en = st + rng.integers(1, 200, n)
        lab = rng.integers(1, 3, n)
        assert D.rttm_pieces(st, en, lab) == [tuple(p) for p in R.rttm_pieces(st, en, lab)]
