"""The slot rule of the fused pooling (csrc/pooled_stats.h) through its six C-ABI size functions, without a GPU: slots per utterance of up
to T rows and rows per slot for every argument that selects a layout. The expected numbers are written out from the closed forms of
DESIGN.md section 3 ("Fused pooling"): 2 ceil(T / 256), 2 ceil(T / 192), ceil(T / 64) and (T + 254) // 128, with 2, 2, 1, 1 for T <= 0."""

import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "kaldi-tflite_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from kaldi_tflite_amd import _lib as L  # noqa: E402

ROWS = (-1, 0, 1, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 998)
BLOCK128 = (2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 4, 8)
BLOCK96 = (2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 4, 4, 4, 4, 12)
TILE64 = (1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 16)
FLAT128 = (1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 9)

LAYOUTS = {
    "stats_slots": (lambda lib, T: lib.ktf_stats_slots(T), BLOCK128),
    "tdnn_bf16x3": (lambda lib, T: lib.ktf_tdnn_stats_slots(T, L.GEMM_BF16X3), BLOCK128),
    "tdnn_bf16x4": (lambda lib, T: lib.ktf_tdnn_stats_slots(T, L.GEMM_BF16X4), TILE64),
    "mx_tile": (lambda lib, T: lib.ktf_mx_stats_slots(T, 0), BLOCK128),
    "mx_tile_other_flags": (lambda lib, T: lib.ktf_mx_stats_slots(T, L.TDNN_DET_STATS), BLOCK128),
    "mx_loader": (lambda lib, T: lib.ktf_mx_stats_slots(T, L.TDNN_MX_LOADER), BLOCK96),
    "mx_loader_other_flags": (lambda lib, T: lib.ktf_mx_stats_slots(T, L.TDNN_MX_LOADER | L.TDNN_DET_STATS), BLOCK96),
    "flat": (lambda lib, T: lib.ktf_flat_stats_slots(T), FLAT128),
}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_slots_per_utterance(name):
    fn, want = LAYOUTS[name]
    lib = L.load()
    assert len(want) == len(ROWS)
    assert tuple(int(fn(lib, T)) for T in ROWS) == want


def test_rows_per_slot():
    lib = L.load()
    assert int(lib.ktf_tdnn_slot_rows(L.GEMM_BF16X4)) == 64
    assert int(lib.ktf_tdnn_slot_rows(L.GEMM_BF16X3)) == 128
    assert int(lib.ktf_tdnn_slot_rows(L.GEMM_BF16)) == 128
    assert int(lib.ktf_mx_slot_rows(L.TDNN_MX_LOADER)) == 96
    assert int(lib.ktf_mx_slot_rows(L.TDNN_MX_LOADER | L.TDNN_DET_STATS)) == 96
    assert int(lib.ktf_mx_slot_rows(0)) == 128
    assert int(lib.ktf_mx_slot_rows(L.TDNN_DET_STATS)) == 128
