"""add-deltas on the MI355X (ktf_add_deltas_f32, ktf.layers.AddDeltas) bit for bit against the NumPy fp32 loop of
tests/_fgmm_ref.py: orders and windows, feature dims, ragged lengths, inputs shorter than the filter, a non-contiguous input."""

import numpy as np
import pytest
import torch

import _fgmm_ref as G
import kaldi_tflite_amd as ktf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("order,window", [(0, 2), (1, 2), (2, 2), (2, 3), (3, 1)])
@pytest.mark.parametrize("D", [1, 23, 60])
def test_bit_exact_with_ragged_lengths(order, window, D):
    rng = np.random.default_rng(order * 100 + window * 10 + D)
    lens = [0, 1, 2, 3, 7, 40, 64]
    x = (rng.standard_normal((len(lens), 64, D)) * 3).astype(np.float32)
    layer = ktf.layers.AddDeltas(order, window)
    got = layer(torch.as_tensor(x, device=DEV), lengths=lens).cpu().numpy()
    want = G.add_deltas(x, lens, order, window)
    assert got.shape == (len(lens), 64, D * (order + 1)) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for b, n in enumerate(lens):
        assert not got[b, n:].any()                                  # rows beyond a length are zero
    full = layer(torch.as_tensor(x, device=DEV)).cpu().numpy()       # no lengths: every row
    assert np.array_equal(full.view(np.uint32), G.add_deltas(x, None, order, window).view(np.uint32))


def test_input_shorter_than_the_filter_and_two_dims():
    rng = np.random.default_rng(1)
    layer = ktf.layers.AddDeltas(2, 3)                               # 13 taps
    for T in (1, 2, 5):
        x = rng.standard_normal((3, T, 20)).astype(np.float32)
        got = layer(torch.as_tensor(x, device=DEV)).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), G.add_deltas(x, None, 2, 3).view(np.uint32))
    x = rng.standard_normal((30, 20)).astype(np.float32)             # (T, D)
    got = layer(torch.as_tensor(x, device=DEV)).cpu().numpy()
    assert got.shape == (30, 60)
    assert np.array_equal(got.view(np.uint32), G.add_deltas(x[None], None, 2, 3)[0].view(np.uint32))
    assert np.array_equal(got[:, :20], x)
    assert layer(torch.zeros((2, 0, 20), device=DEV)).shape == (2, 0, 60)


def test_non_contiguous_input():
    rng = np.random.default_rng(2)
    big = rng.standard_normal((4, 50, 64)).astype(np.float32)
    bd = torch.as_tensor(big, device=DEV)
    layer = ktf.layers.AddDeltas(2, 2)
    for view, ref in ((bd[:, :, 3:27], big[:, :, 3:27]),            # a column slice: row stride 64
                      (bd[::2, 5:45, :24], big[::2, 5:45, :24]),
                      (bd.transpose(1, 2)[:, :40, :], big.transpose(0, 2, 1)[:, :40, :])):   # inner stride != 1
        assert not view.is_contiguous()
        got = layer(view, lengths=[view.shape[1]] * view.shape[0]).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), G.add_deltas(np.ascontiguousarray(ref), None, 2, 2).view(np.uint32))
