"""Agglomerative clustering (ktf.diarization.agglomerative_cluster, ktf_ahc_*) on the MI355X: labels and counts equal the NumPy
restatement of Kaldi's algorithm (tests/_ahc_ref.py) exactly, in fp32 and fp64, in both modes, across the kernel's internal
switches (expand tiles, wave and workgroup widths, per-slot state in LDS or in the workspace); batching; and scoring + clustering
end to end on synthetic four-speaker recordings."""

import numpy as np
import pytest
import torch

import _ahc_ref as A
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import _lib as L

pytestmark = pytest.mark.gpu
D = ktf.diarization
NP = {torch.float64: np.float64, torch.float32: np.float32}
DEV = "cuda:0"


def block(seed, n, dt, kind="clustered"):
    """Scores of one recording: PLDA-like similarities of rows drawn around a few centroids, or small integers (ties); NaN in
    the lower triangle and on the diagonal for some seeds (never read)."""
    rng = np.random.default_rng(seed)
    if kind == "ties":
        s = rng.integers(-3, 4, (n, n)).astype(dt)
    else:
        k = int(rng.integers(2, 7))
        x = rng.standard_normal((k, 16))[rng.integers(0, k, n)] + rng.standard_normal((n, 16)) * 0.8
        s = (x @ x.T / 16 - 0.5).astype(dt)
    if seed % 3 == 0:
        s[np.tril_indices(n)] = np.nan
    return s


def run(scores_np, dtype, **kw):
    t = torch.as_tensor(scores_np, device=DEV)
    labels, counts = D.agglomerative_cluster(t, **kw)
    assert labels.dtype == torch.int32 and labels.device == t.device and counts.shape == (1,)
    return labels.cpu().numpy(), int(counts.cpu()[0])


def check(s, dtype, **kw):
    got, k = run(s, dtype, **kw)
    want, kw_ = A.ahc_fast(s, **kw)
    assert k == kw_ and np.array_equal(got, want), (s.shape, dtype, kw, k, kw_, np.flatnonzero(got != want)[:10])
    return k


MODES = [{}, {"threshold": -0.2}, {"threshold": 0.3}, {"threshold": 2.0}, {"num_speakers": 4},
         {"num_speakers": 2, "max_spk_fraction": 0.4}, {"num_speakers": 1, "read_costs": True}]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [1, 2, 3, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 400, 1000])
def test_labels_equal_restatement(dtype, n):
    for i, kw in enumerate(MODES):
        check(block(1000 * n + i, n, NP[dtype]), dtype, **kw)
    for i, kw in enumerate(MODES[:5]):
        check(block(7 + 1000 * n + i, n, NP[dtype], "ties"), dtype, **kw)


# 5120 = KTF_AHC_LDS_SLOTS: the largest recording whose per-slot state sits in LDS; 5121 runs from the workspace
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n", [5000, L.AHC_LDS_SLOTS, L.AHC_LDS_SLOTS + 1])
def test_labels_equal_restatement_large(dtype, n):
    assert check(block(n, n, NP[dtype]), dtype, num_speakers=4) == 4
    check(block(n + 1, n, NP[dtype]), dtype, threshold=0.1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_nonfinite_scores(dtype):
    rng = np.random.default_rng(11)
    for n in (5, 40, 300):
        s = block(3 * n, n, NP[dtype])
        k = max(1, n // 8)
        s[rng.integers(0, n, k), rng.integers(0, n, k)] = rng.choice([np.nan, np.inf, -np.inf], k)
        for kw in ({}, {"threshold": 1.0}, {"num_speakers": 3}):
            check(s, dtype, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_batched_equals_separate(dtype):
    ns = [400, 1, 17, 5121, 64, 2, 1000]
    blocks = [block(50 + i, n, NP[dtype]) for i, n in enumerate(ns)]
    spk = [4, 1, 3, 5, 2, 2, 6]
    packed = torch.cat([torch.as_tensor(b.reshape(-1)) for b in blocks]).to(DEV)
    views, o = [], 0
    for n in ns:
        views.append(packed[o:o + n * n].view(n, n))
        o += n * n
    for kw in ({"threshold": 0.2}, {"num_speakers": spk}, {"num_speakers": spk, "max_spk_fraction": 0.6}):
        labels, counts = D.agglomerative_cluster(views, **kw)
        assert len(labels) == len(ns) and counts.shape == (len(ns),)
        base = labels[0].data_ptr()
        assert all(lab.data_ptr() == base + 4 * sum(ns[:r]) for r, lab in enumerate(labels))   # views of one allocation
        counts = counts.cpu().numpy()
        for r, n in enumerate(ns):
            one = dict(kw)
            if "num_speakers" in kw:
                one["num_speakers"] = spk[r]
            want, k = A.ahc_fast(blocks[r], **one)
            assert counts[r] == k and np.array_equal(labels[r].cpu().numpy(), want), (r, n, kw)
        # the same recordings in another order, as non-contiguous blocks (packed with one copy): the same labels
        order = [3, 0, 6, 2, 5, 1, 4]
        loose = []
        for r in order:
            wide = torch.full((ns[r], 2 * ns[r]), float("nan"), dtype=dtype, device=DEV)
            wide[:, :ns[r]] = views[r]
            loose.append(wide[:, :ns[r]])
        assert not loose[0].is_contiguous()
        kw2 = dict(kw)
        if "num_speakers" in kw:
            kw2["num_speakers"] = [spk[r] for r in order]
        labels2, counts2 = D.agglomerative_cluster(loose, **kw2)
        for j, r in enumerate(order):
            assert torch.equal(labels2[j], labels[r]) and int(counts2[j]) == counts[r]


def recording(seed, n, dim):
    """Four speakers with well-separated centroids plus noise, rows length-normalised to sqrt(dim); -> (rows, speaker of row)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    scales = 0.985 ** np.arange(dim)
    cent = rng.standard_normal((4, dim)) * scales * 15.0
    spk = np.concatenate([np.arange(4), rng.integers(0, 4, n - 4)])
    rng.shuffle(spk)
    x = (cent[spk] + rng.standard_normal((n, dim)) * scales) @ q.T
    return x * (np.sqrt(dim) / np.linalg.norm(x, axis=1, keepdims=True)), spk


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_score_dense_then_cluster_finds_the_speakers(dtype):
    dim = 64
    rng = np.random.default_rng(31)
    T = rng.standard_normal((dim, dim)) / np.sqrt(dim) + np.eye(dim)
    layer = ktf.layers.PLDA(dim, rng.standard_normal(dim) * 0.1, T, np.sort(rng.uniform(0.05, 30.0, dim))[::-1].copy(),
                            dtype=dtype)
    recs = [recording(100 + i, n, dim) for i, n in enumerate([60, 200, 33, 120])]
    blocks = layer.score_dense(np.concatenate([x for x, _ in recs]), lengths=[len(x) for x, _ in recs], target_energy=0.1)
    labels, counts = D.agglomerative_cluster(blocks, num_speakers=4)
    assert counts.cpu().tolist() == [4, 4, 4, 4]
    for (x, spk), lab, blk in zip(recs, labels, blocks):
        got = lab.cpu().numpy()
        # the true partition up to relabelling
        assert len({(int(a), int(b)) for a, b in zip(got, spk)}) == 4
        want, k = A.ahc_fast(blk.cpu().numpy(), num_speakers=4)
        assert k == 4 and np.array_equal(got, want)
