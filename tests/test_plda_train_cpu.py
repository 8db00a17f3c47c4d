"""Back-end training without a GPU: the fp64 oracle (tests/_plda_train_ref.py) against facts that do not come from it -- recovery of
a known PLDA model, EM monotonicity, the PLDA / LDA / PCA invariants --, the Kaldi writers byte for byte against Kaldi-written
goldens and their text round trips, the host side of ktf.training, and the C-ABI's argument checks."""

import ctypes as C
import os

import numpy as np
import pytest

import _plda_train_ref as R
from kaldi_tflite_amd import _lib as L
from kaldi_tflite_amd import io as kio
from kaldi_tflite_amd import training

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def spd(rng, spectrum):
    Q, _ = np.linalg.qr(rng.standard_normal((len(spectrum),) * 2))
    return (Q * spectrum) @ Q.T


def known_model(D=16, S=3000, seed=7):
    rng = np.random.default_rng(seed)
    phi_b = spd(rng, np.geomspace(8.0, 0.5, D))
    phi_w = spd(rng, np.geomspace(2.0, 0.3, D))
    mean = rng.standard_normal(D)
    x, spk = R.sample_plda(rng, D, S, 2, 12, phi_w, phi_b, mean)
    return x, spk, mean, phi_w, phi_b


def implied(T, psi):
    Ti = np.linalg.inv(T)
    return Ti @ Ti.T, Ti @ np.diag(psi) @ Ti.T


# ----------------------------------------------------------------------------- the oracle against the generative model
def test_oracle_recovers_a_known_plda_model():
    x, spk, mean, phi_w, phi_b = known_model()
    m, T, psi = R.compute_plda(x, spk, num_em_iters=10)
    W, B = implied(T, psi)
    # the bounds are the sampling error of 3000 speakers / ~21000 rows in 16 dimensions (measured 0.028 and 0.064; 30 EM
    # iterations give the same to 1e-5: the EM has converged)
    assert rel(W, phi_w) < 0.04, rel(W, phi_w)
    assert rel(B, phi_b) < 0.08, rel(B, phi_b)
    assert np.linalg.norm(m - mean) < 0.1 * np.linalg.norm(mean)


def test_oracle_em_does_not_decrease_the_likelihood():
    x, spk, *_ = known_model(S=600, seed=8)
    hist = []
    stats = R.plda_stats(x, spk)
    R.compute_plda(x, spk, num_em_iters=8, history=hist)
    ll = [R.plda_log_likelihood(x, spk, stats[2], w, b) for w, b in hist]
    for a, b in zip(ll, ll[1:]):
        assert b >= a - 1e-9 * abs(a), ll
    assert ll[-1] > ll[0]


def test_oracle_plda_invariants():
    x, spk, *_ = known_model(S=800, seed=9)
    hist = []
    _, T, psi = R.compute_plda(x, spk, num_em_iters=5, history=hist)
    W, B = hist[-1]
    D = T.shape[0]
    assert np.abs(T @ W @ T.T - np.eye(D)).max() < 1e-10
    assert np.abs(T @ B @ T.T - np.diag(psi)).max() < 1e-10 * psi.max()
    assert np.all(np.diff(psi) <= 0) and np.all(psi >= 0)


@pytest.mark.parametrize("dim", [4, 16])
def test_oracle_lda_invariants(dim):
    x, spk, *_ = known_model(S=500, seed=10)
    out = R.compute_lda(x, spk, dim)
    A, off = out[:, :-1], out[:, -1]
    m, tot, within = R.lda_scatter(x, spk)
    assert np.abs(A @ within @ A.T - np.eye(dim)).max() < 1e-10
    t = A @ tot @ A.T
    assert np.abs(t - np.diag(np.diag(t))).max() < 1e-10 * np.abs(t).max()
    assert np.all(np.diff(np.diag(t)) <= 0)
    assert np.allclose(off, -A @ m, rtol=0, atol=1e-12 * np.abs(A @ m).max())


@pytest.mark.parametrize("normalize_mean", [False, True])
def test_oracle_pca_whitens(normalize_mean):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((4000, 12)) @ spd(rng, np.geomspace(5.0, 0.1, 12)) + 3.0
    t = R.est_pca(x, normalize_mean=normalize_mean, normalize_variance=True)
    y = x @ t[:, :12].T + (t[:, 12] if normalize_mean else 0.0)
    yc = y - y.mean(0)
    assert np.abs(yc.T @ yc / len(y) - np.eye(12)).max() < 1e-10
    if normalize_mean:
        assert np.abs(y.mean(0)).max() < 1e-10


def test_fast_em_form_matches_kaldis_per_count_form():
    """The simultaneous-diagonalisation update of ktf.training is Kaldi's per-count update, restated."""
    x, spk, *_ = known_model(S=300, seed=12)
    mus, n, mbar, O = stats = R.plda_stats(x, spk)
    rng = np.random.default_rng(1)
    D = x.shape[1]
    phi_w, phi_b = spd(rng, np.geomspace(3, 0.5, D)), spd(rng, np.geomspace(9, 0.2, D))
    want_w, want_b = R.em_step(stats, phi_w, phi_b)
    P, Q, lam = training.plda_diagonalize(phi_w, phi_b)
    y = (mus - mbar) @ P.T
    nl = n[:, None] * lam
    a, b = nl / (1 + nl) * y, y / (1 + nl)
    got_b = Q @ (np.diag((lam / (1 + nl)).sum(0)) + a.T @ a) @ Q.T / len(n)
    got_w = (O + Q @ (np.diag((nl / (1 + nl)).sum(0)) + (n[:, None] * b).T @ b) @ Q.T) / n.sum()
    assert rel(got_b, want_b) < 1e-12 and rel(got_w, want_w) < 1e-12


def test_sign_convention():
    V = np.array([[0.6, -0.8], [-0.8, -0.6]])
    A = V @ np.diag([3.0, 1.0]) @ V.T
    w, U = training.eigh_desc(A)
    assert np.allclose(w, [3.0, 1.0])
    assert U[np.argmax(np.abs(U[:, 0])), 0] > 0 and U[np.argmax(np.abs(U[:, 1])), 1] > 0
    _, U2 = R.eigh_desc(A)
    assert np.allclose(U, U2)


# ----------------------------------------------------------------------------- writers
def test_write_plda_reproduces_kaldis_file(tmp_path):
    src = os.path.join(GOLD, "plda.bin")
    p = kio.KaldiPldaReader(src, True)
    out = tmp_path / "plda"
    kio.WriteKaldiPlda(out, p.mean, p.transformMat, p.psi)
    assert out.read_bytes() == open(src, "rb").read()


@pytest.mark.parametrize("name", ["xvectors_train_combined_200k.transform.mat", "xvectors_train_combined_200k.mean.vec"])
def test_write_array_reproduces_kaldis_binary_files(tmp_path, name):
    src = os.path.join(GOLD, name)
    out = tmp_path / name
    kio.WriteKaldiArray(out, kio.ReadKaldiArray(src, True))
    assert out.read_bytes() == open(src, "rb").read()


def test_write_text_vector_reproduces_kaldis_file(tmp_path):
    v = kio.ReadKaldiArray(os.path.join(GOLD, "xvectors_train_combined_200k.mean.vec"), True)
    out = tmp_path / "mean.vec.txt"
    kio.WriteKaldiArray(out, v, binary=False)
    assert out.read_bytes() == open(os.path.join(GOLD, "xvectors_train_combined_200k.mean.vec.txt"), "rb").read()


def test_text_matrix_and_plda_round_trip(tmp_path):
    A = kio.ReadKaldiArray(os.path.join(GOLD, "xvectors_train_combined_200k.transform.mat"), True)
    out = tmp_path / "transform.mat.txt"
    kio.WriteKaldiArray(out, A, binary=False)
    text = out.read_text()
    assert text.startswith(" [\n  ") and text.endswith(" ]\n")
    back = kio.ReadKaldiArray(str(out), False, np.float32)
    assert back.shape == A.shape and np.all(np.abs(back - A) <= 1e-6 * np.abs(A))      # '%.7g': 7 significant digits
    p = kio.KaldiPldaReader(os.path.join(GOLD, "plda.bin"), True)
    out = tmp_path / "plda.txt"
    kio.WriteKaldiPlda(out, p.mean, p.transformMat, p.psi, binary=False)
    text = out.read_text()
    assert text.startswith("<Plda>  [ ") and text.endswith("]\n</Plda> ")
    parts = []
    for i, chunk in enumerate(text.split("]")[:3]):
        f = tmp_path / f"part{i}.txt"
        f.write_text(chunk[chunk.index("["):] + "]\n")
        parts.append(kio.ReadKaldiArray(str(f), False, np.float64))
    for got, want in zip(parts, (p.mean, p.transformMat, p.psi)):
        assert got.shape == want.shape and np.array_equal(got, want)                     # '%.17g': exact
    # fp64 arrays write DV / DM, fp32 arrays FV / FM
    kio.WriteKaldiArray(tmp_path / "d.vec", np.arange(3.0))
    assert (tmp_path / "d.vec").read_bytes()[:5] == b"\0BDV "
    with pytest.raises(ValueError):
        kio.WriteKaldiArray(tmp_path / "bad", np.zeros((2, 2, 2), np.float32))
    with pytest.raises(ValueError):
        kio.WriteKaldiPlda(tmp_path / "bad", np.zeros(3), np.eye(2), np.zeros(3))


# ----------------------------------------------------------------------------- C-ABI
def test_train_abi_argument_validation_without_gpu():
    lib = L.load()
    f = (C.c_float * 64)()
    d = (C.c_double * 64)()
    i = (C.c_int32 * 8)()
    assert lib.ktf_train_workspace_bytes(0, 8) == -1 and "rows" in L.last_error()
    assert lib.ktf_train_workspace_bytes(4, 0) == -1 and "D must be" in L.last_error()
    assert lib.ktf_train_workspace_bytes(4, 1025) == -1 and "D must be" in L.last_error()
    need = lib.ktf_train_workspace_bytes(4, 8)
    assert need > 0
    ws = (C.c_uint8 * need)()

    def means(x=f, N=4, D=8, off=i, S=2, utts=i, n=3, mu=d, cnt=i):
        return lib.ktf_train_class_means(x, N, D, off, S, utts, n, mu, cnt, None)

    for kw, msg in [({"x": None}, "null"), ({"off": None}, "null"), ({"utts": None}, "null"), ({"mu": None}, "null"),
                    ({"cnt": None}, "null"), ({"N": 0}, "bad sizes"), ({"S": 0}, "bad sizes"), ({"n": 0}, "bad sizes"),
                    ({"D": 0}, "D must be"), ({"D": 1025}, "D must be"), ({"S": 1 << 31}, "too many")]:
        assert means(**kw) == -1, kw
        assert msg in L.last_error(), (kw, L.last_error())

    for name, buf in (("ktf_train_mean_f32", f), ("ktf_train_mean_f64", d)):
        fn = getattr(lib, name)

        def mean(y=buf, rows=4, D=8, out=d, w=ws, nb=need):
            return fn(y, rows, D, out, w, nb, None)

        for kw, msg in [({"y": None}, "null"), ({"out": None}, "null"), ({"w": None}, "null"), ({"rows": 0}, "bad sizes"),
                        ({"D": 1025}, "D must be"), ({"nb": need - 1}, "workspace too small")]:
            assert mean(**kw) == -1, (name, kw)
            assert msg in L.last_error(), (name, kw, L.last_error())

    for name, buf in (("ktf_train_gram_f32", f), ("ktf_train_gram_f64", d)):
        fn = getattr(lib, name)

        def gram(y=buf, N=4, D=8, idx=None, rows=4, G=d, w=ws, nb=need):
            return fn(y, N, D, idx, rows, None, None, G, w, nb, None)

        for kw, msg in [({"y": None}, "null"), ({"G": None}, "null"), ({"w": None}, "null"), ({"N": 0}, "bad sizes"),
                        ({"rows": 0}, "bad sizes"), ({"rows": 5}, "bad sizes"), ({"D": 0}, "D must be"),
                        ({"nb": need - 1}, "workspace too small")]:
            assert gram(**kw) == -1, (name, kw)
            assert msg in L.last_error(), (name, kw, L.last_error())

    def proj(mu=d, S=2, D=8, mbar=d, P=d, lam=d, cnt=i, a=d, b=d):
        return lib.ktf_plda_em_project(mu, S, D, mbar, P, lam, cnt, a, b, None)

    for kw, msg in [({"mu": None}, "null"), ({"P": None}, "null"), ({"cnt": None}, "null"), ({"b": None}, "null"),
                    ({"S": 0}, "bad sizes"), ({"D": 1025}, "D must be")]:
        assert proj(**kw) == -1, kw
        assert msg in L.last_error(), (kw, L.last_error())
