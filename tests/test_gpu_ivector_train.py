"""GPU half of i-vector extractor training: the accumulated statistics of IvectorExtractor.accumulate_from_posteriors against the
fp64 oracle (_ivector_train_ref) on supplied posteriors, so that no selection can flip, then the EM loop, the writer round trip and
the rejected inputs. Shapes: (a) everything ragged against the 16 x 16 x 4 MFMA tile and an utterance without frames, (b) at least
three chunks and a posterior scale, (c) S = 130 across the Cholesky's 32-column panels and the 128 boundary.

Measured on an MI355X (the largest deviation of any accumulator from the oracle, relative to that array's largest magnitude;
the bound is 1e-8): see INTEGRATION.md §2h."""

import functools

import numpy as np
import pytest
import torch

import _ivector_ref as R
import _ivector_train_ref as T
import kaldi_tflite_amd as ktf
from kaldi_tflite_amd import ops
from kaldi_tflite_amd.io import IvecExtractorModel, KaldiDiagGmmReader, KaldiIvecExtractorReader, WriteKaldiIvecExtractor

pytestmark = pytest.mark.gpu

SHAPES = {"a": dict(I=8, D=5, S=7, lens=[13, 40, 0, 1, 7, 22, 31, 5, 17, 9, 40, 3, 26, 11, 2, 35, 19, 8, 28], n=3, ps=1.0, seed=31),
          "b": dict(I=33, D=24, S=40, lens=[15 + (7 * k) % 21 for k in range(70)], n=4, ps=0.75, seed=32),
          "c": dict(I=5, D=6, S=130, lens=[12, 30, 7, 21, 16, 9, 25, 14, 18], n=2, ps=1.0, seed=33)}
NAMES = ("gamma", "Y", "R", "Ssec", "ivector_sum", "ivector_scatter")


def _ubm(w, mi, iv):
    g = KaldiDiagGmmReader.__new__(KaldiDiagGmmReader)
    g.path, g.binary, g.storedGconsts = None, True, None
    g.weights, g.means_invvars, g.inv_vars = w, mi, iv
    g.numGauss, g.featDim = mi.shape
    g.gconsts = g.computeGconsts()
    return g


@functools.lru_cache(maxsize=None)
def case(name):
    """The model, the batch, the oracle's posteriors, statistics and objective of one shape (computed once, never modified)."""
    c = SHAPES[name]
    rng = np.random.default_rng(c["seed"])
    I, D, S = c["I"], c["D"], c["S"]
    (w, mi, iv), (M, sig) = R.random_models(rng, I, D, S, prior_offset=30.0)
    ubm = _ubm(w, mi, iv)
    utts = []
    for T_u in c["lens"]:
        x = (rng.standard_normal((T_u, D)) * 1.3 + rng.standard_normal(D) * 0.5).astype(np.float32)
        g, p = R.posteriors(x, (ubm.gconsts, mi, iv), c["n"], 0.025) if T_u else (np.zeros((0, c["n"]), np.int32), np.zeros((0, c["n"])))
        utts.append((x, g, p.astype(np.float32)))
    acc = T.accumulate(utts, M, sig, 30.0, posterior_scale=c["ps"])
    objf = T.marginal_objf(utts, M, sig, 30.0, posterior_scale=c["ps"])
    return dict(c, M=M, sig=sig, po=30.0, ubm=ubm, utts=utts, acc=acc, objf=objf)


def batch(utts, D):
    """-> feats (B, T, D), gauss (F, n), post (F, n) on the GPU and the lengths: the arguments of accumulate_from_posteriors."""
    Tm = max(1, max(x.shape[0] for x, _, _ in utts))
    feats = np.zeros((len(utts), Tm, D), np.float32)
    for b, (x, _, _) in enumerate(utts):
        feats[b, :x.shape[0]] = x
    dev = "cuda:0"
    return (torch.as_tensor(feats, device=dev), torch.as_tensor(np.concatenate([g for _, g, _ in utts]), device=dev),
            torch.as_tensor(np.concatenate([p for _, _, p in utts]), device=dev), [x.shape[0] for x, _, _ in utts])


def layer_of(c, model=None, **kw):
    model = IvecExtractorModel(c["M"], c["sig"], c["po"]) if model is None else model
    return model, ktf.layers.IvectorExtractor(model, c["ubm"], num_gselect=c["n"], posterior_scale=c["ps"], **kw)


def run(c, utts=None, **kw):
    model, layer = layer_of(c, **kw)
    st = ktf.training.IvectorStats(model)
    chunks = layer.accumulate_from_posteriors(st, *batch(c["utts"] if utts is None else utts, c["D"]))
    return st, chunks


def limit_for(c, step):
    return step * ops.ivector_train_workspace_bytes(1, c["I"], c["D"], c["S"])


def oracle_arrays(acc):
    return dict(gamma=acc["gamma"], Y=acc["Y"], R=T.pack(acc["R"]), Ssec=acc["Ssec"], ivector_sum=acc["ivector_sum"],
                ivector_scatter=acc["ivector_scatter"])


def worst(h, want):
    return {k: float(np.abs(h[k] - want[k]).max() / np.abs(want[k]).max()) for k in NAMES}


def test_atb_layout_is_exact_on_integers():
    rng = np.random.default_rng(30)
    for M, N, K in ((37, 21, 7), (1, 3, 5), (130, 70, 1), (16, 64, 4), (129, 65, 9)):
        A = rng.integers(-8, 9, (K, M)).astype(np.float64)
        B = rng.integers(-8, 9, (K, N)).astype(np.float64)
        C0 = rng.integers(-8, 9, (M, N)).astype(np.float64)
        got = ops.atb_f64(torch.as_tensor(A, device="cuda:0"), torch.as_tensor(B, device="cuda:0"), torch.as_tensor(C0, device="cuda:0"))
        assert np.array_equal(got.cpu().numpy(), C0 + A.T @ B), (M, N, K)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_statistics_and_objf_match_oracle(name):
    c = case(name)
    kw = dict(workspace_limit=limit_for(c, 30)) if name == "b" else {}
    st, chunks = run(c, **kw)
    if name == "b":
        assert chunks >= 3
    h = st.host()
    dev = worst(h, oracle_arrays(c["acc"]))
    print(f"shape ({name}): chunks {chunks}, worst relative deviations {dev}")
    assert h["num_ivectors"] == c["acc"]["num_ivectors"] == sum(1 for n in c["lens"] if n > 0)
    for k in NAMES:
        assert dev[k] <= 1e-8, (k, dev)
    assert np.array_equal(h["Ssec"], np.swapaxes(h["Ssec"], 1, 2))
    rel = abs(st.objf() - c["objf"]) / abs(c["objf"])
    print(f"shape ({name}): objf {st.objf()} oracle {c['objf']} relative {rel:.3e}")
    assert rel <= 1e-9


@pytest.mark.parametrize("name", ["a", "b"])
def test_run_to_run_bit_identical(name):
    c = case(name)
    kw = dict(workspace_limit=limit_for(c, 30)) if name == "b" else {}
    s1, _ = run(c, **kw)
    s2, _ = run(c, **kw)
    for k in NAMES + ("totals",):
        assert torch.equal(getattr(s1, k), getattr(s2, k)), k


def test_merge_and_skipped_utterance():
    c = case("a")
    whole, _ = run(c)
    h = whole.host()
    s1, _ = run(c, utts=c["utts"][:10])
    s2, _ = run(c, utts=c["utts"][10:])
    m = s1.merge(s2).host()
    assert m["num_ivectors"] == h["num_ivectors"] == 18
    for k in NAMES + ("objf_sum",):
        assert np.abs(np.asarray(m[k]) - np.asarray(h[k])).max() <= 1e-12 * np.abs(np.asarray(h[k])).max(), k
    assert c["lens"][2] == 0
    without, _ = run(c, utts=c["utts"][:2] + c["utts"][3:])
    w = without.host()
    assert w["num_ivectors"] == 18
    for k in NAMES + ("objf_sum",):
        assert np.abs(np.asarray(w[k]) - np.asarray(h[k])).max() <= 1e-12 * np.abs(np.asarray(h[k])).max(), k


def test_extraction_bits_unchanged_by_accumulate():
    c = case("a")
    model, layer = layer_of(c)
    args = batch(c["utts"], c["D"])
    before = layer.from_posteriors(*args, dtype=torch.float64)
    layer.accumulate_from_posteriors(ktf.training.IvectorStats(model), *args)
    after = layer.from_posteriors(*args, dtype=torch.float64)
    assert torch.equal(before, after)
    want = np.stack([R.extract_dense(*R.stats(x, g, p, c["I"], posterior_scale=c["ps"]), c["M"], c["sig"], c["po"]) for x, g, p in c["utts"]])
    assert np.abs(before.cpu().numpy() - want).max() <= 1e-8 * np.abs(want).max()


def test_em_loop_matches_oracle_and_round_trips(tmp_path):
    c = case("b")
    args = batch(c["utts"], c["D"])
    est = dict(variance_floor_factor=1e-8, gaussian_min_count=0.0)
    model = IvecExtractorModel(c["M"], c["sig"], c["po"])
    M, sig, po = c["M"], c["sig"], c["po"]
    objf = []
    for _ in range(3):
        _, layer = layer_of(c, model=model, workspace_limit=limit_for(c, 30))
        st = ktf.training.IvectorStats(model)
        layer.accumulate_from_posteriors(st, *args)
        objf.append(st.objf())
        model = ktf.training.ivector_extractor_est(model, st, **est)
        M, sig, po = T.update(M, sig, T.accumulate(c["utts"], M, sig, po, posterior_scale=c["ps"]), **est)
    _, layer = layer_of(c, model=model)
    st = ktf.training.IvectorStats(model)
    layer.accumulate_from_posteriors(st, *args)
    objf.append(st.objf())
    dM = float(np.abs(np.asarray(model.M) - M).max() / np.abs(M).max())
    dS = float(np.abs(np.asarray(model.sigmaInv) - sig).max() / np.abs(sig).max())
    print(f"objf {objf}; after 3 iterations: M {dM:.3e}, SigmaInv {dS:.3e}, prior offset {model.priorOffset} vs {po}; est {model.estInfo}")
    assert all(b >= a - 1e-12 * abs(a) for a, b in zip(objf, objf[1:])), objf
    assert dM <= 1e-6 and dS <= 1e-6
    path = str(tmp_path / "final.ie")
    WriteKaldiIvecExtractor(path, model)
    _, reread = layer_of(c, model=KaldiIvecExtractorReader(path))
    a = layer.from_posteriors(*args, dtype=torch.float64)
    b = reread.from_posteriors(*args, dtype=torch.float64)
    assert torch.equal(a, b)


def test_rejected_inputs():
    c = case("a")
    model = IvecExtractorModel(c["M"], c["sig"], c["po"])
    args = batch(c["utts"], c["D"])
    st = ktf.training.IvectorStats(model)
    for kw in (dict(acoustic_weight=0.5), dict(max_count=100.0)):
        _, layer = layer_of(c, **kw)
        with pytest.raises(ValueError):
            layer.accumulate_from_posteriors(st, *args)
        with pytest.raises(ValueError):
            layer.accumulate(st, args[0], lengths=args[3])
    _, layer = layer_of(c)
    other = ktf.training.IvectorStats(IvecExtractorModel(c["M"][:, :, :5], c["sig"], c["po"]))
    with pytest.raises(ValueError):
        layer.accumulate_from_posteriors(other, *args)
    assert st.device is None                            # nothing was accumulated by the refused calls
    with pytest.raises(NotImplementedError):
        ktf.training.IvectorStats(IvecExtractorModel(c["M"], c["sig"], c["po"], w=np.ones((c["I"], c["S"]))))
    with pytest.raises(NotImplementedError):
        ktf.layers.IvectorExtractor(IvecExtractorModel(c["M"], c["sig"], c["po"], w=np.ones((c["I"], c["S"]))), c["ubm"])


def test_accumulate_runs_the_posterior_stage():
    """`accumulate` (its own posteriors, diagonal UBM) equals `accumulate_from_posteriors` on what `posteriors` returns, bit for bit."""
    c = case("a")
    model, layer = layer_of(c, min_post=0.025)
    feats, _, _, lens = batch(c["utts"], c["D"])
    g, p, _ = layer.posteriors(feats, lengths=lens)
    s1, s2 = ktf.training.IvectorStats(model), ktf.training.IvectorStats(model)
    layer.accumulate(s1, feats, lengths=lens)
    layer.accumulate_from_posteriors(s2, feats, g, p, lengths=lens)
    for k in NAMES + ("totals",):
        assert torch.equal(getattr(s1, k), getattr(s2, k)), k
    assert s1.host()["num_ivectors"] == 18
