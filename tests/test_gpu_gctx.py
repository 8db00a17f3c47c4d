"""Global-context attention on the GPU (include/ktf_gctx.h) against tests/_gctx_ref.py: the logits bit for bit on exact inputs, the
invariances of rule 9, mu / sigma / g within the reference's bounds, random inputs against torch.cat + the TDNN kernels
(e_new <= 2 e_comp + 2^-20 max|ref|, the rule of test_gpu_agg.py) and the layer in the fused runner. Tolerances print their figures."""

import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "kaldi-tflite_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import _lib as L, ops  # noqa: E402
import _attn_ref  # noqa: E402
import _gctx_ref as R  # noqa: E402
from test_gpu_agg import _bits, _rows  # noqa: E402

pytestmark = pytest.mark.gpu
DEV, SENTINEL = "cuda:0", -77.0
MODES = {"f32": L.GEMM_F32, "bf16x3": L.GEMM_BF16X3}
dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)      # noqa: E731


def check_logits(c, lens, mode, pad=0, off=0, only=None):
    """One call (NaN in every unread row and pad column, bases `off` floats off a 256-byte boundary, e full of SENTINEL) against the reference."""
    sl = slice(None) if only is None else slice(only, only + 1)
    x, g, lens = np.array(c["x"][sl]), c["g"][sl], lens[sl]
    (B, T, D), H = x.shape, c["w2"].shape[1]
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    t = {k: _rows(a, a.shape[-1] + pad, off, np.nan)[..., :a.shape[-1]] for k, a in (("x", x), ("g", g), ("w1x", c["w1x"]), ("w2", c["w2"]))}
    te = _rows(np.full((B, T, H), SENTINEL, np.float32), H + pad, off, SENTINEL)
    ops.gctx_logits(t["x"], dev(np.asarray(lens, np.int32)), t["w1x"], t["g"], L.ACT_RELU, t["w2"], dev(c["b2"]), MODES[mode], te[:, :, :H])
    e = te.cpu().numpy()
    assert (e[:, :, H:] == SENTINEL).all()
    for b, n in enumerate(lens):
        ref = R.logits(c["x"][sl][b], n, c["w1x"], g[b], c["w2"], c["b2"], "relu")[1]
        assert np.array_equal(_bits(e[b, :n, :H]), _bits(ref)) and (e[b, n:] == SENTINEL).all(), (b, n)


# every shape with ldx = D + 4 on a 16-byte base; two of them -- at the second every operand has a DMA path and there are two blocks of heads --
# also with ldx = D, D + 3 and one float off (no 16-byte alignment: the scalar feed); the whole batch, then two utterances alone
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("D,A,H,pad,off", [s + (4, 0) for s in R.EXACT_SHAPES] + [s + po for s in ((96, 128, 130), (100, 132, 260)) for po in ((0, 0), (3, 0), (0, 1), (4, 1))])
def test_exact_inputs_give_the_reference_bit_for_bit_whatever_strides_alignment_and_batch(D, A, H, pad, off, mode):
    lens, c = R.exact_case(D, A, H, ops.gctx_row_tile(A, H, MODES[mode]))
    for only in (None, 3, 6):
        check_logits(c, lens, mode, pad, off, only)


@pytest.mark.parametrize("A", [1, 33, 128])
@pytest.mark.parametrize("D", [1, 5, 64, 130])
def test_stats_and_bias_within_the_bounds_of_the_reference(D, A):
    c, lens, eps = R.stats_case(D, A), R.STATS_LENS, 1e-10
    x = c["x"].copy()
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    tx, tl = _rows(x, D + 3, 1, np.nan)[:, :, :D], dev(np.asarray(lens, np.int32))
    ctx = ops.gctx_stats(tx, tl, eps, torch.zeros((len(lens), 2, D), dtype=torch.float64, device=DEV))
    tg = _rows(np.full((len(lens), A), SENTINEL, np.float32), A + 2, 0, SENTINEL)
    ops.gctx_bias(ctx, _rows(c["w1c"], A + 1, 1, np.nan)[:, :A], dev(c["b1"]), tg[:, :A])
    e = ops.gctx_logits(tx, tl, dev(c["w1c"][:D]), tg[:, :A], L.ACT_TANH, dev(np.ones((A, 1), np.float32)), None, L.GEMM_F32,
                        torch.full((len(lens), max(lens), 1), SENTINEL, device=DEV)).cpu().numpy()
    ctx, g = ctx.cpu().numpy(), tg.cpu().numpy()      # an empty utterance: NaN statistics, a NaN row of g and no row of e
    assert np.isnan(ctx[0]).all() and np.isnan(g[0, :A]).all() and (g[:, A:] == SENTINEL).all() and (e[0] == SENTINEL).all()
    for b, n in enumerate(lens[1:], 1):
        r = R.stats(c["x"][b], n, eps)
        gr, S = R.bias(r["mu"], r["sigma"], c["w1c"], c["b1"])
        assert (np.abs(ctx[b] - [r["mu"], r["sigma"]]) <= [r["mu_bound"], r["sigma_bound"]]).all(), (b, n)
        assert (np.abs(g[b, :A] - gr) <= 1.01 * 2.0 ** -24 * np.abs(gr) + 2.0 ** -36 * S + 2.0 ** -149).all(), (b, n)
        assert np.isfinite(e[b, :n]).all() and (e[b, n:] == SENTINEL).all()


def _weights(D, A, H, seed=9):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((3 * D, A)) / np.sqrt(3 * D)).astype(np.float32), (0.1 * rng.standard_normal(A)).astype(np.float32),
            (2.0 * rng.standard_normal((A, H)) / np.sqrt(A)).astype(np.float32), rng.standard_normal(H).astype(np.float32)]


def _composition(rows, refs, w, A, H, tl, gemm):
    """What the parent commit offers: torch.cat([x, mu, sigma]) and the plain layer's attend with the (3 D, A) W1 -> e (B, T, H)."""
    B, T, D = rows.shape
    ctx = dev(np.stack([np.concatenate([r["mu"], r["sigma"]]) for r in refs]).astype(np.float32))
    plain = ktf.layers.AttentiveStatsPooling(A, heads=H, name="composition")
    plain.set_weights(w)
    cat = torch.cat([rows, ctx[:, None, :].expand(B, T, 2 * D)], 2).contiguous()
    return plain.attend(plain.hidden.prepare_input(cat, gemm)[:, :, :3 * D], tl, gemm)


def _check_errors(got, comp, ref, lens, what):
    e_new, e_comp = (max(float(np.abs(a[b, :n] - ref[b]).max()) for b, n in enumerate(lens)) for a in (got, comp))
    top = max(float(np.abs(r).max()) for r in ref)
    print(f"{what}: e_new {e_new:.3e} e_comp {e_comp:.3e} max|ref| {top:.3e}")
    assert e_new <= 2 * e_comp + 2.0 ** -20 * top


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("D,A,H", [(96, 128, 96), (130, 64, 130)])
def test_random_inputs_against_cat_and_the_tdnn_kernels(D, A, H, mode):
    lens, w = [37, ops.gctx_row_tile(A, H, MODES[mode]) + 5], _weights(D, A, H)
    x = np.random.default_rng(8).standard_normal((2, max(lens), D)).astype(np.float32)
    refs = [R.utterance(x[b], n, *w, act="tanh") for b, n in enumerate(lens)]
    layer = ktf.layers.AttentiveStatsPooling(A, heads=H, global_context=True, name="gctx")
    layer.set_weights(w)
    tx, tl = dev(x), dev(np.asarray(lens, np.int32))
    got, comp = layer.attend(tx, tl, MODES[mode]).cpu().numpy(), _composition(tx, refs, w, A, H, tl, MODES[mode]).cpu().numpy()
    _check_errors(got, comp, [r["e"] for r in refs], lens, f"D {D} A {A} H {H} {mode}")


FEAT, WIDE, ATT, HEADS, LENS = 24, 96, 32, 4, (9, 150, 61)
CFG = {"layers": [{"type": "input", "shape": [None, None, FEAT]},
                  {"name": "t1", "type": ["tdnn", "relu", "bn"], "cfg": {"units": 64, "context": [-2, -1, 0, 1, 2]}}, {"name": "t2", "type": ["tdnn", "relu"], "cfg": {"units": WIDE}},
                  {"name": "pool", "type": "attentive_stats_pooling", "cfg": {"attention_units": ATT, "heads": HEADS, "global_context": True}}]}


@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16x3", "f16mx"])
def test_layer_from_yaml_in_the_fused_runner_in_every_mode(mode, monkeypatch):
    mdl = ktf.models.SequentialFromConfig(CFG, None, "gctx", gemm=mode)
    pool, w = mdl.layers[-1], _weights(WIDE, ATT, HEADS, seed=4)
    pool.set_weights(w)
    mdl.min_tiles, mdl.min_frames = {}, {}               # every batch on the mode's own kernels
    assert pool.globalContext and [st[0] for st in mdl._plan()][-1] == "attn"
    x, tl = dev(np.random.default_rng(22).standard_normal((len(LENS), max(LENS), FEAT)).astype(np.float32)), dev(np.asarray(LENS, np.int32))
    seen, plain_pool = [], pool.pool                     # the rows the layer in front wrote (their precision depends on what follows it)
    monkeypatch.setattr(pool, "pool", lambda x, *a, **kw: (seen.append(x.clone()), plain_pool(x, *a, **kw))[1])
    got = mdl.run_ragged(ktf.models._padded_copy(x, torch.float32), tl).float().cpu().numpy().reshape(len(LENS), -1)
    rows = seen[0]
    want = plain_pool(rows, tl, ktf.layers._GEMM[mode])
    assert got.shape == (len(LENS), 2 * WIDE) and np.array_equal(_bits(got), _bits(want.cpu().numpy()))
    if mode == "f32":
        h = rows.cpu().numpy()
        refs = [R.utterance(h[b], n, *w, act="tanh") for b, n in enumerate(LENS)]
        ref = [_attn_ref.forward(h[b], r["e"].astype(np.float32), n)["out"][None] for b, (r, n) in enumerate(zip(refs, LENS))]
        comp = torch.empty_like(want)
        ops.attn_pool(rows, _composition(rows, refs, w, ATT, HEADS, tl, L.GEMM_F32), tl, True, pool.epsilon, comp,
                      torch.empty((len(LENS), HEADS, 2), dtype=torch.float64, device=DEV), None)
        _check_errors(got[:, None], comp.cpu().numpy()[:, None], ref, [1] * len(LENS), "layer f32")
