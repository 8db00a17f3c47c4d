"""Attentive statistics pooling on the GPU: ktf_attn_pool / ktf_attn_pool_backward against the fp64 restatement of
tests/_attn_ref.py (bounds: its docstring; test_attn_cpu.py checks what they assume of the inputs used here), the bit-level
invariances of rules 8 and 9, the layer in a Sequential and an XvectorExtractor in every gemm mode, and training through
ktf.autograd.attentive_stats_pooling and TrainableSequential. Every comparison prints worst |err| / bound; the limit is 1."""

import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "kaldi-tflite_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import ops  # noqa: E402
import _attn_ref as R  # noqa: E402
import _pool_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
F64 = torch.float64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows(a, ld, off, fill=NAN):
    """a (B, T, C) fp32 as a device tensor (B, T, ld) whose base lies `off` floats behind a 256-byte boundary; pad columns = fill."""
    B, T, C = a.shape
    buf = torch.full((B * T * ld + 8,), fill, dtype=torch.float32, device=DEV)
    v = buf[off:off + B * T * ld].view(B, T, ld)
    assert v.data_ptr() % 16 == 4 * off
    v[:, :, :C] = torch.as_tensor(a, device=DEV)
    return v


def run(x, e, lens, include_std=True, gout=None, ldx=None, lde=None, off=0, eps=R.EPS, poison=True):
    """The forward and (with gout) the backward call on copies of x (B, T, D) / e (B, T, H) with row strides ldx / lde, NaN in every
    row from the utterance's length on and in every pad column -> numpy out (B, D or 2 D), norm, stats, dx (B, T, ldx), de (B, T, lde)."""
    B, T, D = x.shape
    H = e.shape[2]
    ldx, lde = ldx or D, lde or H
    x, e = np.array(x, np.float32), np.array(e, np.float32)
    if poison and lens is not None:
        for b in range(B):
            n = R.clamp_len(lens[b], T)
            x[b, n:], e[b, n:] = NAN, NAN
    tx, te = _rows(x, ldx, off), _rows(e, lde, off)
    tl = None if lens is None else torch.as_tensor(np.asarray(lens, np.int32), device=DEV)
    od = 2 * D if include_std else D
    out = torch.full((B, od + 1), 7.0, device=DEV)
    norm = torch.empty((B, H, 2), dtype=F64, device=DEV)
    stats = torch.empty((B, 2, D), dtype=F64, device=DEV)
    ops.attn_pool(tx, te, tl, include_std, eps, out, norm, stats, D=D, H=H)
    res = dict(out=out[:, :od].cpu().numpy(), norm=norm.cpu().numpy(), stats=stats.cpu().numpy())
    assert (out[:, od] == 7.0).all()                               # rule 7
    if gout is not None:
        tg = torch.as_tensor(np.array(np.asarray(gout, np.float32)[:, :od]), device=DEV)
        dx = torch.full((B, T, ldx), NAN, device=DEV)
        de = torch.full((B, T, lde), NAN, device=DEV)
        ws = ops.attn_pool_backward_workspace(B, D, H, DEV)
        ops.attn_pool_backward(tx, te, tl, include_std, eps, norm, stats, tg, dx, de, ws, D=D, H=H)
        res.update(dx=dx.cpu().numpy(), de=de.cpu().numpy())
    return res


def check_zero_fill(res, lens, D, H):
    """Rule 12: rows from the length on and the pad columns of dx and de are zero."""
    B, T = res["dx"].shape[:2]
    for b in range(B):
        n = R.clamp_len(None if lens is None else lens[b], T)
        assert not res["dx"][b, n:].any() and not res["de"][b, n:].any(), b
    assert not res["dx"][:, :, D:].any() and not res["de"][:, :, H:].any()
    assert not np.isnan(res["dx"]).any() and not np.isnan(res["de"]).any()


@functools.lru_cache(maxsize=None)
def reference(D, H, include_std, with_lens, const_channel=None):
    x, e, lens, gout = R.kernel_case(D, H, with_lens, const_channel)
    ref = R.pool(x, e, lens, include_std, R.EPS, gout)
    for a in (x, e, gout):
        a.setflags(write=False)
    return x, e, lens, gout, ref


def compare(tag, res, ref, D, H):
    ratios = dict(out=R.ratio(res["out"], ref["out"], ref["out_bound"]),
                  dx=R.ratio(res["dx"][:, :, :D], ref["dx"], ref["dx_bound"]),
                  de=R.ratio(res["de"][:, :, :H], ref["de"], ref["de_bound"]))
    print(f"{tag}: worst |err| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (tag, ratios)
    return ratios


# ----------------------------------------------------------------------------- the kernels against the restatement
@pytest.mark.parametrize("with_lens", [True, False], ids=["lens", "nolens"])
@pytest.mark.parametrize("include_std", [True, False], ids=["std", "mean"])
@pytest.mark.parametrize("D,H", R.DIMS)
def test_kernels_match_the_restatement(D, H, include_std, with_lens):
    x, e, lens, gout, ref = reference(D, H, include_std, with_lens)
    res = run(x, e, lens, include_std, gout)
    check_zero_fill(res, lens, D, H)
    compare(f"attn D={D} H={H} std={int(include_std)} lens={int(with_lens)}", res, ref, D, H)
    for b, f in enumerate(ref["fwd"]):                            # rule 11
        if f["n"]:
            assert np.array_equal(res["norm"][b, :, 0], f["m"])
            assert np.abs(res["norm"][b, :, 1] - f["Z"]).max() <= 2.0 ** -40 * f["Z"].max()
            assert np.abs(res["stats"][b, 0] - f["mu"]).max() <= 2.0 ** -36 * f["mu_abs"].max()
    if with_lens:                                                 # rule 10: what ktf_stats_pool writes for an utterance without a row
        empty = [b for b, n in enumerate(lens) if n == 0]
        assert empty
        sp = torch.zeros((len(lens), 2 * D if include_std else D), device=DEV)
        ops.stats_pool(torch.as_tensor(x, device=DEV), D, torch.as_tensor(lens, device=DEV), 1, include_std, R.EPS, sp)
        assert np.array_equal(_bits(res["out"][empty]), _bits(sp.cpu().numpy()[empty]))


@pytest.mark.parametrize("D,H", R.STRIDE_DIMS)
def test_strides_and_alignment_do_not_change_a_bit(D, H):
    x, e, lens, gout = R.stride_case(D, H)
    base = run(x, e, lens, True, gout, poison=False)
    ref = R.pool(x, e, lens, True, R.EPS, gout)
    compare(f"strides D={D} H={H}", base, ref, D, H)
    for ldx in (D, D + 3, D + 4):
        for lde in (H, H + 1):
            for off in (0, 1):
                res = run(x, e, lens, True, gout, ldx=ldx, lde=lde, off=off)
                check_zero_fill(res, lens, D, H)
                for k in ("out", "dx", "de"):
                    got = res[k] if k == "out" else res[k][:, :, :(D if k == "dx" else H)]
                    assert np.array_equal(_bits(got), _bits(base[k])), (k, ldx, lde, off)


@pytest.mark.parametrize("D,H,B,lens", R.INVARIANCE_CASES)
def test_bits_do_not_depend_on_batch_position_width_or_launch_shape(D, H, B, lens):
    """The batch runs the throughput shapes (for the first two cases), an utterance alone the few-utterances ones."""
    T = max(lens) + 1
    x, e, lens_b, gout = R.invariance_case(D, H, B, lens)
    lens_b = [int(n) for n in lens_b]
    base = run(x, e, lens_b, True, gout)
    again = run(x, e, lens_b, True, gout)
    perm = np.random.default_rng(3).permutation(B)
    shuffled = run(x[perm], e[perm], [lens_b[i] for i in perm], True, gout[perm])
    for k in ("out", "dx", "de"):
        assert np.array_equal(_bits(base[k]), _bits(again[k])), k
        assert np.array_equal(_bits(base[k][perm]), _bits(shuffled[k])), k
    for b in range(len(lens)):
        n = lens_b[b]
        wide_x, wide_e = np.full((1, T + 37, D), NAN, np.float32), np.full((1, T + 37, H), NAN, np.float32)
        wide_x[0, :T], wide_e[0, :T] = x[b], e[b]
        for xs, es in ((x[b:b + 1], e[b:b + 1]), (wide_x, wide_e)):
            one = run(xs, es, [n], True, gout[b:b + 1])
            assert np.array_equal(_bits(one["out"][0]), _bits(base["out"][b])), (b, n)
            assert np.array_equal(_bits(one["dx"][0, :T]), _bits(base["dx"][b])), (b, n)
            assert np.array_equal(_bits(one["de"][0, :T]), _bits(base["de"][b])), (b, n)
            assert not one["dx"][0, T:].any() and not one["de"][0, T:].any()


@pytest.mark.parametrize("D,H", R.SHIFT_DIMS)
def test_a_shift_of_the_logits_per_head_changes_no_bit(D, H):
    x, e, shifted, lens, gout = R.shift_case(D, H)
    a, b = run(x, e, lens, True, gout), run(x, shifted, lens, True, gout)
    for k in ("out", "dx", "de"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    ref = R.pool(x, e, lens, True, R.EPS, gout)
    compare(f"shift D={D} H={H}", b, ref, D, H)


def test_one_dominant_logit_selects_its_row():
    D, H, T, row = R.DOMINANT
    x, e = R.dominant_case()
    res = run(x, e, None, True)
    assert np.array_equal(_bits(res["out"][0, :D]), _bits(x[0, row]))
    f = R.forward(x[0], e[0], T)
    root = np.sqrt(np.float64(np.float32(R.EPS)))
    r = R.ratio(res["out"][0, D:], np.full(D, root), f["out_bound"][D:])
    print(f"dominant logit: worst |std - sqrt(eps)| / bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("D,H", R.CONST_LOGIT_DIMS)
def test_constant_logits_give_the_plain_statistics(D, H):
    x, e, lens = R.const_logit_case(D, H)
    res = run(x, e, lens, True)
    sp = torch.zeros((4, 2 * D), device=DEV)
    ops.stats_pool(torch.as_tensor(x, device=DEV), D, torch.as_tensor(np.asarray(lens, np.int32), device=DEV), 1, True, R.EPS, sp)
    ref = R.pool(x, e, lens)
    _, pb = P.pool(x, lens)
    r = R.ratio(res["out"], sp.cpu().numpy(), ref["out_bound"] + pb)
    print(f"constant logits D={D} H={H}: worst |attn - stats_pool| / bound {r:.3f}")
    assert r <= 1.0


def test_a_constant_channel_and_a_zero_gradient():
    D, H = 30, 5
    x, e, lens, gout, ref = reference(D, H, True, True, 7)
    res = run(x, e, lens, True, gout)
    check_zero_fill(res, lens, D, H)
    compare("constant channel", res, ref, D, H)
    zero = run(x, e, lens, True, np.zeros_like(gout))
    assert not zero["dx"].any() and not zero["de"].any()
    assert np.array_equal(_bits(zero["out"]), _bits(res["out"]))


# ----------------------------------------------------------------------------- the layer in a Sequential and an XvectorExtractor
# max |got - want| <= limit * max(1, max |want|) per gemm mode: the limits test_gpu_parity.py holds the same modes to
# (test_tdnn_options_vs_oracle; "bf16": test_extractor_reduced_precision_modes)
MODE_LIMITS = {"f32": 2e-5, "bf16x3": 2e-4, "bf16": 5e-2, "f16mx": 2e-3}
FEAT, WIDE, POOLED, ATT, HEADS, EMB = 24, 192, 160, 32, 4, 48
RUN_LENS = (1, 65, 300)


def _model_cfg(pooling):
    layers = [{"name": "input", "type": "input", "shape": [None, None, FEAT]},
              {"name": "tdnn1", "type": ["tdnn", "relu", "batchnorm"], "cfg": {"units": WIDE, "context": [-2, 0, 2]}},
              {"name": "tdnn2", "type": ["tdnn", "relu", "batchnorm"], "cfg": {"units": POOLED, "context": [-1, 0, 1]}}]
    if pooling == "attentive":
        layers.append({"name": "pool", "type": "attentive_stats_pooling", "cfg": {"attention_units": ATT, "heads": HEADS}})
    else:
        layers.append({"name": "pool", "type": "stats_pooling", "cfg": {"left_context": 0, "right_context": 10000, "reduce_time_axis": True}})
    layers.append({"name": "embed", "type": "tdnn", "cfg": {"units": EMB, "context": [0]}})
    return {"type": "sequential", "layers": layers}


def _model_weights(seed=11, zero_w2=False):
    rng = np.random.default_rng(seed)
    w, din = {}, FEAT
    for name, U, K in (("tdnn1", WIDE, 3), ("tdnn2", POOLED, 3)):
        w[f"{name}.affine"] = [(rng.standard_normal((U, K * din)) / np.sqrt(K * din)).astype(np.float32), (0.1 * rng.standard_normal(U)).astype(np.float32)]
        w[f"{name}.batchnorm"] = [np.float32(1.0), rng.uniform(0.2, 1.0, U).astype(np.float32), rng.uniform(0.5, 2.0, U).astype(np.float32)]
        din = U
    # logits of unit-order spread: the hidden units are O(1) behind tanh, W2 ~ N(0, 4 / A)
    w["pool"] = [(rng.standard_normal((POOLED, ATT)) / np.sqrt(POOLED)).astype(np.float32), (0.1 * rng.standard_normal(ATT)).astype(np.float32),
                 (0.0 if zero_w2 else 2.0) * (rng.standard_normal((ATT, HEADS)) / np.sqrt(ATT)).astype(np.float32),
                 rng.standard_normal(HEADS).astype(np.float32)]
    w["embed.affine"] = [(rng.standard_normal((EMB, 2 * POOLED)) / np.sqrt(2 * POOLED)).astype(np.float32), (0.1 * rng.standard_normal(EMB)).astype(np.float32)]
    return w


def _build(pooling, w, gemm):
    mdl = ktf.models.SequentialFromConfig(_model_cfg(pooling), None, "attentive", gemm=gemm)
    for layer in mdl.layers:
        if layer.name in w and not (pooling != "attentive" and layer.name == "pool"):
            layer.set_weights(list(w[layer.name]))
    mdl.min_tiles, mdl.min_frames = {}, {}               # every batch on the mode's own kernels
    return mdl


def _run(mdl, x, lens):
    tx = ktf.models._padded_copy(torch.as_tensor(x, device=DEV), torch.float32)
    tl = torch.as_tensor(np.asarray(lens, np.int32), device=DEV)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return mdl.run_ragged(tx, tl).float().cpu().numpy().reshape(len(lens), -1)


@functools.lru_cache(maxsize=None)
def _composition(zero_w2=False):
    """The input, the weights and the fp64 composition of public pieces: the stack up to the pooling in "f32", the logits, the pooling
    (_attn_ref) and the tail affine in fp64."""
    w = _model_weights(zero_w2=zero_w2)
    x = np.random.default_rng(12).standard_normal((len(RUN_LENS), max(RUN_LENS), FEAT)).astype(np.float32)
    full = _build("attentive", w, "f32")
    front = ktf.models.Sequential([ktf.models.Input(shape=(None, FEAT))] + full.layers[:6], gemm="f32")
    tx = ktf.models._padded_copy(torch.as_tensor(x, device=DEV), torch.float32)
    h = front.run_ragged(tx, torch.as_tensor(np.asarray(RUN_LENS, np.int32), device=DEV)).cpu().numpy().astype(np.float64)
    w1, b1, w2, b2 = (a.astype(np.float64) for a in w["pool"])
    e = np.tanh(h @ w1 + b1) @ w2 + b2
    spread = max(float(np.ptp(e[b, :n], axis=0).max()) for b, n in enumerate(RUN_LENS) if n > 1)
    pooled = R.pool(h.astype(np.float32), e.astype(np.float32), RUN_LENS)["out"]       # (the rows are fp32 already; e to fp32 as the layer holds it)
    We, be = (a.astype(np.float64) for a in w["embed.affine"])
    return x, w, pooled @ We.T + be, spread


@pytest.mark.parametrize("gemm", ["f32", "bf16x3", "bf16", "f16mx"])
def test_sequential_with_the_layer_in_every_mode(gemm):
    x, w, want, spread = _composition()
    got = _run(_build("attentive", w, gemm), x, RUN_LENS)
    err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
    print(f"attentive model {gemm}: max |got - fp64 composition| / max(1, |want|) = {err:.3e} = {err / MODE_LIMITS[gemm]:.3f} of the "
          f"mode's limit {MODE_LIMITS[gemm]:g} (logit spread {spread:.2f})")
    assert spread > 1.0
    assert err <= MODE_LIMITS[gemm]


def test_zero_attention_weights_give_the_stats_pooling_model():
    x, w, want, _ = _composition(zero_w2=True)
    got = _run(_build("attentive", w, "f32"), x, RUN_LENS)
    plain = _run(_build("stats", w, "f32"), x, RUN_LENS)
    scale = max(1.0, np.abs(want).max())
    print(f"W2 = 0: max |attentive - StatsPooling model| / scale = {np.abs(got - plain).max() / scale:.3e}")
    assert np.abs(got - plain).max() <= MODE_LIMITS["f32"] * scale
    assert np.abs(got - want).max() <= MODE_LIMITS["f32"] * scale


def test_extractor_with_the_layer_batch_equals_single_and_the_fused_tail():
    import synth
    cfg = synth.extractor_cfg()
    mc = synth.model_config(narrow=True, out_dim=64)
    at = [i for i, l in enumerate(mc["layers"]) if l["name"] == "stats"][0]
    mc["layers"][at] = {"name": "stats", "type": "attentive_stats", "cfg": {"attention_units": 32, "heads": 4}}
    w = synth.make_weights(seed=77, narrow=True, out_dim=64)
    rng = np.random.default_rng(78)
    w["stats"] = ((rng.standard_normal((96, 32)) / np.sqrt(96)).astype(np.float32), (0.1 * rng.standard_normal(32)).astype(np.float32),
                  (2 * rng.standard_normal((32, 4)) / np.sqrt(32)).astype(np.float32), rng.standard_normal(4).astype(np.float32))
    seq = ktf.models.SequentialFromConfig(mc, None, "cmvn2xvec", gemm="f32")
    for layer in seq.layers:
        if layer.name in w:
            layer.set_weights(list(w[layer.name]))
    mdl = ktf.models.XvectorExtractor.from_parts(cfg, seq, w["mean"], w["lda"])
    assert mdl._tail_fusable()
    wav = torch.as_tensor(np.concatenate([synth.make_wav(2, 48000, seed=21), synth.make_wav(3, 48000, seed=22, ragged=True)], 0), device=DEV)
    fused = mdl(wav)
    assert torch.equal(mdl(wav), fused), "not reproducible"
    for b in (0, 4):
        assert torch.equal(mdl(wav[b:b + 1]).reshape(-1), fused[b]), "batch != single"
    mdl.fuse_tail = False
    plain = mdl(wav)
    for b in (0, 4):
        assert torch.equal(mdl(wav[b:b + 1]).reshape(-1), plain[b]), "batch != single (three-launch tail)"
    d = (fused - plain).abs().max().item()
    print(f"extractor: max |fused tail - three-launch tail| = {d:.3e}")
    assert d <= 1e-5                                   # (fp32 summation order of the tail's dot products: test_gpu_mx.py's limit)
    assert bool(torch.isfinite(fused).all()) and not torch.equal(fused[0], fused[1])


# ----------------------------------------------------------------------------- training
TRAIN_LENS = [40, 90, 57, 64, 65, 71]
CLASSES = 3


def _restated_bn(x, lens, gamma, eps):
    rows = torch.cat([x[b, :n] for b, n in enumerate(lens)])
    mean, var = rows.mean(0), rows.var(0, unbiased=False)
    mask = (torch.arange(x.shape[1])[None, :] < torch.tensor(lens)[:, None]).unsqueeze(-1)
    return torch.where(mask, gamma * (x - mean) / torch.sqrt(var + eps), torch.zeros((), dtype=x.dtype))


def _restated_net(seq, params, feats, lens, keep=None):
    """The attentive network in fp64 torch ops: restated_tdnn / torch_pool of the CPU tests. `keep`: a dict that receives the logits
    (their gradient retained)."""
    from test_attn_cpu import torch_pool
    from test_tdnn_grad_cpu import restated_tdnn
    x, it, pooled = feats, iter(params), False
    for l in seq.layers:
        if isinstance(l, ktf.layers.TDNN):
            w, b = next(it), next(it)
            x = x @ w[:, 0, :].T + b if pooled else restated_tdnn(x, w, b, lens, list(l.context), 1, "SAME")
        elif isinstance(l, ktf.layers.ReLU):
            x = torch.relu(x)
        elif isinstance(l, ktf.layers.BatchNorm):
            x = _restated_bn(x, lens, next(it), l.epsilon)
        else:
            w1, b1, w2, b2 = next(it), next(it), next(it), next(it)
            e = torch.tanh(x @ w1[:, 0, :].T + b1) @ w2[:, 0, :].T + b2
            if keep is not None:
                e.retain_grad()
                keep["e"] = e
            x, pooled = torch.stack([torch_pool(x[b], e[b], n, l.includeStd, l.epsilon) for b, n in enumerate(lens)]), True
    return x


@pytest.mark.parametrize("D,H", R.AUTOGRAD_DIMS)
def test_autograd_function_is_the_kernels(D, H):
    """ktf.autograd.attentive_stats_pooling: the values and gradients of the ops calls, bit for bit, and within the restatement's bounds."""
    x, e, lens, gout = R.autograd_case(D, H)
    A = ktf.autograd
    tx = torch.as_tensor(x, device=DEV).requires_grad_(True)
    te = torch.as_tensor(e, device=DEV).requires_grad_(True)
    out = A.attentive_stats_pooling(tx, te, torch.as_tensor(np.asarray(lens), device=DEV))
    out.backward(torch.as_tensor(gout, device=DEV))
    res = run(x, e, lens, True, gout)
    got = dict(out=out.detach().cpu().numpy(), dx=tx.grad.cpu().numpy(), de=te.grad.cpu().numpy())
    for k in got:
        assert np.array_equal(_bits(got[k]), _bits(res[k])), k
    ref = R.pool(x, e, lens, True, R.EPS, gout)
    compare(f"autograd D={D} H={H}", got, ref, D, H)


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_training_step_gradients_and_export(mode):
    """First-step gradients of every parameter (the four attention tensors among them) and of the input features against fp64
    autograd of the restatement. Bound per tensor, as test_gpu_tdnn_grad.py derives it: |got - ref| <= stages * (n + 2) * 2^-24 * 8 *
    max |ref| with n = 6 * 90 rows and 16 stages here (five GEMMs, two normalisations and the pooling, forward and back); the
    split-bf16 operand term is two orders below (test_gpu_tdnn_grad16.py). The gradient of b2 is the exception: a softmax does not
    see a shift of its logits, so every column of de sums to zero over an utterance and max |ref| is rounding noise of the fp64
    restatement itself; its bound is the same factor times what that sum is made of, max_j sum_{b,t} |de_ref[b,t,j]| (the S of the
    derivation in place of 8 |value|). After export() the inference model reproduces the module's eval-mode output within the
    same factor."""
    from test_loss_cpu import torch_inv_norm, torch_loss
    A = ktf.autograd
    U = 2.0 ** -24
    w = _model_weights(seed=13)
    seq = _build("attentive", w, "f32")
    rng = np.random.default_rng(14)
    labels = np.arange(len(TRAIN_LENS)) % CLASSES
    centres = rng.standard_normal((CLASSES, FEAT))
    feats = (rng.standard_normal((len(TRAIN_LENS), max(TRAIN_LENS), FEAT)) + centres[labels][:, None, :]).astype(np.float32)
    torch.manual_seed(5)
    net = A.TrainableSequential(seq, gemm=mode, fused_norm=True).train()
    head = A.ClassifierHead(EMB, CLASSES, kind="aam", margin=0.2, scale=16.0, device=DEV)
    tf_ = torch.as_tensor(feats, device=DEV).requires_grad_(True)
    tl, ty = torch.as_tensor(TRAIN_LENS, device=DEV), torch.as_tensor(labels, device=DEV)
    loss, _ = head(net(tf_, tl), ty)
    loss.backward()

    params = list(net.params) + [head.weight]
    ref_params = [p.detach().cpu().to(F64).requires_grad_(True) for p in params]
    rf = torch.tensor(feats, dtype=F64, requires_grad=True)
    keep = {}
    emb = _restated_net(seq, ref_params[:-1], rf, TRAIN_LENS, keep)
    w64 = ref_params[-1]
    ref_loss = torch_loss(emb @ w64.T, torch.tensor(labels), torch_inv_norm(emb, 1e-12), torch_inv_norm(w64, 1e-12), "aam", 0.2, 16.0).mean()
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
    factor = 16 * (len(TRAIN_LENS) * max(TRAIN_LENS) + 2) * U * 8
    worst = 0.0
    names = {i: n for i, n in zip(range(6, 10), ("W1", "b1", "W2", "b2"))}
    for i, (g, r) in enumerate(zip([p.grad for p in params] + [tf_.grad], [r.grad for r in ref_params] + [rf.grad])):
        err, scale = float((g.cpu().to(F64) - r).abs().max()), float(r.abs().max())
        if names.get(i) == "b2":
            mask = torch.arange(max(TRAIN_LENS))[None, :] < torch.tensor(TRAIN_LENS)[:, None]
            scale = float((keep["e"].grad.abs() * mask.unsqueeze(-1)).sum((0, 1)).max()) / 8
        worst = max(worst, err / (factor * scale))
        tag = names.get(i, "features" if i == len(params) else f"parameter {i}")
        print(f"{mode} {tag} {tuple(g.shape)}: max |err| {err:.3e}, max |ref| {scale:.3e}, bound {factor * scale:.3e}")
        assert scale > 0 and err <= factor * scale, (mode, i, err, factor * scale)
    print(f"{mode}: worst |err| / bound over the tensors {worst:.4f}")
    assert [tuple(params[i].shape) for i in range(6, 10)] == [(ATT, 1, POOLED), (ATT,), (HEADS, 1, ATT), (HEADS,)]

    assert net.export() is seq
    asp = seq.get_layer("pool")
    for a, p in zip(asp.get_weights(), (params[6][:, 0, :].T, params[7], params[8][:, 0, :].T, params[9])):
        assert np.array_equal(_bits(a), _bits(p.detach().cpu().numpy()))
    with torch.no_grad():
        want = net.eval()(tf_.detach(), tl).cpu().numpy()
    seq.gemm = mode
    got = _run(seq, feats, TRAIN_LENS)
    d = np.abs(got - want).max() / max(1.0, np.abs(want).max())
    print(f"{mode}: exported model against the module in eval mode: {d:.3e} (limit {factor:.3e})")
    assert d <= factor
