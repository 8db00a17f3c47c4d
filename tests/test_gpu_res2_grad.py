"""The Res2Net backward on the GPU (include/ktf_res2.h rules 7 - 13): the training forward against the inference one bit for bit,
every gradient in every mode against tests/_res2_grad_ref.py with the limit measured on the slice composition through
ktf.autograd.tdnn_affine (e_new <= 2 e_comp + 2^-20 max|ref|: both round at the same points and differ in summation order), and the
bit-level invariances, and a small Res2Net x-vector model under TrainableSequential with a ClassifierHead against fp64 autograd of its
restatement. Every comparison prints its figures."""

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
from kaldi_tflite_amd import _lib as L, ops  # noqa: E402
import _res2_ref as R  # noqa: E402
import _res2_grad_ref as G  # noqa: E402
from test_loss_cpu import torch_inv_norm, torch_loss  # noqa: E402
from test_res2_grad_cpu import MODEL_CLASSES, MODEL_EMB, MODEL_LENS, model, model_inputs  # noqa: E402
from test_tdnn_grad_cpu import restated_pool, restated_tdnn  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77.0
MODES = {"f32": L.GEMM_F32, "bf16": L.GEMM_BF16, "bf16x3": L.GEMM_BF16X3}
CASES = [(16, 2, 1), (16, 3, 8), (64, 8, 2), (128, 4, 3), (128, 8, 4)]
KEYS = ("dx", "dW", "dbias", "dnscale", "dnshift")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows(a, ld, off, fill):
    """a (B, T, C) fp32 as a device tensor (B, T, ld) whose base lies `off` floats behind a 256-byte boundary; pad columns = fill."""
    B, T, C = a.shape
    buf = torch.full((B * T * ld + 64 + off,), fill, dtype=torch.float32, device=DEV)
    at = (-buf.data_ptr() // 4) % 64 + off
    v = buf[at:at + B * T * ld].view(B, T, ld)
    v[:, :, :C] = torch.as_tensor(a, device=DEV)
    return v


def _lens_for(s, d, Rt):
    return [0, 1, 2, d, d + 1, (s - 1) * d - 1, (s - 1) * d + 1, Rt - 1, Rt, Rt + 1, 2 * Rt + 1]


def _case(w, s, d, lens, seed):
    rng = np.random.default_rng(seed)
    f = lambda *sh: rng.standard_normal(sh).astype(np.float32)      # noqa: E731
    B, T = len(lens), max(lens) + 3
    return dict(x=f(B, T, s * w), g=f(B, T, s * w), W=(f(s - 1, 3, w, w) / np.sqrt(3 * w)).astype(np.float32), bias=0.1 * f(s - 1, w),
                nscale=rng.uniform(0.5, 2.0, (s - 1, w)).astype(np.float32), nshift=0.1 * f(s - 1, w))


def run(c, lens, s, d, gemm=L.GEMM_F32, relu=True, bn=True, ld=0, off=0, only=None):
    """Training forward and both gradient calls on copies of c's x and g with NaN in every row from the length on and in every pad
    column, into outputs full of SENTINEL -> dict of numpy arrays (y, a, dx with their pad columns)."""
    sel = slice(None) if only is None else slice(only, only + 1)
    x, g = np.array(c["x"][sel]), np.array(c["g"][sel])
    lens = lens if only is None or lens is None else lens[only:only + 1]
    B, T, C = x.shape
    w = C // s
    for b in range(B if lens is not None else 0):
        x[b, R.clamp_len(lens[b], T):] = g[b, R.clamp_len(lens[b], T):] = np.nan
    sent = lambda cols: _rows(np.full((B, T, cols), SENTINEL, np.float32), cols + ld, off, SENTINEL)      # noqa: E731
    tx, tg, ty, ta, tdx, tgt = _rows(x, C + ld, off, np.nan), _rows(g, C + ld, off, np.nan), sent(C), sent(C - w), sent(C), sent(C - w)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)      # noqa: E731
    tl = None if lens is None else dev(np.asarray(lens, np.int32))
    W, nsc, nsh = dev(c["W"].reshape(s - 1, 3 * w, w)), dev(c["nscale"]) if bn else None, dev(c["nshift"]) if bn else None
    act = L.ACT_RELU if relu else L.ACT_NONE
    a = ta[:, :, :C - w] if bn else None
    ops.res2_conv_train(tx[:, :, :C], tl, s, d, W, dev(c["bias"]), nsc, nsh, act, gemm, ty[:, :, :C], a)
    for b in range(B if lens is not None else 0):                # the unwritten rows of y and a become NaN: the backward may not read them
        n = R.clamp_len(lens[b], T)
        assert (ty[b, n:] == SENTINEL).all() and (ta[b, n:] == SENTINEL).all(), b
        ty[b, n:] = ta[b, n:] = np.nan
    ops.res2_grad_data(tg[:, :, :C], tl, s, d, W, nsc, ty[:, :, :C], a, act, gemm, tdx[:, :, :C], tgt[:, :, :C - w])
    new = lambda *sh: torch.full(sh, SENTINEL, dtype=torch.float32, device=DEV)      # noqa: E731
    dw, db, dsc, dsh = new(s - 1, 3 * w, w), new(s - 1, w), new(s - 1, w) if bn else None, new(s - 1, w) if bn else None
    ops.res2_grad_weights(tx[:, :, :C], tl, s, d, nsc, ty[:, :, :C], a, tgt[:, :, :C - w], act, gemm, dw, db, dsc, dsh,
                          ops.res2_grad_scratch(B, T, w, s, DEV))
    torch.cuda.synchronize()
    out = dict(y=ty, a=ta, dx=tdx, dW=dw.view(s - 1, 3, w, w), dbias=db, dnscale=dsc, dnshift=dsh)
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _reference(c, out, lens, s, d, relu, bn):
    """The fp64 gradients on the GPU forward's y and a: parameter gradients summed over the batch, dx per utterance."""
    C = c["x"].shape[2]
    tot, dxs = {}, []
    for b, n in enumerate(lens):
        if n == 0:
            dxs.append(np.zeros((0, C)))
            continue
        r, _ = G.grad(c["x"][b, :n], out["y"][b, :n, :C], out["a"][b, :n, :C - C // s] if bn else None, c["g"][b, :n], s, d, c["W"],
                      c["nscale"] if bn else None, relu)
        dxs.append(r["dx"])
        for k in KEYS[1:]:
            tot[k] = tot.get(k, 0.0) + r[k]
    return tot, dxs


@pytest.mark.parametrize("w,s,d", CASES)
def test_training_forward_has_the_inference_bits_and_saves_the_activation(w, s, d):
    C = s * w
    lens = R.exact_lens(s, d, ops.res2_row_tile(w, s, d))
    c = R.exact_case(w, s, d, lens)
    c["g"] = np.zeros_like(c["x"])
    out = run(c, lens, s, d, ld=8)
    y = torch.full((len(lens), c["x"].shape[1], C), SENTINEL, dtype=torch.float32, device=DEV)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)      # noqa: E731
    ops.res2_conv(dev(c["x"]), dev(np.asarray(lens, np.int32)), s, d, dev(c["W"].reshape(s - 1, 3 * w, w)), dev(c["bias"]), dev(c["nscale"]),
                  dev(c["nshift"]), L.ACT_RELU, L.GEMM_F32, y)
    y = y.cpu().numpy()
    for b, n in enumerate(lens):
        assert (out["a"][b, :n, C - w:] == SENTINEL).all() and (out["y"][b, :n, C:] == SENTINEL).all()
        assert np.array_equal(_bits(out["y"][b, :n, :C]), _bits(y[b, :n])) and (out["a"][b, :n, :C - w] != SENTINEL).all()
        trace = []
        if n:
            R.conv(c["x"][b, :n], s, d, c["W"], c["bias"], c["nscale"], c["nshift"], trace=trace)
            assert np.array_equal(_bits(out["a"][b, :n, :C - w]), _bits(np.concatenate([st["A"] for st in trace], 1))), (b, n)
    # all-zero g: every gradient is exactly zero
    assert all((out[k] == 0).all() for k in KEYS[1:]) and all((out["dx"][b, :, :C] == 0).all() for b in range(len(lens)))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("w,s,d", CASES)
def test_gradients_against_fp64_with_the_limit_of_the_slice_composition(w, s, d, mode):
    C = s * w
    lens = _lens_for(s, d, ops.res2_grad_row_tile(w, s, d, MODES[mode]))
    c = _case(w, s, d, lens, 7 + w + s + d)
    for sel, Tc, ls, relu, bn, slots in ((slice(None), None, lens, True, True, 3), (slice(None), None, None, True, False, 3),
                                         (slice(1, 3), 4, lens[1:3], False, True, 2), (slice(2, 3), 4, lens[2:3], True, False, 1)):
        cc = {k: (v[sel, :Tc] if k in ("x", "g") else v) for k, v in c.items()}
        out = run(cc, ls, s, d, MODES[mode], relu, bn)
        B, T = cc["x"].shape[:2]
        ns = [T] * B if ls is None else [R.clamp_len(n, T) for n in ls]
        ref, ref_dx = _reference(cc, out, ns, s, d, relu, bn)
        # today's route: slices, tdnn_affine and torch ops in the same mode
        t = lambda a: torch.tensor(a, device=DEV, requires_grad=True)      # noqa: E731
        x, W, bias, nsc, nsh = t(cc["x"]), t(cc["W"]), t(cc["bias"]), t(cc["nscale"]), t(cc["nshift"])
        tl = None if ls is None else torch.as_tensor(np.asarray(ls, np.int32), device=DEV)
        ys = [x[:, :, :w]]
        for i in range(1, s):
            u = x[:, :, i * w:(i + 1) * w] + ys[-1] if i >= 2 else x[:, :, w:2 * w]
            z = ktf.autograd.tdnn_affine(u, W[i - 1].permute(2, 0, 1), bias[i - 1], [-d, 0, d], tl, gemm=mode)
            z = torch.relu(z) if relu else z
            ys.append(z * nsc[i - 1] + nsh[i - 1] if bn else z)
        gm = np.array(cc["g"])
        for b, n in enumerate(ns):
            gm[b, n:] = 0
        (torch.cat(ys, 2) * torch.as_tensor(gm, device=DEV)).sum().backward()
        comp = dict(dW=W.grad, dbias=bias.grad, dnscale=nsc.grad, dnshift=nsh.grad)
        assert min(ops.res2_grad_slots(B, T, w, s), 3) == slots
        for k in KEYS:
            if k in ("dnscale", "dnshift") and not bn:
                continue
            if k == "dx":
                e_new, e_comp = (max([float(np.abs(a[b, :n, :C] - ref_dx[b]).max()) for b, n in enumerate(ns) if n] + [0.0])
                                 for a in (out["dx"], x.grad.cpu().numpy()))
                top = max([float(np.abs(r).max()) for r in ref_dx if len(r)] + [0.0])
            else:
                e_new, e_comp = (float(np.abs(a - ref[k]).max()) for a in (out[k], comp[k].cpu().numpy()))
                top = float(np.abs(ref[k]).max())
            print(f"w {w} s {s} d {d} {mode} relu {relu} bn {bn} {k}: e_new {e_new:.3e} e_comp {e_comp:.3e} max|ref| {top:.3e} "
                  f"e_new/max|ref| {e_new / max(top, 1e-300):.3e}")
            assert e_new <= 2 * e_comp + 2.0 ** -20 * top, (k, relu, bn)
        for b, n in enumerate(ns):
            assert np.array_equal(_bits(out["dx"][b, :n, :w]), _bits(cc["g"][b, :n, :w])) and (out["dx"][b, n:, :C] == 0).all(), b


@pytest.mark.parametrize("w,s,d,mode", [(16, 3, 8, "f32"), (64, 8, 2, "f32"), (64, 8, 2, "bf16x3"), (128, 4, 3, "bf16")])
def test_strides_alignment_batch_and_repeats_do_not_change_a_bit(w, s, d, mode):
    C, Rt = s * w, ops.res2_grad_row_tile(w, s, d, MODES[mode])
    lens = [Rt + 3, 0, 5, 2 * Rt + 1, (s - 1) * d + 1]
    c = _case(w, s, d, lens, 5)
    for relu, bn in ((True, True), (False, False)):
        plain = run(c, lens, s, d, MODES[mode], relu, bn)
        again = run(c, lens, s, d, MODES[mode], relu, bn)
        assert np.isfinite(plain["dx"][0, :lens[0]]).all() and all(np.isfinite(plain[k]).all() for k in KEYS[1:] if k in plain)
        assert all(np.array_equal(_bits(plain[k]), _bits(again[k])) for k in plain)
        moved = run(c, lens, s, d, MODES[mode], relu, bn, ld=8, off=4)
        assert np.array_equal(_bits(moved["dx"][:, :, :C]), _bits(plain["dx"])) and (moved["dx"][:, :, C:] == SENTINEL).all()
        assert all(np.array_equal(_bits(moved[k]), _bits(plain[k])) for k in KEYS[1:] if k in plain)
        for b in (0, 3):
            assert np.array_equal(_bits(run(c, lens, s, d, MODES[mode], relu, bn, only=b)["dx"][0]), _bits(plain["dx"][b])), b
        for b, n in enumerate(lens):
            assert (plain["dx"][b, n:] == 0).all()


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_autograd_function_gives_the_gradients_of_the_calls(mode):
    w, s, d, lens = 32, 4, 2, [70, 9, 33]
    c = _case(w, s, d, lens, 11)
    out = run(c, lens, s, d, MODES[mode])
    t = lambda a: torch.tensor(a, device=DEV, requires_grad=True)      # noqa: E731
    x, W, bias, nsc, nsh = t(c["x"]), t(c["W"].reshape(s - 1, 3 * w, w)), t(c["bias"]), t(c["nscale"]), t(c["nshift"])
    y = ktf.autograd.res2_conv(x, W, bias, nsc, nsh, s, d, lens=lens, gemm=mode)
    assert all((y[b, n:] == 0).all() for b, n in enumerate(lens))
    (y * torch.as_tensor(c["g"], device=DEV)).sum().backward()
    got = dict(dx=x.grad, dW=W.grad.view(s - 1, 3, w, w), dbias=bias.grad, dnscale=nsc.grad, dnshift=nsh.grad)
    assert all(np.array_equal(_bits(got[k].cpu().numpy()), _bits(out[k])) for k in KEYS)


def _restated_model(seq, params, feats, lens):
    """The model of test_res2_grad_cpu.model() in torch ops on fp64, training-mode BatchNorm on the valid rows."""
    x, it, pooled = feats, iter(params), False
    mask = (torch.arange(feats.shape[1])[None, :] < torch.tensor(lens)[:, None]).unsqueeze(-1)
    for l in seq.layers:
        if isinstance(l, ktf.layers.TDNN):
            w, b = next(it), next(it)
            x = x @ w[:, 0, :].T + b if pooled else restated_tdnn(x, w, b, lens, list(l.context), 1, "SAME")
        elif isinstance(l, ktf.layers.ReLU):
            x = torch.relu(x)
        elif isinstance(l, ktf.layers.BatchNorm):
            rows = torch.cat([x[b, :n] for b, n in enumerate(lens)])
            y = next(it) * (x - rows.mean(0)) / torch.sqrt(rows.var(0, unbiased=False) + l.epsilon)
            x = torch.where(mask, y, torch.zeros((), dtype=x.dtype))
        elif isinstance(l, ktf.layers.Res2Conv):
            k, b, nsc, nsh = (next(it) for _ in range(4))
            ys = [G.restatement(x[i, :n], k.view(l.scale - 1, 3, l.width, l.width), b, nsc, nsh, l.scale, l.dilation)[0] for i, n in enumerate(lens)]
            x = torch.stack([torch.cat([y, torch.zeros((x.shape[1] - len(y), x.shape[2]), dtype=x.dtype)]) for y in ys])
        else:
            x, pooled = restated_pool(x, lens, l.includeStd, l.epsilon, l.inputPeriod), True
    return x


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_model_with_a_res2conv_under_trainable_sequential_and_a_classifier_head(mode):
    """TDNN -> ReLU -> BatchNorm -> Res2Conv -> BatchNorm -> StatsPooling -> TDNN with an AAM ClassifierHead. First-step gradients of
    every parameter and of the input against fp64 autograd of the restatement, within the bound tests/test_gpu_tdnn_grad.py derives,
    per tensor |got - ref| <= 14 * (n + 2) * 2^-24 * 8 * max|ref| with n = B * T rows of this batch; the seeded inputs keep every ReLU
    input away from zero (tests/test_res2_grad_cpu.py). After export() the inference model against the module's eval output at the
    limits of tests/test_gpu_parity.py: 2e-5 ("f32") and 2e-4 ("bf16x3") of max(1, max|want|)."""
    seq = model()
    feats, labels = model_inputs()
    torch.manual_seed(5)
    net = ktf.autograd.TrainableSequential(seq, gemm=mode).train()
    head = ktf.autograd.ClassifierHead(MODEL_EMB, MODEL_CLASSES, kind="aam", margin=0.2, scale=16.0, gemm=mode, device=DEV)
    tf_ = torch.tensor(feats, device=DEV, requires_grad=True)
    tl, ty = torch.as_tensor(MODEL_LENS, device=DEV), torch.as_tensor(labels, device=DEV)
    loss, _ = head(net(tf_, tl), ty)
    loss.backward()
    params = [tf_] + list(net.params) + [head.weight]
    ref = [p.detach().cpu().to(torch.float64).requires_grad_(True) for p in params]
    emb = _restated_model(seq, ref[1:-1], ref[0], MODEL_LENS)
    ref_loss = torch_loss(emb @ ref[-1].T, torch.tensor(labels), torch_inv_norm(emb, 1e-12), torch_inv_norm(ref[-1], 1e-12), "aam", 0.2, 16.0).mean()
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) <= 1e-4 * abs(ref_loss.item())
    factor = 14 * (len(MODEL_LENS) * max(MODEL_LENS) + 2) * 2.0 ** -24 * 8
    worst = []
    for i, (p, r) in enumerate(zip(params, ref)):
        err, top = float((p.grad.cpu().to(torch.float64) - r.grad).abs().max()), float(r.grad.abs().max())
        print(f"{mode} tensor {i} {tuple(p.shape)}: max |err| {err:.3e}, max |ref| {top:.3e}, bound {factor * top:.3e}")
        worst.append((err, factor * top, i))
    for err, bound, i in worst:
        assert err <= bound, (mode, i, err, bound)

    res = seq.layers[3]
    assert net.export() is seq
    at = [st[2] for st in net.steps if st[1] is res][0]
    for k, wgt in enumerate(res.get_weights()):
        assert np.array_equal(_bits(wgt.reshape(net.params[at + k].shape)), _bits(net.params[at + k].detach().cpu().numpy())), k
    one = tf_[0:1].detach()                                      # the longest utterance: no padding rows, no lengths needed
    with torch.no_grad():
        want = net.eval()(one, None).cpu().numpy().reshape(-1)
    seq.gemm = mode
    got = seq(one).float().cpu().numpy().reshape(-1)
    tol = {"f32": 2e-5, "bf16x3": 2e-4}[mode] * max(1.0, float(np.abs(want).max()))
    print(f"{mode} export: max |inference - eval| {np.abs(got - want).max():.3e}, limit {tol:.3e}")
    assert got.shape == want.shape and np.abs(got - want).max() <= tol
