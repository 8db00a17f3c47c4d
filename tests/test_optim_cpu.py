"""ktf.optim without a GPU: the fp64 oracle (tests/_optim_ref.py) against torch.optim.SGD / Adam / AdamW and clip_grad_norm_ in
fp64 on the CPU, its max-change and skipped-step branches by hand, the C-ABI of include/ktf_optim.h (symbols, argument types,
every refusal before any launch, the workspace size), kaldi_lr and the argument checks of ktf.optim.Optimizer."""

import ctypes as C
import os
import re
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
from kaldi_tflite_amd import _lib as L  # noqa: E402
import _optim_ref as R  # noqa: E402

F64 = np.float64
SIZES = (7, 0, 33)


def _close(got, want, what):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max()) if np.asarray(want).size else 0.0
    scale = max(float(np.abs(np.asarray(want)).max()) if np.asarray(want).size else 0.0, 1.0)
    assert err <= 1e-12 * scale, (what, err, scale)


# ----------------------------------------------------------------------------- the oracle against torch.optim
TORCH_CASES = {
    "sgd": dict(kind="sgd"),
    "sgd-momentum": dict(kind="sgd", momentum=0.9),
    "sgd-nesterov": dict(kind="sgd", momentum=0.9, nesterov=True),
    "sgd-momentum-decay": dict(kind="sgd", momentum=0.8, wd=0.05),
    "sgd-clip": dict(kind="sgd", momentum=0.9, clip=0.5),
    "adam": dict(kind="adam"),
    "adam-decay": dict(kind="adam", wd=0.05),
    "adamw": dict(kind="adam", wd=0.05, decoupled=True),
    "adam-clip": dict(kind="adam", clip=0.5, wd=0.01),
}


@pytest.mark.parametrize("case", list(TORCH_CASES))
def test_oracle_equals_torch_optim_in_fp64(case):
    o = dict(momentum=0.0, nesterov=False, wd=0.0, decoupled=False, clip=0.0)
    o.update(TORCH_CASES[case])
    rng = np.random.default_rng(11)
    lr, betas, eps = 0.05, (0.9, 0.99), 1e-6
    rows, total = R.layout(SIZES)
    segs = [(b, e, 0, 0.0) for b, e in rows]
    p = np.zeros(total)
    for b, e in rows:
        p[b:e] = rng.standard_normal(e - b)
    has_m, adam = o["kind"] == "adam" or o["momentum"] != 0.0, o["kind"] == "adam"
    m, v = (np.zeros(total) if has_m else None), (np.zeros(total) if adam else None)

    tp = [torch.tensor(p[b:e], dtype=torch.float64, requires_grad=True) for b, e in rows]
    if adam:
        cls = torch.optim.AdamW if o["decoupled"] else torch.optim.Adam
        opt = cls(tp, lr=lr, betas=betas, eps=eps, weight_decay=o["wd"])
    else:
        opt = torch.optim.SGD(tp, lr=lr, momentum=o["momentum"], nesterov=o["nesterov"], weight_decay=o["wd"])

    for step in range(1, 6):
        g = np.zeros(total)
        for b, e in rows:
            g[b:e] = rng.standard_normal(e - b) * step
        want = R.step(p, g, m, v, segs, [(lr, o["wd"])], kind=o["kind"], momentum=o["momentum"], nesterov=o["nesterov"], betas=betas, eps=eps,
                      step=step, decoupled=o["decoupled"], clip_norm=o["clip"], sums="exact", dtype=F64)
        for t, (b, e) in zip(tp, rows):
            t.grad = torch.tensor(g[b:e], dtype=torch.float64)
        if o["clip"]:
            # torch's coefficient is max_norm / (G + 1e-6), the rule's is clip_norm / G: the norms agree, the clipped gradients agree
            # once torch's are freed of its 1e-6, and the step is then taken from the rule's
            G = float(torch.nn.utils.clip_grad_norm_(tp, o["clip"]))
            _close(want["G"], G, "G")
            assert want["G"] > o["clip"] and want["c"] == o["clip"] / want["G"] < 1.0
            for t, (b, e) in zip(tp, rows):
                _close(t.grad.numpy() * (G + 1e-6) / G, want["c"] * g[b:e], "clipped gradient")
                t.grad = torch.tensor(want["c"] * g[b:e], dtype=torch.float64)
        else:
            assert want["G"] == 0.0 and want["c"] == 1.0
        opt.step()
        assert not want["skipped"] and want["sigma"] == 1.0 and (want["sigma_s"] == 1.0).all()
        p, m, v = want["p"], want["m"], want["v"]
        for t, (b, e) in zip(tp, rows):
            _close(p[b:e], t.detach().numpy(), f"{case} p step {step}")
            if has_m and e > b:
                st = opt.state[t]
                _close(m[b:e], st["exp_avg" if adam else "momentum_buffer"].numpy(), f"{case} m step {step}")
                if adam:
                    _close(v[b:e], st["exp_avg_sq"].numpy(), f"{case} v step {step}")


def test_decoupled_decay_under_sgd_is_the_shrink_then_step_form():
    rows, total = R.layout((5,))
    p, g = np.zeros(total), np.zeros(total)
    p[:5], g[:5] = [1.0, -2.0, 3.0, 0.5, 0.0], [0.5, 0.25, -1.0, 2.0, 1.0]
    out = R.step(p, g, np.zeros(total), None, [(0, 5, 0, 0.0)], [(0.1, 0.2)], momentum=0.5, decoupled=True, dtype=F64, sums="exact")
    _close(out["p"][:5], p[:5] * (1 - 0.1 * 0.2) - 0.1 * g[:5], "p")
    _close(out["m"][:5], g[:5], "m holds no decay")


# ----------------------------------------------------------------------------- max-change and the guard, by hand
def _two_segments():
    """d = g (plain SGD): segment 0 has |d| = 5 under lr 1/2, segment 1 has |d| = 13 under lr 1/4."""
    rows, total = R.layout((2, 2))
    p, g = np.zeros(total, dtype=np.float32), np.zeros(total, dtype=np.float32)
    p[0:2], g[0:2] = [10.0, 20.0], [3.0, 4.0]
    p[R.SLOT:R.SLOT + 2], g[R.SLOT:R.SLOT + 2] = [30.0, 40.0], [5.0, 12.0]
    return rows, p, g


def test_max_change_branches_by_hand():
    rows, p, g = _two_segments()
    (b0, e0), (b1, e1) = rows
    groups = [(0.5, 0.0), (0.25, 0.0)]

    def run(mc0, mc1, glob):
        return R.step(p, g, None, None, [(b0, e0, 0, mc0), (b1, e1, 1, mc1)], groups, max_change_global=glob)

    out = run(1.25, 0.0, 0.0)                                  # N_0 = 2.5, N_1 = 3.25: segment 0 alone is halved
    assert np.array_equal(out["Ns"], [2.5, 3.25]) and np.array_equal(out["sigma_s"], [0.5, 1.0]) and out["sigma"] == 1.0
    assert out["N"] == np.sqrt(1.25 ** 2 + 3.25 ** 2) and not out["skipped"] and out["G"] == 0.0 and out["c"] == 1.0
    assert np.array_equal(out["p"][b0:e0], [10 - 0.25 * 3, 20 - 0.25 * 4]) and np.array_equal(out["p"][b1:e1], [30 - 0.25 * 5, 40 - 0.25 * 12])

    out = run(4.0, 4.0, 2.0)                                   # no segment is limited, the whole step is: N = sqrt(2.5^2 + 3.25^2)
    N = float(np.sqrt(np.float64(2.5 ** 2 + 3.25 ** 2)))
    assert np.array_equal(out["sigma_s"], [1.0, 1.0]) and out["N"] == N and out["sigma"] == 2.0 / N
    assert np.array_equal(out["p"][b0:e0], (np.array([10.0, 20.0]) - ((2.0 / N) * 0.5) * np.array([3.0, 4.0])).astype(np.float32))

    out = run(1.5, 2.0, 1.25)                                  # both: (1.5, 2) are what the segments may move, N = 2.5 is halved
    assert np.array_equal(out["sigma_s"], [1.5 / 2.5, 2.0 / 3.25]) and out["sigma"] == 0.5
    t0, t1 = (1.5 / 2.5) * 2.5, (2.0 / 3.25) * 3.25
    assert out["N"] == float(np.sqrt(np.float64(t0 * t0 + t1 * t1)))
    assert np.array_equal(out["p"][b1:e1], (np.array([30.0, 40.0]) - ((0.5 * (2.0 / 3.25)) * 0.25) * np.array([5.0, 12.0])).astype(np.float32))

    out = run(0.0, 0.0, 0.0)                                   # everything off: nothing is reduced
    assert out["N"] == 0.0 and out["sigma"] == 1.0 and np.array_equal(out["p"][b0:e0], [8.5, 18.0])


def test_limited_sgd_step_scales_the_stored_momentum_and_adam_does_not():
    rows, p, g = _two_segments()
    (b0, e0), (b1, e1) = rows
    segs = [(b0, e0, 0, 1.25), (b1, e1, 0, 0.0)]
    z = np.zeros_like(p)
    out = R.step(p, g, z, None, segs, [(0.5, 0.0)], momentum=0.5)
    assert np.array_equal(out["sigma_s"], [0.5, 1.0])
    assert np.array_equal(out["m"][b0:e0], [1.5, 2.0]) and np.array_equal(out["m"][b1:e1], [5.0, 12.0])
    segs = [(b0, e0, 0, 0.25), (b1, e1, 0, 0.0)]                # Adam's d = g / (|g| + 1) here: N_0 = 0.5 * sqrt(0.75^2 + 0.8^2)
    ad = R.step(p, g, z, z, segs, [(0.5, 0.0)], kind="adam", betas=(0.5, 0.75), eps=1.0)
    free = R.step(p, g, z, z, [(b0, e0, 0, 0.0), (b1, e1, 0, 0.0)], [(0.5, 0.0)], kind="adam", betas=(0.5, 0.75), eps=1.0)
    assert ad["sigma_s"][0] < 1.0 and np.array_equal(ad["m"], free["m"]) and np.array_equal(ad["v"], free["v"])
    assert not np.array_equal(ad["p"][b0:e0], free["p"][b0:e0]) and np.array_equal(ad["p"][b1:e1], free["p"][b1:e1])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_norm_skips_the_step(bad):
    rows, p, g = _two_segments()
    (b0, e0), (b1, e1) = rows
    g[b1] = bad
    m = np.ones_like(p)
    for kw in (dict(clip_norm=1.0), dict(max_change_global=1.0), dict(clip_norm=1.0, max_change_global=1.0)):
        out = R.step(p, g, m, None, [(b0, e0, 0, 0.0), (b1, e1, 0, 0.0)], [(0.5, 0.0)], momentum=0.5, **kw)
        assert out["skipped"] == 1.0 and np.array_equal(out["p"], p) and np.array_equal(out["m"], m)
        assert R.stats_vector(out)[4] == 1.0
    out = R.step(p, g, m, None, [(b0, e0, 0, 0.0), (b1, e1, 0, 0.0)], [(0.5, 0.0)], momentum=0.5)      # no reduction, no guard
    assert out["skipped"] == 0.0 and not np.isfinite(out["p"][b1])


def test_kernel_order_sums_equal_exact_sums_on_integers():
    rng = np.random.default_rng(3)
    sizes = (0, 1, 3, R.SLOT - 1, R.SLOT, R.SLOT + 1, 2 * R.SLOT + 17)
    rows, total = R.layout(sizes)
    g = np.full(total, np.nan, dtype=np.float32)
    for b, e in rows:
        g[b:e] = rng.integers(-8, 9, e - b)
    segs = [(b, e, 0, 0.0) for b, e in rows]
    p = np.full(total, np.nan, dtype=np.float32)
    for x, y in rows:
        p[x:y] = 0.0
    a = R.step(p, g, None, None, segs, [(0.5, 0.0)], clip_norm=1.0, max_change_global=1.0, sums="kernel")
    b = R.step(p, g, None, None, segs, [(0.5, 0.0)], clip_norm=1.0, max_change_global=1.0, sums="exact")
    assert a["G"] == b["G"] == float(np.sqrt(np.float64(sum(float((g[x:y].astype(F64) ** 2).sum()) for x, y in rows))))
    assert np.isnan(a["p"][rows[1][1]:rows[2][0]]).all()          # padding is carried over
    # without clipping d is a small dyadic number too (integers, powers of two): Nesterov momentum, decay and both max-change limits
    # give the same bits whichever way the sums are added -- what the exact-input cases of the GPU tests rest on under SGD
    p[:] = np.where(np.isnan(p), np.nan, 0.0) + np.nan_to_num(np.roll(g, 1))
    m = np.nan_to_num(np.roll(g, 2)).astype(np.float32)
    segs = [(x, y, i % 2, 2.0 ** -6 if i % 3 != 2 else 0.0) for i, (x, y) in enumerate(rows)]
    kw = dict(momentum=0.5, nesterov=True, max_change_global=2.0 ** -8)
    a, b = (R.step(p, g, m, None, segs, [(0.5, 0.125), (0.25, 0.0)], sums=s, **kw) for s in ("kernel", "exact"))
    assert a["sigma"] < 1.0 and (a["sigma_s"] < 1.0).any()
    assert np.array_equal(R.stats_vector(a), R.stats_vector(b))
    assert np.array_equal(a["p"].view(np.uint32), b["p"].view(np.uint32)) and np.array_equal(a["m"].view(np.uint32), b["m"].view(np.uint32))


# ----------------------------------------------------------------------------- the C-ABI
def test_header_symbols_are_the_optim_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_optim.h")).read()
    code = hdr[hdr.index("#ifndef KTF_OPTIM_H_"):]
    protos = re.findall(r"^(int|int32_t|int64_t) (ktf_[a-z0-9_]+)\(([^;]*)\);", code, flags=re.M)
    assert {n for _, n, _ in protos} == set(L.OPTIM_PROTOTYPES) == set(re.findall(r"\b(ktf_[a-z0-9_]+)\s*\(", code))
    ctype = {"float*": L._P, "const float*": L._P, "double*": L._P, "void*": L._P, "const KtfOptimSeg*": L._P, "const KtfOptimGroup*": L._P,
             "int64_t": L._i64, "int32_t": L._i32, "double": C.c_double, "size_t": C.c_size_t}
    res = {"int": C.c_int, "int32_t": L._i32, "int64_t": L._i64}
    for r, name, args in protos:
        args = [a.strip() for a in " ".join(args.split()).split(",")]
        want = [] if args == ["void"] else [ctype[a.rsplit(" ", 1)[0]] for a in args]
        assert L.OPTIM_PROTOTYPES[name] == (res[r], want), name
    assert all(n.startswith("ktf_optim_") for n in L.OPTIM_PROTOTYPES)
    lib = L.load()
    for name in L.OPTIM_PROTOTYPES:
        assert hasattr(lib, name), name
    others = (set(L.PROTOTYPES) | set(L.AUGMENT_PROTOTYPES) | set(L.RESAMPLE_PROTOTYPES) | set(L.GRAD_PROTOTYPES) | set(L.NORM_PROTOTYPES)
              | set(L.LOSS_PROTOTYPES) | set(L.EGS_PROTOTYPES))
    assert not set(L.OPTIM_PROTOTYPES) & others
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "ktf_optim.h":
            assert "ktf_optim_" not in open(os.path.join(ROOT, "include", other)).read(), other
    slot = int(re.search(r"#define KTF_OPTIM_SLOT_ELEMS (\d+)", hdr).group(1))
    assert lib.ktf_optim_slot_elems() == slot == R.SLOT and slot % 1024 == 0
    assert int(re.search(r"#define KTF_OPTIM_MAX_GROUPS (\d+)", hdr).group(1)) == L.OPTIM_MAX_GROUPS == 8
    assert (int(re.search(r"#define KTF_OPTIM_SGD (\d+)", hdr).group(1)), int(re.search(r"#define KTF_OPTIM_ADAM (\d+)", hdr).group(1))) \
        == (L.OPTIM_SGD, L.OPTIM_ADAM)
    # the structures as the header lays them out
    assert C.sizeof(L.OptimSeg) == 24 and C.sizeof(L.OptimGroup) == 16
    assert [(n, getattr(L.OptimSeg, n).offset) for n, _ in L.OptimSeg._fields_] == [("begin", 0), ("end", 8), ("group", 16), ("max_change", 20)]
    assert re.search(r"int64_t begin, end;.*\n\s*int32_t group;.*\n\s*float max_change;", hdr) and re.search(r"double lr, weight_decay;", hdr)
    assert "No Kaldi source" in hdr


def _refused(rc, text):
    assert rc == -1, rc
    assert text in L.last_error(), L.last_error()
    with pytest.raises(ValueError):
        L.check(rc, "x")


def test_argument_checks_without_gpu():
    lib = L.load()
    S = lib.ktf_optim_slot_elems()
    total = 3 * S
    raw = (C.c_float * (4 * total + 4096))()
    base = (C.addressof(raw) + 255) & ~255
    at = lambda k: C.c_void_p(base + 4 * total * k)  # noqa: E731   stands for any aligned device pointer: every refusal comes before a launch
    need = lib.ktf_optim_workspace_bytes(total, 2)
    assert need > 0
    ok_segs = [(0, 5, 0, 0.0), (S, 3 * S, 1, 1.0)]
    ok_groups = [(0.5, 0.0), (0.25, 0.125)]

    def call(p=at(0), g=at(1), m=at(2), v=at(3), total=total, segs=ok_segs, segs_host="table", segs_dev=at(0), n_seg=None, groups=ok_groups,
             groups_ptr="table", n_groups=None, kind=0, momentum=0.5, nesterov=0, beta1=0.9, beta2=0.999, eps=1e-8, step=1, decoupled=0,
             clip=0.0, glob=0.0, ws=at(0), ws_bytes=None):
        table = (L.OptimSeg * max(len(segs), 1))(*[L.OptimSeg(*s) for s in segs])
        gt = (L.OptimGroup * max(len(groups), 1))(*[L.OptimGroup(*x) for x in groups])
        return lib.ktf_optim_step(p, g, m, v, total, C.cast(table, C.c_void_p) if segs_host == "table" else segs_host, segs_dev,
                                  len(segs) if n_seg is None else n_seg, C.cast(gt, C.c_void_p) if groups_ptr == "table" else groups_ptr,
                                  len(groups) if n_groups is None else n_groups, kind, momentum, nesterov, beta1, beta2, eps, step, decoupled,
                                  clip, glob, None, ws, need if ws_bytes is None else ws_bytes, None)

    for name in ("p", "g", "segs_host", "segs_dev", "groups_ptr", "ws"):
        _refused(call(**{name: None}), "null")
    _refused(call(m=None), "null m")                              # momentum 0.5
    _refused(call(kind=1, m=None), "null m or v")
    _refused(call(kind=1, v=None), "null m or v")
    _refused(call(n_seg=-1), "negative n_seg")
    _refused(call(total=-1), "negative total")
    _refused(call(total=1 << 40), "2^40")
    for segs, text in (([(1, 5, 0, 0.0)], "no multiple"), ([(-S, 5, 0, 0.0)], "no multiple"), ([(S, S - 1, 0, 0.0)], "ends before"),
                       ([(0, total + 1, 0, 0.0)], "beyond total"), ([(0, S + 1, 0, 0.0), (S, 2 * S, 0, 0.0)], "ascending"),
                       ([(S, 2 * S, 0, 0.0), (0, 5, 0, 0.0)], "ascending"), ([(0, 5, 2, 0.0)], "group"), ([(0, 5, -1, 0.0)], "group"),
                       ([(0, 5, 0, -1.0)], "max_change"), ([(0, 5, 0, float("inf"))], "max_change"), ([(0, 5, 0, float("nan"))], "max_change")):
        _refused(call(segs=segs), text)
    _refused(call(n_groups=0), "n_groups")
    _refused(call(groups=[(0.5, 0.0)] * 9, segs=[(0, 5, 0, 0.0)]), "n_groups")
    for bad in (-0.5, float("inf"), float("nan")):
        _refused(call(groups=[(bad, 0.0), (0.25, 0.0)]), "lr")
        _refused(call(groups=[(0.5, 0.0), (0.25, bad)]), "weight_decay")
        _refused(call(clip=bad), "clip_norm")
        _refused(call(glob=bad), "max_change_global")
    for bad in (-0.1, 1.0, float("nan")):
        _refused(call(momentum=bad), "momentum")
        _refused(call(kind=1, beta1=bad), "beta")
        _refused(call(kind=1, beta2=bad), "beta")
    _refused(call(momentum=0.0, nesterov=1), "nesterov")
    for bad in (0.0, -1e-8, float("inf"), float("nan")):
        _refused(call(kind=1, eps=bad), "eps")
    _refused(call(kind=1, step=0), "step")
    _refused(call(kind=2), "unknown kind")
    _refused(call(kind=-1), "unknown kind")
    _refused(call(ws_bytes=need - 1), "workspace")
    _refused(call(ws=C.c_void_p(base + 4)), "256-byte")
    last = C.c_void_p(base + 4 * (total - 1))                     # the last float of p
    _refused(call(g=last), "overlap")
    _refused(call(m=last), "overlap")
    _refused(call(kind=1, v=last), "overlap")
    _refused(call(kind=1, g=at(2)), "overlap")                    # g on m
    _refused(call(kind=1, v=at(1)), "overlap")                    # v on g
    _refused(call(kind=1, v=at(2)), "overlap")                    # v on m
    for bad in ((-1, 0), (1 << 40, 0), (0, -1)):
        assert lib.ktf_optim_workspace_bytes(*bad) == -1


def test_workspace_size_is_its_formula():
    lib = L.load()
    S = lib.ktf_optim_slot_elems()
    al = lambda b: (b + 255) & ~255  # noqa: E731
    for total, n_seg in [(0, 0), (1, 1), (S, 1), (S + 1, 2), (100 * S - 3, 31), (8_200_000, 30), (1 << 30, 1000)]:
        want = al(max(-(-total // S), 1) * 8) + al((5 + n_seg) * 8) + al(max(n_seg, 1) * 8)
        assert lib.ktf_optim_workspace_bytes(total, n_seg) == want > 0, (total, n_seg)


# ----------------------------------------------------------------------------- ktf.optim
def test_kaldi_lr_at_both_ends_and_between():
    lr = ktf.optim.kaldi_lr
    assert lr(0, 100, 0.01, 0.001) == 0.01
    assert abs(lr(100, 100, 0.01, 0.001) - 0.001) <= 1e-15
    assert abs(lr(50, 100, 0.01, 0.0001) - 0.001) <= 1e-15          # the geometric mean half way
    assert lr(3, 7, 0.5, 0.5) == 0.5
    for bad in (dict(num_steps=0), dict(initial=0.0), dict(final=-1.0), dict(initial=float("inf"))):
        with pytest.raises(ValueError):
            lr(**{**dict(step=1, num_steps=10, initial=0.1, final=0.01), **bad})


def test_optimizer_value_errors_name_the_argument():
    w = [torch.nn.Parameter(torch.zeros(4))]
    bad = dict(kind=("kind", "rmsprop"), lr=("lr", -1.0), momentum=("momentum", 1.0), weight_decay=("weight_decay", -0.1),
               betas=("betas", (0.9, 1.0)), eps=("eps", 0.0), max_change=("max_change", -1.0),
               max_change_global=("max_change_global", float("nan")), clip_norm=("clip_norm", float("inf")))
    for name, (match, value) in bad.items():
        with pytest.raises(ValueError, match=match):
            ktf.optim.Optimizer(w, **{**dict(lr=0.1), name: value})
    with pytest.raises(ValueError, match="lr"):
        ktf.optim.Optimizer(w)
    with pytest.raises(ValueError, match="nesterov"):
        ktf.optim.Optimizer(w, lr=0.1, nesterov=True)
    with pytest.raises(ValueError, match="nesterov"):
        ktf.optim.Optimizer(w, kind="adam", lr=0.1, momentum=0.9, nesterov=True)
    with pytest.raises(ValueError, match="betas"):
        ktf.optim.Optimizer(w, kind="adam", lr=0.1, betas=0.9)
    with pytest.raises(ValueError, match="lr of group 1"):
        ktf.optim.Optimizer([dict(params=w), dict(params=[torch.nn.Parameter(torch.zeros(2))], lr=-1.0)], lr=0.1)
    with pytest.raises(ValueError, match="groups"):
        ktf.optim.Optimizer([dict(params=[torch.nn.Parameter(torch.zeros(2))]) for _ in range(9)], lr=0.1)


def test_optimizer_refuses_parameters_off_the_gpu():
    with pytest.raises(ktf.KtfBackendError, match="parameter 0"):
        ktf.optim.Optimizer([torch.nn.Parameter(torch.zeros(4))], lr=0.1)
    with pytest.raises(ktf.KtfBackendError):
        ktf.optim.Optimizer([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))], kind="adam", lr=0.1)
    assert issubclass(ktf.optim.Optimizer, torch.optim.Optimizer)
