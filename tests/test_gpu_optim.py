"""The optimiser step kernels (include/ktf_optim.h) on the GPU against the fp64 oracle of tests/_optim_ref.py, and
ktf.optim.Optimizer over them.

Exact inputs (small integers, powers of two) are compared bit for bit with the oracle adding in the order of rule 8. Gaussian
inputs are compared with the oracle whose sums are exact (math.fsum), within (u = 2^-24, e = 2^-53, n the elements of all segments,
n_s those of a segment):
    G        |got - ref| <= n e G           (a sum of n non-negative terms in any order is within (n - 1) e of exact, the exact sum
                                             rounded once within e; the square root halves the relative error and adds e)
    c        |got - ref| <= (n + 2) e c     (one more division)
    sigma_s, N, sigma   relative error <= max_s eps_s + (n_seg + 8) e,  eps_s = (n + 2) e K_s + (n_s + 2) e,
             K_s = lr sqrt(sum (|dd / dghat| |c g|)^2) / N_s: what the error of c makes of d (the oracle's Ns_sens), then the sum over
             the segment; the n_seg + 8 covers the sum over the segments, the square roots and the divisions
    p        |got - ref| <= 2 u (|p| + |a d|)      (one rounding to fp32, doubled; a d is the step itself, as the oracle takes it)
    m, v     |got - ref| <= 2 u (the magnitudes of their terms)
The fp64 differences of the scales (1e-13 of d's terms) are far inside the doubling."""

import functools
import itertools
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
from kaldi_tflite_amd import autograd as A, ops  # noqa: E402
import _optim_ref as R  # noqa: E402
from test_gpu_loss import NET_LENS, UNITS, _problem, _stack  # noqa: E402

pytestmark = pytest.mark.gpu
U, E = 2.0 ** -24, 2.0 ** -53
DEV = "cuda:0"
NAN = float("nan")
GUARD = 64                       # floats of NaN on either side of an arena (a multiple of 4: offset 0 stays 16-byte aligned)
S = R.SLOT
SIZES = (0, 1, 3, S - 1, S, S + 1, 2 * S + 17)
GROUPS = [(0.5, 0.125), (0.25, 0.0)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b, tag):
    assert np.array_equal(_bits(a), _bits(b)), tag


def table(sizes, limits=None):
    """Segments of `sizes` elements, alternating between the two groups; limits: max_change per segment."""
    rows, total = R.layout(sizes)
    return [(b, e, i % 2, 0.0 if limits is None else limits[i]) for i, (b, e) in enumerate(rows)], total


def fill(segs, total, draw):
    """A float32 arena: draw(n) in every segment, NaN in the padding."""
    a = np.full(total, NAN, dtype=np.float32)
    for b, e, _, _ in segs:
        a[b:e] = draw(e - b)
    return a


def on_device(host, offset):
    """host as a 1-D device view `offset` floats off an aligned address, NaN guards on both sides. Returns (view, whole)."""
    whole = torch.full((GUARD + offset + host.size + GUARD,), NAN, dtype=torch.float32, device=DEV)
    view = whole[GUARD + offset:GUARD + offset + host.size]
    view.copy_(torch.as_tensor(host))
    return view, whole


def run_kernels(c, offset=0, **over):
    """One ktf_optim_step of case c on fresh buffers. Returns numpy p, m, v, stats; checks the padding and the guards."""
    kw = {**c["kw"], **over}
    segs, total = c["segs"], c["total"]
    host_t, dev_t = ops.optim_segments(segs, DEV)
    bufs = {k: (on_device(c[k], offset) if c.get(k) is not None else (None, None)) for k in ("p", "g", "m", "v")}
    stats = torch.full((5 + len(segs),), NAN, dtype=torch.float64, device=DEV)
    ws = ops.optim_workspace(total, len(segs), DEV)
    ws.fill_(0xFF)
    ops.optim_step(bufs["p"][0], bufs["g"][0], bufs["m"][0], bufs["v"][0], host_t, dev_t, len(segs), c["groups"], stats=stats, workspace=ws, **kw)
    torch.cuda.synchronize()
    out = dict(stats=stats.cpu().numpy())
    pad = np.ones(total, dtype=bool)
    for b, e, _, _ in segs:
        pad[b:e] = False
    for k, (view, whole) in bufs.items():
        if view is None:
            out[k] = None
            continue
        w = whole.cpu().numpy()
        lo = GUARD + offset
        assert np.isnan(w[:lo]).all() and np.isnan(w[lo + total:]).all(), f"{k}: the guards around the arena were written"
        out[k] = w[lo:lo + total]
        assert np.isnan(out[k][pad]).all(), f"{k}: padding was written"
        if k == "g":
            same_bits(out[k], c[k], "g was written")
    return out


def oracle(c, sums, **over):
    kw = {**c["kw"], **over}
    return R.step(c["p"], c["g"], c.get("m"), c.get("v"), c["segs"], c["groups"], sums=sums, **kw)


# ----------------------------------------------------------------------------- exact inputs: bit for bit
VARIANTS = {
    "sgd": dict(kind="sgd"),
    "sgd-momentum": dict(kind="sgd", momentum=0.5),
    "sgd-nesterov": dict(kind="sgd", momentum=0.5, nesterov=True),
    "sgd-decoupled": dict(kind="sgd", momentum=0.25, decoupled=True),
    "adam": dict(kind="adam", betas=(0.5, 0.75), eps=2.0 ** -10, step=3),
    "adam-decoupled": dict(kind="adam", betas=(0.5, 0.75), eps=2.0 ** -10, step=1, decoupled=True),
}


def exact_case(variant, clip, seg_limit, glob, sizes=SIZES, seed=0):
    """Small integers in p, g, m (and v), powers of two everywhere else: every square and every sum of squares of g, and of d under
    SGD without clipping, is exact in fp64 whatever the order (with clipping c = clip_norm / G is no power of two, and Adam divides:
    there the oracle's sums in the order of rule 8 give the bits). The limits are powers of two far below the norms, so each one
    that is on bites."""
    rng = np.random.default_rng(seed + 1000 * len(sizes))
    ints = lambda n: rng.integers(-8, 9, n)  # noqa: E731
    limits = [(2.0 ** -6 if i % 3 != 2 else 0.0) for i in range(len(sizes))] if seg_limit else None
    segs, total = table(sizes, limits)
    kw = dict(VARIANTS[variant])
    # |g| is about 5 per element: a power of two near sqrt(n) is a few times below G and leaves c large enough for the other limits
    kw.update(clip_norm=2.0 ** (int(np.log2(sum(sizes) + 1)) // 2) if clip else 0.0, max_change_global=2.0 ** -8 if glob else 0.0)
    c = dict(segs=segs, total=total, groups=GROUPS, kw=kw, p=fill(segs, total, ints), g=fill(segs, total, ints))
    has_m = kw["kind"] == "adam" or kw.get("momentum", 0.0) != 0.0
    c["m"] = fill(segs, total, ints) if has_m else None
    c["v"] = fill(segs, total, lambda n: rng.integers(0, 9, n)) if kw["kind"] == "adam" else None
    return c


def check_exact(c, tag):
    want = oracle(c, "kernel")
    for offset in (0, 1):                                  # the 16-byte path and the element-wise one
        got = run_kernels(c, offset)
        for k in ("p", "m", "v"):
            if c[k] is not None:
                same_bits(got[k], want[k], (tag, k, offset))
                assert want["n_terms"] < 100 or not np.array_equal(_bits(got[k]), _bits(c[k])), (tag, k, "nothing moved")
        same_bits(got["stats"], R.stats_vector(want), (tag, "stats", offset))
    return want


@pytest.mark.parametrize("clip,seg_limit,glob", list(itertools.product([False, True], repeat=3)),
                         ids=lambda v: None)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_exact_inputs_equal_the_oracle_bit_for_bit(variant, clip, seg_limit, glob):
    c = exact_case(variant, clip, seg_limit, glob)
    want = check_exact(c, variant)
    # each limit that is on bites, each one that is off reports its neutral values
    assert (want["c"] < 1.0) == clip and (want["G"] > 0.0) == clip
    assert (want["sigma"] < 1.0) == glob and (want["N"] > 0.0) == (seg_limit or glob)
    limited = [i for i, s in enumerate(c["segs"]) if s[3] > 0.0 and s[1] > s[0]]
    assert all(want["sigma_s"][i] < 1.0 for i in limited) and bool(limited) == seg_limit
    assert all(want["sigma_s"][i] == 1.0 for i in range(len(c["segs"])) if i not in limited)
    assert not want["skipped"]


@pytest.mark.parametrize("variant", ["sgd-nesterov", "adam"])
def test_each_segment_alone(variant):
    for n in SIZES:
        c = exact_case(variant, True, True, True, sizes=(n,), seed=n)
        c["segs"] = [(b, e, grp, 2.0 ** -6) for b, e, grp, _ in c["segs"]]
        want = check_exact(c, (variant, n))
        assert want["n_terms"] == n and (want["sigma_s"][0] < 1.0) == (n > 0)


def test_arrays_a_call_does_not_use_are_not_looked_at():
    """Rules 3 and 14: without momentum m may be NULL or lie anywhere, p and g included; under SGD the same holds for v. The call
    is accepted, gives the bits of the call without them and leaves them alone."""
    c = exact_case("sgd", True, True, True)
    want = oracle(c, "kernel")
    host_t, dev_t = ops.optim_segments(c["segs"], DEV)

    def run(m_is, v_is):
        p, g = on_device(c["p"], 0)[0], on_device(c["g"], 0)[0]
        pick = {"none": None, "p": p, "g": g}
        stats = torch.full((5 + len(c["segs"]),), NAN, dtype=torch.float64, device=DEV)
        ops.optim_step(p, g, pick[m_is], pick[v_is], host_t, dev_t, len(c["segs"]), c["groups"], stats=stats, **c["kw"])
        torch.cuda.synchronize()
        same_bits(g.cpu().numpy(), c["g"], ("g", m_is, v_is))
        same_bits(p.cpu().numpy(), want["p"], ("p", m_is, v_is))
        same_bits(stats.cpu().numpy(), R.stats_vector(want), ("stats", m_is, v_is))

    for m_is, v_is in (("none", "none"), ("p", "none"), ("g", "p"), ("none", "g")):
        run(m_is, v_is)
    # with momentum the same m is an overlap, and refused
    p, g = on_device(c["p"], 0)[0], on_device(c["g"], 0)[0]
    with pytest.raises(ValueError, match="overlap"):
        ops.optim_step(p, g, g, None, host_t, dev_t, len(c["segs"]), c["groups"], **{**c["kw"], "momentum": 0.5})
    same_bits(p.cpu().numpy(), c["p"], "p after the refusal")


# ----------------------------------------------------------------------------- Gaussian inputs: within the bounds
@functools.lru_cache(maxsize=None)
def gaussian_case(variant):
    """Inputs and their exact-sum oracle, computed once and shared (read-only)."""
    rng = np.random.default_rng(77)
    normal = lambda n: rng.standard_normal(n).astype(np.float32)  # noqa: E731
    segs, total = table(SIZES)
    kw = dict(VARIANTS[variant])
    if kw["kind"] == "adam":
        kw.update(betas=(0.9, 0.999), eps=1e-8, step=7)
    else:
        kw.update(momentum=0.9 if kw.get("momentum") else 0.0)
    c = dict(segs=segs, total=total, groups=[(0.01, 1e-3), (0.003, 0.0)], kw=kw, p=fill(segs, total, normal), g=fill(segs, total, normal))
    has_m = kw["kind"] == "adam" or kw["momentum"] != 0.0
    c["m"] = fill(segs, total, lambda n: 0.3 * normal(n)) if has_m else None
    c["v"] = fill(segs, total, lambda n: np.abs(normal(n)) * 0.5) if kw["kind"] == "adam" else None
    free = oracle(c, "exact", clip_norm=1e30, max_change_global=1e30)         # the norms with no limit biting
    c["segs"] = [(b, e, grp, (0.5 * free["Ns"][i] if i % 3 != 2 else 0.0)) for i, (b, e, grp, _) in enumerate(segs)]
    kw.update(clip_norm=0.75 * free["G"], max_change_global=0.25 * free["N"])
    c["want"] = oracle(c, "exact")
    assert c["want"]["c"] < 1.0 and c["want"]["sigma"] < 1.0 and (c["want"]["sigma_s"] < 1.0).any()
    return c


def check_bounds(got, want, c, tag):
    n, n_seg = want["n_terms"], len(c["segs"])
    st, ref = got["stats"], R.stats_vector(want)
    worst = {}

    def within(name, err, bound):
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))) if np.size(err) else 0.0
        worst[name] = ratio
        assert ratio <= 1.0, (tag, name, ratio)

    within("G", abs(st[0] - ref[0]), n * E * ref[0])
    within("c", abs(st[1] - ref[1]), (n + 2) * E * ref[1])
    sizes = np.array([e - b for b, e, _, _ in c["segs"]], dtype=np.float64)
    K = np.where(want["Ns"] > 0, want["Ns_sens"] / np.where(want["Ns"] > 0, want["Ns"], 1.0), 0.0)
    eps = float(np.max((n + 2) * E * K + (sizes + 2) * E)) + (n_seg + 8) * E
    within("N", abs(st[2] - ref[2]), eps * ref[2])
    within("sigma", abs(st[3] - ref[3]), eps * ref[3])
    within("sigma_s", np.abs(st[5:] - ref[5:]), eps * ref[5:])
    assert st[4] == ref[4] == 0.0
    live = np.zeros(c["total"], dtype=bool)
    for b, e, _, _ in c["segs"]:
        live[b:e] = True
    for k in ("p", "m", "v"):
        if c[k] is not None:
            within(k, np.abs(got[k][live].astype(np.float64) - want[k][live]), 2 * U * want[k + "_mag"][live])
    print(f"{tag}: worst |err| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("offset", [0, 1], ids=["16-byte", "element-wise"])
@pytest.mark.parametrize("variant", ["sgd", "sgd-nesterov", "sgd-decoupled", "adam", "adam-decoupled"])
def test_gaussian_inputs_within_the_bounds(variant, offset):
    c = gaussian_case(variant)
    check_bounds(run_kernels(c, offset), c["want"], c, f"{variant} offset {offset}")


@pytest.mark.parametrize("variant", ["sgd-nesterov", "adam"])
def test_a_segment_of_more_slots_than_a_wave_has_lanes(variant):
    """70 slots: lanes 0 to 5 of the finalize wave add two slots each. Gaussian inputs against the oracle adding in the order of
    rule 8: the same bits, sums included."""
    rng = np.random.default_rng(9)
    normal = lambda n: rng.standard_normal(n).astype(np.float32)  # noqa: E731
    segs, total = table((69 * S + 5, 3), [0.01, 0.0])
    kw = dict(VARIANTS[variant])
    kw.update(clip_norm=100.0, max_change_global=0.005)
    c = dict(segs=segs, total=total, groups=[(0.01, 1e-3), (0.003, 0.0)], kw=kw, p=fill(segs, total, normal), g=fill(segs, total, normal),
             m=fill(segs, total, normal))
    c["v"] = fill(segs, total, lambda n: np.abs(normal(n))) if kw["kind"] == "adam" else None
    want = check_exact(c, variant)
    assert want["c"] < 1.0 and want["sigma_s"][0] < 1.0 and want["sigma"] < 1.0


# ----------------------------------------------------------------------------- the same bits, the guard
@pytest.mark.parametrize("variant", ["sgd-nesterov", "adam"])
def test_two_calls_and_two_paths_give_the_same_bits(variant):
    c = gaussian_case(variant)
    a, b, other = run_kernels(c, 0), run_kernels(c, 0), run_kernels(c, 1)
    for k in ("p", "m", "v", "stats"):
        if a[k] is not None:
            same_bits(a[k], b[k], (k, "second call"))
            same_bits(a[k], other[k], (k, "element-wise path"))


@pytest.mark.parametrize("bad", [NAN, float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("limit", ["clip", "segment", "global"])
@pytest.mark.parametrize("variant", ["sgd-nesterov", "adam"])
def test_a_non_finite_gradient_changes_nothing(variant, limit, bad):
    c = dict(gaussian_case(variant))
    c["g"] = c["g"].copy()
    b, e, _, _ = c["segs"][-1]
    c["g"][e - 1] = bad                                    # one element, the last of the table
    kw = dict(clip_norm=0.0, max_change_global=0.0)
    if limit == "clip":
        kw["clip_norm"] = 1.0
    elif limit == "global":
        kw["max_change_global"] = 1.0
    if limit != "segment":
        c["segs"] = [(b, e, grp, 0.0) for b, e, grp, _ in c["segs"]]
    for offset in (0, 1):
        got = run_kernels(c, offset, **kw)
        assert got["stats"][4] == 1.0
        for k in ("p", "m", "v"):
            if c[k] is not None:
                same_bits(got[k], c[k], (k, offset))
    # no limit, no guard: the element goes into p (documented)
    c["segs"] = [(b, e, grp, 0.0) for b, e, grp, _ in c["segs"]]
    got = run_kernels(c, 0, clip_norm=0.0, max_change_global=0.0)
    assert got["stats"][4] == 0.0 and not np.isfinite(got["p"][e - 1]) and np.isfinite(got["p"][b:e - 1]).all()


def test_a_device_table_that_is_not_the_host_table_is_clamped():
    """Rule 13: a device table with wild entries gives wrong values inside the arenas, nothing outside them."""
    c = exact_case("sgd-momentum", True, True, True)
    total = c["total"]
    wild = [(0, 1 << 50, 7, 1.0), (-(1 << 40), 5, -3, 1.0), (S + 3, total + 9, 1, 1.0)]
    host_t, _ = ops.optim_segments(c["segs"][:3], DEV)
    _, dev_t = ops.optim_segments(wild, DEV)
    bufs = {k: on_device(np.nan_to_num(c[k]), 0) for k in ("p", "g", "m")}
    ops.optim_step(bufs["p"][0], bufs["g"][0], bufs["m"][0], None, host_t, dev_t, 3, c["groups"], **c["kw"])
    torch.cuda.synchronize()
    for k, (view, whole) in bufs.items():
        w = whole.cpu().numpy()
        assert np.isnan(w[:GUARD]).all() and np.isnan(w[GUARD + total:]).all(), k


# ----------------------------------------------------------------------------- ktf.optim.Optimizer
def _params(seed=5, shapes=((3, 5), (S + 1,), (7,), (2, 3, 4))):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in shapes]


def _set_grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad.copy_(torch.randn(p.shape, generator=g))


def _direct(opt, groups=None, step=None):
    """What one ops.optim_step gives from copies of the optimiser's arenas, with its own table: (p, m, v) as numpy."""
    p, g = opt._p.clone(), opt._g.clone()
    m, v = (None if t is None else t.clone() for t in (opt._m, opt._v))
    groups = groups or [(gr["lr"], gr["weight_decay"]) for gr in opt.param_groups]
    ops.optim_step(p, g, m, v, opt._segs_host, opt._segs_dev, len(opt._rows), groups, opt.kind, momentum=opt.momentum, nesterov=opt.nesterov,
                   betas=opt.betas, eps=opt.eps, step=opt._step + 1 if step is None else step, decoupled=opt.decoupled, clip_norm=opt.clip_norm,
                   max_change_global=opt.max_change_global)
    return tuple(None if t is None else t.cpu().numpy() for t in (p, m, v))


def _arenas(opt):
    return tuple(None if t is None else t.cpu().numpy() for t in (opt._p, opt._m, opt._v))


def _same_arenas(a, b, tag):
    for x, y, k in zip(a, b, "pmv"):
        assert (x is None) == (y is None)
        if x is not None:
            same_bits(x, y, (tag, k))


def test_construction_keeps_values_and_the_forward_pass():
    torch.manual_seed(3)
    net = A.TrainableSequential(_stack(), fused_norm=True).train()
    feats, _ = _problem()
    tf_, tl = torch.as_tensor(feats, device=DEV), torch.as_tensor(NET_LENS, device=DEV)
    before = [p.detach().cpu().numpy().copy() for p in net.parameters()]
    with torch.no_grad():
        out0 = net.eval()(tf_, tl).cpu().numpy()
    opt = ktf.optim.Optimizer(net.parameters(), lr=0.05, momentum=0.9)
    lo, hi = opt._p.data_ptr(), opt._p.data_ptr() + 4 * opt._total
    for p, b, (begin, end, _, _) in zip(net.parameters(), before, opt._rows):
        same_bits(p.detach().cpu().numpy(), b, "parameter")
        assert p.data_ptr() == lo + 4 * begin and begin % S == 0 and end - begin == p.numel() and lo <= p.data_ptr() < hi
        assert p.grad is not None and p.grad.data_ptr() == opt._g.data_ptr() + 4 * begin and not p.grad.any()
    with torch.no_grad():
        same_bits(net(tf_, tl).cpu().numpy(), out0, "forward")
    # .grad views survive backward(): autograd accumulates in place
    views = [p.grad for p in net.parameters()]
    net.train()(tf_, tl).square().sum().backward()
    assert all(p.grad is v for p, v in zip(net.parameters(), views)) and opt._g.any()
    opt.zero_grad()
    assert not opt._g.any() and all(p.grad is v for p, v in zip(net.parameters(), views))
    with pytest.raises(ValueError, match="set_to_none"):
        opt.zero_grad(set_to_none=True)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_step_is_the_direct_call(kind):
    params = _params()
    opt = ktf.optim.Optimizer([dict(params=params[:2], max_change=0.05), dict(params=params[2:], lr=0.02, weight_decay=0.01)], kind=kind, lr=0.1,
                              momentum=0.9 if kind == "sgd" else 0.0, nesterov=kind == "sgd", clip_norm=50.0, max_change_global=0.08)
    assert [r[2:] for r in opt._rows] == [(0, 0.05), (0, 0.05), (1, 0.0), (1, 0.0)]
    for step in (1, 2):
        _set_grads(params, 10 + step)
        want = _direct(opt)
        opt.step()
        _same_arenas(_arenas(opt), want, (kind, step))
    st = opt.stats.cpu().numpy()
    assert st.shape == (5 + 4,) and st[0] > 50.0 and st[1] < 1.0 and st[4] == 0.0 and (st[5:7] < 1.0).all() and (st[7:] == 1.0).all()
    # a replaced .grad is copied in and the view restored; a missing one is refused and nothing moves
    mine = torch.full_like(params[1], 0.5)
    params[1].grad = mine
    p, g = opt._p.clone(), opt._g.clone()
    g[opt._rows[1][0]:opt._rows[1][1]] = 0.5
    m, v = (None if t is None else t.clone() for t in (opt._m, opt._v))
    ops.optim_step(p, g, m, v, opt._segs_host, opt._segs_dev, 4, [(0.1, 0.0), (0.02, 0.01)], kind, momentum=opt.momentum, nesterov=opt.nesterov,
                   betas=opt.betas, eps=opt.eps, step=3, clip_norm=50.0, max_change_global=0.08)
    opt.step()
    _same_arenas(_arenas(opt), tuple(None if t is None else t.cpu().numpy() for t in (p, m, v)), "replaced grad")
    assert params[1].grad is not mine and params[1].grad.data_ptr() == opt._g.data_ptr() + 4 * opt._rows[1][0]
    params[2].grad = None
    before = _arenas(opt)
    with pytest.raises(ValueError, match="parameter 2"):
        opt.step()
    _same_arenas(_arenas(opt), before, "refused step")
    # ... and so does a step the library refuses: neither counts towards Adam's bias correction
    params[2].grad = opt._gviews[2]
    opt.clip_norm = -1.0
    with pytest.raises(ValueError, match="clip_norm"):
        opt.step()
    _same_arenas(_arenas(opt), before, "step refused by the library")
    assert opt._step == 3
    opt.clip_norm = 50.0
    opt.step()
    assert opt._step == 4
    with pytest.raises(ValueError, match="fixed at construction"):
        opt.add_param_group(dict(params=_params(shapes=((2,),))))


def test_an_lr_scheduler_changes_the_next_step():
    params = _params()
    opt = ktf.optim.Optimizer(params, lr=0.5, momentum=0.5)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda epoch: 0.5 ** epoch)
    for step, lr in ((1, 0.5), (2, 0.25), (3, 0.125)):
        assert opt.param_groups[0]["lr"] == lr
        _set_grads(params, 20 + step)
        want = _direct(opt, groups=[(lr, 0.0)])
        other = _direct(opt, groups=[(0.5, 0.0)])
        opt.step()
        sched.step()
        _same_arenas(_arenas(opt), want, ("scheduled", step))
        assert (step == 1) == np.array_equal(_bits(want[0]), _bits(other[0]))
    opt.param_groups[0]["lr"] = ktf.optim.kaldi_lr(1, 2, 0.01, 0.0001)
    assert abs(opt.param_groups[0]["lr"] - 0.001) < 1e-15


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_state_dict_resume_reproduces_the_following_steps(kind):
    kw = dict(kind=kind, lr=0.1, momentum=0.9 if kind == "sgd" else 0.0, weight_decay=0.01, clip_norm=1.0, max_change=0.05)
    a = _params()
    full = ktf.optim.Optimizer(a, **kw)
    snap = {}
    for step in (1, 2, 3, 4):
        _set_grads(a, 30 + step)
        full.step()
        snap[step] = _arenas(full)
    b = _params()
    first = ktf.optim.Optimizer(b, **kw)
    for step in (1, 2):
        _set_grads(b, 30 + step)
        first.step()
    sd = first.state_dict()
    assert sd["ktf"]["step"] == 2 and sd["param_groups"][0]["lr"] == 0.1
    c = [torch.nn.Parameter(p.detach().clone()) for p in b]
    resumed = ktf.optim.Optimizer(c, **{**kw, "lr": 0.7})
    resumed.load_state_dict(sd)
    assert resumed.param_groups[0]["lr"] == 0.1 and resumed._step == 2
    for step in (3, 4):
        _set_grads(c, 30 + step)
        resumed.step()
        _same_arenas(_arenas(resumed), snap[step], ("resumed", step))
    with pytest.raises(ValueError, match="another set of parameters"):
        ktf.optim.Optimizer(_params(shapes=((4,),)), **kw).load_state_dict(sd)
    # the limits live in the segment table of the optimiser that loads: a state saved under other limits is refused, not half applied
    other = ktf.optim.Optimizer(_params(), **{**kw, "max_change": 0.5})
    with pytest.raises(ValueError, match="max_change"):
        other.load_state_dict(sd)
    assert other.param_groups[0]["max_change"] == 0.5 and other._step == 0


# ----------------------------------------------------------------------------- end to end
def test_training_the_network_with_ktf_optim():
    """The five-GEMM network of test_gpu_loss.py under an 8-class AAM head: the first step from the GPU's own gradients against the
    oracle within the Gaussian bounds, with a max-change limit of half the first step's unlimited norm; then 30 steps."""
    seq = _stack()
    feats, labels = _problem()
    torch.manual_seed(5)
    net = A.TrainableSequential(seq, fused_norm=True).train()
    head = A.ClassifierHead(UNITS, 8, kind="aam", margin=0.2, scale=16.0, device=DEV)
    tf_, tl, ty = torch.as_tensor(feats, device=DEV), torch.as_tensor(NET_LENS, device=DEV), torch.as_tensor(labels, device=DEV)
    opt = ktf.optim.Optimizer([dict(params=list(net.parameters())), dict(params=list(head.parameters()), weight_decay=1e-4)], lr=0.05,
                              momentum=0.5, clip_norm=100.0)
    opt.zero_grad()
    loss, _ = head(net(tf_, tl), ty)
    loss.backward()
    segs = [tuple(r) for r in opt._rows]
    c = dict(segs=segs, total=opt._total, groups=[(0.05, 0.0), (0.05, 1e-4)], p=opt._p.cpu().numpy(), g=opt._g.cpu().numpy(),
             m=opt._m.cpu().numpy(), v=None, kw=dict(kind="sgd", momentum=0.5, clip_norm=100.0))
    assert np.abs(c["g"]).max() > 0
    free = oracle(c, "exact", max_change_global=1e30)
    limit = 0.5 * free["N"]
    assert limit > 0
    opt.max_change_global = c["kw"]["max_change_global"] = limit
    want = oracle(c, "exact")
    opt.step()
    st = opt.stats.cpu().numpy()
    assert st[3] < 1.0 and st[4] == 0.0                      # the limit bit on the first step
    check_bounds(dict(stats=st, p=opt._p.cpu().numpy(), m=opt._m.cpu().numpy(), v=None), want, c, "first step")

    losses = [loss.item()]
    for _ in range(30):
        opt.zero_grad()
        step_loss, _ = head(net(tf_, tl), ty)
        step_loss.backward()
        opt.step()
        losses.append(step_loss.item())
    print(f"loss: first {losses[0]:.4f}, after 30 steps {losses[-1]:.4f}; sigma of the last step {opt.stats[3].item():.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]

    assert net.export() is seq
    it = iter(net.params)
    for l in seq.layers:
        if isinstance(l, ktf.layers.TDNN):
            kernel, bias = l.get_weights()
            same_bits(kernel[0].transpose(2, 0, 1), next(it).detach().cpu().numpy(), l.name)
            same_bits(bias, next(it).detach().cpu().numpy(), l.name)
        elif isinstance(l, ktf.layers.BatchNorm):
            same_bits(l.get_weights()[0], next(it).detach().cpu().numpy(), l.name)
    for p, (begin, end, _, _) in zip(list(net.parameters()) + list(head.parameters()), opt._rows):
        assert p.data_ptr() == opt._p.data_ptr() + 4 * begin
