"""ReLU + BatchNorm in training without a GPU: the fp64 oracle (tests/_norm_ref.py) against fp64 torch.autograd of
autograd.batch_norm(torch.relu(z), ...), the C-ABI of include/ktf_norm.h (symbols, argument refusals before any launch, the
workspace size) and the argument checks of ktf.autograd.relu_batch_norm / TrainableSequential(fused_norm=)."""

import ctypes as C
import itertools
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
from kaldi_tflite_amd import _lib as L, autograd as A  # noqa: E402
import _norm_ref as N  # noqa: E402

F64 = torch.float64


def _close(got, want, what):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    scale = max(float(np.abs(np.asarray(want)).max()), 1.0)
    assert err <= 1e-12 * scale, (what, err, scale)


# ----------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("training,relu,with_lens", list(itertools.product([True, False], repeat=3)))
def test_oracle_equals_autograd_of_the_torch_composition(training, relu, with_lens):
    rng = np.random.default_rng(7)
    B, T, D = 4, 11, 6
    lens = [11, 0, 1, 7] if with_lens else None
    z = rng.standard_normal((B, T, D)) + 0.3
    z[:, :, 2] = -np.abs(z[:, :, 2])                              # under relu: a column of zeros, variance 0
    z[0, 0, 3] = 0.0                                              # relu's gradient at 0 is 0
    gy = rng.standard_normal((B, T, D))
    gamma = rng.uniform(0.5, 2.0, D)
    mm0, mv0 = rng.standard_normal(D), rng.uniform(0.5, 2.0, D)
    momentum, eps = 0.9, 1e-3

    f = N.forward(z, lens, relu, training, gamma, mm0, mv0, momentum, eps)
    g = N.backward(gy, z, lens, relu, training, gamma, f["mean"], f["invstd"])

    tz = torch.tensor(z, dtype=F64, requires_grad=True)
    tg = torch.tensor(gamma, dtype=F64, requires_grad=True)
    mm, mv = torch.tensor(mm0, dtype=F64), torch.tensor(mv0, dtype=F64)
    tl = None if lens is None else torch.tensor(lens, dtype=torch.int32)
    y = A.batch_norm(torch.relu(tz) if relu else tz, tl, mm, mv, tg, momentum=momentum, epsilon=eps, training=training)
    (y * torch.tensor(gy)).sum().backward()

    _close(f["y"], y.detach().numpy(), "y")
    _close(g["dz"], tz.grad.numpy(), "dz")
    _close(g["dgamma"], tg.grad.numpy(), "dgamma")
    _close(f["moving_mean"], mm.numpy(), "moving_mean")
    _close(f["moving_var"], mv.numpy(), "moving_var")
    if not training:
        assert np.array_equal(f["moving_mean"], mm0) and np.array_equal(f["moving_var"], mv0)
    # the magnitudes dominate the values they bound; invalid rows are zero
    assert (f["y_mag"] >= np.abs(f["y"]) - 1e-12).all() and (g["dz_mag"] >= np.abs(g["dz"]) - 1e-12).all()
    assert (g["dgamma_abs"] >= np.abs(g["dgamma"]) - 1e-12).all()
    for b, n in enumerate(lens or []):
        assert not f["y"][b, n:].any() and not g["dz"][b, n:].any()
    assert f["n"] == (sum(lens) if lens else B * T)
    if relu:
        assert not g["dz"][0, 0, 3]


def test_oracle_corner_counts():
    z = np.array([[[-2.0, 3.0]]])
    f = N.forward(z, None, True, True, [1.0, 1.0], [0.0, 0.0], [1.0, 1.0], 0.5, 0.25)            # n = 1
    assert f["n"] == 1 and np.array_equal(f["mean"], [0.0, 3.0]) and np.array_equal(f["invstd"], [2.0, 2.0]) and not f["y"].any()
    assert np.array_equal(f["moving_mean"], [0.0, 1.5]) and np.array_equal(f["moving_var"], [0.5, 0.5])
    e = N.forward(z, [0], True, True, [1.0, 1.0], [5.0, 5.0], [1.0, 1.0], 0.5, 0.25)              # n = 0
    assert e["n"] == 0 and not e["y"].any() and not e["invstd"].any() and np.array_equal(e["moving_mean"], [5.0, 5.0])
    g = N.backward(np.ones((1, 1, 2)), z, [0], True, True, [1.0, 1.0], e["mean"], e["invstd"])
    assert not g["dz"].any() and not g["dgamma"].any()


# ----------------------------------------------------------------------------- the C-ABI
def test_header_symbols_are_the_norm_prototypes_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ktf_norm.h")).read()
    declared = set(re.findall(r"\b(ktf_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.NORM_PROTOTYPES), declared ^ set(L.NORM_PROTOTYPES)
    assert all(n.startswith("ktf_norm_") for n in declared)
    assert "ktf_grad_" not in hdr
    lib = L.load()
    for name in declared:
        assert hasattr(lib, name), name
    others = set(L.PROTOTYPES) | set(L.AUGMENT_PROTOTYPES) | set(L.RESAMPLE_PROTOTYPES) | set(L.GRAD_PROTOTYPES)
    assert not set(L.NORM_PROTOTYPES) & others
    for other in ("ktf_hip.h", "ktf_augment.h", "ktf_resample.h", "ktf_grad.h"):
        assert "ktf_norm_" not in open(os.path.join(ROOT, "include", other)).read()
    assert len(L.PROTOTYPES) == 120 and lib.ktf_version() == 117
    assert lib.ktf_norm_slot_rows() == 128
    assert int(re.search(r"#define KTF_NORM_SLOT_ROWS (\d+)", hdr).group(1)) == 128


def _refused(rc, text):
    assert rc == -1, rc
    assert text in L.last_error(), L.last_error()
    with pytest.raises(ValueError):
        L.check(rc, "x")


def test_argument_checks_without_gpu():
    lib = L.load()
    raw = (C.c_float * 8192)()
    buf = C.c_void_p((C.addressof(raw) + 255) & ~255)      # stands for any aligned non-null device pointer: every refusal comes before a launch
    far = C.c_void_p(buf.value + 16384)                    # a second one that does not overlap B * T * ld floats at buf
    gyp = C.c_void_p(buf.value + 8192)
    odd = C.c_void_p(buf.value + 4)
    B, Tm, D = 2, 10, 8
    need = lib.ktf_norm_workspace_bytes(B, Tm, D)
    assert need > 0

    def fwd(z=buf, ldz=8, B=B, T=Tm, D=D, gamma=buf, mm=buf, mv=buf, momentum=0.9, eps=1e-3, y=far, ldy=8, saved=buf, ws=buf, ws_bytes=None):
        return lib.ktf_norm_relu_bn_forward(z, ldz, B, T, D, None, 1, 1, gamma, mm, mv, momentum, eps, y, ldy, saved, ws,
                                            need if ws_bytes is None else ws_bytes, None)

    def bwd(gy=gyp, ldg=8, z=buf, ldz=8, B=B, T=Tm, D=D, gamma=buf, saved=buf, dz=far, ld_dz=8, dgamma=buf, ws=buf, ws_bytes=None):
        return lib.ktf_norm_relu_bn_backward(gy, ldg, z, ldz, B, T, D, None, 1, 1, gamma, saved, dz, ld_dz, dgamma, ws,
                                             need if ws_bytes is None else ws_bytes, None)

    for name in ("z", "gamma", "mm", "mv", "y", "saved", "ws"):
        _refused(fwd(**{name: None}), "null")
    for name in ("gy", "z", "gamma", "saved", "dz", "ws"):
        _refused(bwd(**{name: None}), "null")
    for fn, lds in ((fwd, ("ldz", "ldy")), (bwd, ("ldg", "ldz", "ld_dz"))):
        _refused(fn(D=0), "below 1")
        _refused(fn(D=-3), "below 1")
        for ld in lds:
            _refused(fn(**{ld: 7}), "leading dimension")
        _refused(fn(ws_bytes=need - 1), "workspace")
        _refused(fn(ws=odd), "256-byte")
        _refused(fn(B=-1), "negative size")
        _refused(fn(T=-1), "negative size")
        _refused(fn(B=1 << 16, T=1 << 15), "2^31")
        _refused(fn(B=1 << 40, T=1 << 40), "2^31")
    _refused(fwd(eps=0.0), "eps")
    _refused(fwd(eps=-1e-3), "eps")
    _refused(fwd(eps=float("nan")), "eps")
    _refused(fwd(momentum=-0.01), "momentum")
    _refused(fwd(momentum=1.01), "momentum")
    _refused(fwd(y=buf), "overlaps z")
    _refused(fwd(y=C.c_void_p(buf.value + 4 * (B * Tm * 8 - 1))), "overlaps z")       # the last float of z
    _refused(bwd(dz=buf), "overlaps")
    _refused(bwd(dz=gyp), "overlaps")
    for bad in ((-1, 1, 1), (1, -1, 1), (1, 1, 0), (1 << 16, 1 << 15, 1)):
        assert lib.ktf_norm_workspace_bytes(*bad) == -1


def test_workspace_size_is_its_formula():
    lib = L.load()
    slot = lib.ktf_norm_slot_rows()
    al = lambda b: (b + 255) & ~255  # noqa: E731
    for B, T, D in [(0, 0, 1), (0, 5, 3), (1, 1, 1), (1, slot, 23), (1, slot + 1, 23), (5, 90, 512), (64, 300, 1500), (1, 64, 512)]:
        nslots = max(-(-(B * T) // slot), 1)
        want = al(nslots * 2 * D * 8) + al((2 * D + 1) * 8)
        assert lib.ktf_norm_workspace_bytes(B, T, D) == want > 0, (B, T, D)


# ----------------------------------------------------------------------------- ktf.autograd
def test_relu_batch_norm_refuses_cpu_tensors():
    z, v = torch.zeros((1, 4, 8)), torch.ones(8)
    with pytest.raises(ktf.KtfBackendError):
        A.relu_batch_norm(z, None, torch.zeros(8), v, v, training=True)
    with pytest.raises(ktf.KtfBackendError):
        A.relu_batch_norm(torch.zeros((4, 8)), None, torch.zeros(8), v, v, relu=False)


def test_fused_norm_must_be_a_bool_and_changes_no_name():
    Lr, M = ktf.layers, ktf.models
    cpu = torch.device("cpu")

    def stack():
        return M.Sequential([M.Input(shape=(None, 24)), Lr.TDNN(16, [-1, 0, 1], activation="relu", name="t1"), Lr.BatchNorm(name="b1"),
                             Lr.StatsPooling(0, 0, reduce_time_axis=True, name="pool"), Lr.TDNN(8, [0], name="t2"), Lr.ReLU(),
                             Lr.BatchNorm(name="b2")])
    for bad in (1, 0, "yes", None, "True"):
        with pytest.raises(ValueError, match="fused_norm"):
            A.TrainableSequential(stack(), device=cpu, fused_norm=bad)
    plain, fused = A.TrainableSequential(stack(), device=cpu), A.TrainableSequential(stack(), device=cpu, fused_norm=True)
    assert plain.fused_norm is False and fused.fused_norm is True
    assert list(plain.state_dict()) == list(fused.state_dict())
    assert [tuple(p.shape) for p in plain.parameters()] == [tuple(p.shape) for p in fused.parameters()]
