"""The 16-bit TDNN gradients without a GPU: the oracle of tests/_tdnn_grad16_ref.py against fp64 torch.autograd of the gather + matmul
restatement fed the operands each mode multiplies, the folded-term magnitudes, the C-ABI of the ktf_grad_tdnn16_* calls (symbols,
every refusal before a launch, the workspace size) and the `gemm=` argument of ktf.autograd."""

import ctypes as C
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

from kaldi_tflite_amd import _lib as L, autograd as A, ops  # noqa: E402
import _tdnn_grad_ref as R  # noqa: E402
import _tdnn_grad16_ref as R16  # noqa: E402
from test_tdnn_grad_cpu import _desc, _refused, _rel, restated_tdnn  # noqa: E402

CASES = R.cases()
F64 = torch.float64
NEW = ("ktf_grad_tdnn16_workspace_bytes", "ktf_grad_tdnn16_data", "ktf_grad_tdnn16_weights")


@pytest.mark.parametrize("mode", R16.MODES)
@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_oracle_equals_autograd_of_the_restatement_on_the_modes_operands(c, mode):
    rng = np.random.default_rng(13)
    lens = R.lens_for(c, 512)
    B, Tm = len(lens), R.T
    valid = c["padding"] == "VALID"
    Tout = R.out_len(Tm, c["context"], c["sub"], valid)[0]
    x = rng.standard_normal((B, Tm, c["din"])).astype(np.float32)
    W = rng.standard_normal((c["units"], len(c["context"]), c["din"])).astype(np.float32)
    g = rng.standard_normal((B, Tout, c["units"])).astype(np.float32)
    want = R16.tdnn_grads16(x, W, g, lens, c["context"], c["sub"], c["padding"], mode)
    xq, Wq, gq = R16.operands(x, W, g, mode)
    if mode == "bf16":                                       # 8 significant bits, and the rounding moved something
        for a, q in ((x, xq), (W, Wq), (g, gq)):
            assert not (q.view(np.uint32) & 0xFFFF).any() and (q != a).any() and (np.abs(q - a) <= 2.0 ** -8 * np.abs(a)).all()
    else:
        assert all(np.array_equal(a, q) for a, q in ((x, xq), (W, Wq), (g, gq)))
    tx, tW = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (xq, Wq))
    tb = torch.zeros(c["units"], dtype=F64, requires_grad=True)
    z = restated_tdnn(tx, tW, tb, lens, c["context"], c["sub"], c["padding"])
    (z * torch.tensor(gq.astype(np.float64))).sum().backward()
    assert _rel(want["dx"], tx.grad.numpy()) <= 1e-12
    assert _rel(want["dW"], tW.grad.numpy()) <= 1e-12
    # the bias gradient is taken of the unrounded g in both modes
    tb.grad = None
    (restated_tdnn(tx.detach(), tW.detach(), tb, lens, c["context"], c["sub"], c["padding"]) * torch.tensor(g.astype(np.float64))).sum().backward()
    assert _rel(want["db"], tb.grad.numpy()) <= 1e-12
    rows = sum(R.out_len(n, c["context"], c["sub"], valid)[0] for n in lens)
    assert (want["db_n"] == rows).all() and (want["dW_n"] == rows).all()
    assert (want["db_S"] >= np.abs(want["db"]) - 1e-9).all()
    for k in ("dx", "dW", "db"):
        assert want[k + "_bound"].shape == want[k].shape and (want[k + "_bound"] >= 0).all()
    # the folded terms: none with VALID padding or in the x3 mode's budget, and only at rows 0 and len - 1 otherwise
    fold = want["dx_S_fold"]
    assert (fold >= 0).all() and (fold <= want["dx_S"] + 1e-9).all()
    if valid or mode == "bf16x3":
        assert not fold.any()
    else:
        for b, n in enumerate(lens):
            assert not fold[b, 1:max(n - 1, 1)].any() and not fold[b, n:].any()
        multi = len(c["context"]) > 1
        assert fold.any() == multi                           # every multi-offset context of the cases clamps at some edge
        if multi:
            b = int(np.argmax(lens))
            assert fold[b, 0].all() and fold[b, lens[b] - 1].all()
            assert ((want["dx_bound"] - (want["dx_n"] + 2) * R16.U32 * want["dx_S"])[b, 0] > 0).all()


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "ktf_grad.h")).read()
    lib = L.load()
    for name in NEW:
        assert name + "(" in hdr and name in L.GRAD_PROTOTYPES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == L.GRAD_PROTOTYPES[name][1]
        assert hasattr(ops, name[len("ktf_"):].replace("_bytes", ""))
    # the fp32 calls' prototypes with the mode in front of the stream (or at the end, for the size)
    for new, old in (("ktf_grad_tdnn16_data", "ktf_grad_tdnn_data"), ("ktf_grad_tdnn16_weights", "ktf_grad_tdnn_weights")):
        assert L.GRAD_PROTOTYPES[new][1] == L.GRAD_PROTOTYPES[old][1][:-1] + [C.c_int32, C.c_void_p]
    assert L.GRAD_PROTOTYPES[NEW[0]][1] == L.GRAD_PROTOTYPES["ktf_grad_tdnn_workspace_bytes"][1] + [C.c_int32]


def test_every_refusal_comes_before_a_launch():
    lib = L.load()
    raw = (C.c_float * 4096)()
    buf = C.c_void_p((C.addressof(raw) + 255) & ~255)      # stands for any aligned non-null device pointer: every refusal comes before a launch
    odd = C.c_void_p(buf.value + 4)
    B, Tm = 2, 10
    good = _desc()
    for gemm in (L.GEMM_BF16, L.GEMM_BF16X3):
        need = lib.ktf_grad_tdnn16_workspace_bytes(B, Tm, C.byref(good), gemm)
        assert need > 0 and need % 256 == 0

        def data(g=buf, ldg=40, B=B, T=Tm, d=good, w=buf, dx=buf, ldx=32, ws=buf, ws_bytes=None, gemm=gemm):
            return lib.ktf_grad_tdnn16_data(g, ldg, B, T, None, None if d is None else C.byref(d), w, dx, ldx, ws, need if ws_bytes is None else ws_bytes,
                                            gemm, None)

        def weights(x=buf, B=B, T=Tm, ldx=32, d=good, g=buf, ldg=40, dw=buf, dbias=buf, ws=buf, ws_bytes=None, gemm=gemm):
            return lib.ktf_grad_tdnn16_weights(x, B, T, ldx, None, None if d is None else C.byref(d), g, ldg, dw, dbias, ws,
                                               need if ws_bytes is None else ws_bytes, gemm, None)

        def size(d=good, gemm=gemm):
            return lib.ktf_grad_tdnn16_workspace_bytes(B, Tm, None if d is None else C.byref(d), gemm)

        def changed(**kw):
            d = _desc()
            for k, v in kw.items():
                setattr(d, k, v)
            return d

        unsorted = _desc()
        unsorted.ctx[0], unsorted.ctx[1] = 2, -1
        for fn in (data, weights, size):
            _refused(fn(d=None), "null")
            _refused(fn(d=changed(gemm=L.GEMM_BF16X3)), "KTF_GEMM_F32")         # the descriptor is the trainable forward's
            _refused(fn(d=changed(gemm=L.GEMM_F16MX)), "KTF_GEMM_F32")
            _refused(fn(d=changed(act=L.ACT_RELU)), "KTF_ACT_NONE")
            _refused(fn(d=changed(x_dtype=L.KTF_BF16)), "KTF_F32")
            _refused(fn(d=unsorted), "ascending")
            _refused(fn(d=changed(nctx=17)), "nctx")
            _refused(fn(d=changed(din_pad=24)), "din_pad")
            _refused(fn(d=changed(subsampling=0)), "subsampling")
            for bad in (L.GEMM_F32, L.GEMM_F16MX, L.GEMM_BF16X4, 99):
                _refused(fn(gemm=bad), "KTF_GEMM_BF16 or KTF_GEMM_BF16X3")
        for fn, ptrs in ((data, ("g", "w", "dx", "ws")), (weights, ("x", "g", "dw", "ws"))):
            for name in ptrs:
                _refused(fn(**{name: None}), "null")
            _refused(fn(ldx=31), "din_pad")
            _refused(fn(ldx=34), "multiple of 4")
            _refused(fn(ldg=39), "units")
            _refused(fn(ws_bytes=need - 1), "workspace")
            _refused(fn(ws=odd), "256-byte")
            _refused(fn(B=-1), "negative size")
            _refused(fn(B=65536), "65535")
            _refused(fn(B=60000, T=1 << 20), "2^31")
        _refused(data(w=odd), "16-byte")
        _refused(data(dx=odd), "16-byte")
        _refused(weights(x=odd), "16-byte")
        _refused(weights(dw=odd), "16-byte")
        assert data(B=0) == 0 and data(T=0) == 0                 # nothing to launch
    # the fp32 calls keep refusing the other modes (their descriptor check is shared)
    d16 = _desc()
    d16.gemm = L.GEMM_BF16
    _refused(lib.ktf_grad_tdnn_workspace_bytes(B, Tm, C.byref(d16)), "KTF_GEMM_F32")


def test_workspace_size_is_positive_aligned_and_that_of_the_fp32_calls():
    lib = L.load()
    d = _desc(units=130, din=30, context=(-2, -1, 0, 1, 2))
    for gemm in (L.GEMM_BF16, L.GEMM_BF16X3):
        for B, T in ((0, 0), (1, 0), (0, 5), (1, 1), (1, 513), (3, 700), (64, 300)):
            n = lib.ktf_grad_tdnn16_workspace_bytes(B, T, C.byref(d), gemm)
            assert n > 0 and n % 256 == 0
            assert n == lib.ktf_grad_tdnn_workspace_bytes(B, T, C.byref(d))      # the same folded rows and slots


def test_gemm_argument_of_autograd():
    x = torch.zeros((1, 4, 8))
    with pytest.raises(ValueError, match="gemm"):
        A.tdnn_affine(x, torch.zeros((3, 1, 8)), None, [0], gemm="x")
    with pytest.raises(ValueError, match="gemm"):
        A.tdnn_affine(x, torch.zeros((3, 1, 8)), None, [0], gemm="f16mx")
    for mode in ("f32", "bf16", "bf16x3"):                   # a known mode gets as far as the device check
        with pytest.raises(L.KtfBackendError):
            A.tdnn_affine(x, torch.zeros((3, 1, 8)), None, [0], gemm=mode)
    import kaldi_tflite_amd as ktf
    Lr, M = ktf.layers, ktf.models
    seq = M.Sequential([M.Input(shape=(None, 24)), Lr.TDNN(16, [-1, 0, 1], name="t1"), Lr.ReLU(),
                        Lr.StatsPooling(0, 0, reduce_time_axis=True, name="pool"), Lr.TDNN(8, [0], name="t2")])
    with pytest.raises(ValueError, match="gemm"):
        A.TrainableSequential(seq, device=torch.device("cpu"), gemm="fp8")
    assert A.TrainableSequential(seq, device=torch.device("cpu")).gemm == "f32"
    net = A.TrainableSequential(seq, device=torch.device("cpu"), gemm="bf16x3")
    assert net.gemm == "bf16x3" and all(p.dtype == torch.float32 for p in net.parameters())
