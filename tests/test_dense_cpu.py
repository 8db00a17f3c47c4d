"""The dense affine of the classification head without a GPU: the C-ABI of include/ktf_dense.h (symbols, every refusal of rule 8
before any launch, the workspace size) and the host side of ktf.autograd.dense_affine / ClassifierHead(affine=)."""

import ctypes as C
import os
import re

import pytest
import torch

import kaldi_tflite_amd as ktf                                         # (tests/conftest.py puts the package and tests/ on sys.path)
from kaldi_tflite_amd import _lib as L, autograd as A
from test_loss_cpu import _refused

M, N, D = 5, 6, 7
_RAW = (C.c_float * 16384)()
_BASE = (C.addressof(_RAW) + 255) & ~255                  # stands for aligned device memory: every refusal comes before a launch


def at(floats):
    return C.c_void_p(_BASE + 4 * floats)


X, W, Z, BIAS, WS = at(0), at(1024), at(2048), at(3072), at(4096)      # x / dx, w / dw, z / g, bias / dbias, workspace (ld = 8)
BIG = 1 << 31
ARGS = {"forward": "x ldx w ldw bias M N D gemm z ldz", "grad_data": "g ldg w ldw M N D gemm dx lddx ws ws_bytes",
        "grad_weights": "g ldg x ldx M N D gemm dw lddw dbias"}
OPERANDS = {n: ([k for k in a.split() if k in ("x", "w", "z", "g", "dx", "dw", "ws")], [k for k in a.split() if k.startswith("ld")])
            for n, a in ARGS.items()}                     # name -> (required pointers, leading dimensions)


def call(name, **kw):
    a = dict(dict(x=X, w=W, bias=BIAS, g=Z, z=Z, dx=X, dw=W, dbias=BIAS, ws=WS, ws_bytes=256, M=M, N=N, D=D, gemm=0), **kw)
    return getattr(L.load(), "ktf_dense_" + name)(*[a.get(k, 8) for k in ARGS[name].split()], None)     # every leading dimension is 8


REFUSALS = [(n, {p: None}, "null") for n, (ptrs, _) in OPERANDS.items() for p in ptrs]
REFUSALS += [(n, {"gemm": bad}, "gemm") for n in OPERANDS for bad in (-1, 3, 5)]
REFUSALS += [(n, bad, "are required") for n in OPERANDS for bad in (dict(M=-1), dict(N=0), dict(D=0))]
REFUSALS += [(n, dict({ld: BIG for ld in lds}, **{dim: BIG}), "2^31") for n, (_, lds) in OPERANDS.items() for dim in ("M", "N", "D")]
REFUSALS += [(n, {ld: bad}, text) for n, (_, lds) in OPERANDS.items() for ld in lds for bad, text in ((5, "below the row length"), (BIG, "2^31"))]
REFUSALS += [("forward", dict(N=2097121, ldz=2097121), "above"), ("grad_weights", dict(N=2097121, ldg=2097121), "above"),       # grids
             ("grad_data", dict(M=2097121), "above"), ("grad_data", dict(N=65535 * 256 + 1, ldg=1 << 30), "slots"),
             ("grad_data", dict(M=1 << 20, lddx=1 << 18), "2^38"),
             ("grad_data", dict(ws_bytes=255), "workspace"), ("grad_data", dict(ws=at(4097)), "256-byte"),
             # an output on the last element of an input, or on another output
             ("forward", dict(z=at((M - 1) * 8 + D - 1)), "overlaps"), ("forward", dict(z=at(3072 + N - 1)), "overlaps"),
             ("grad_data", dict(dx=at(1024 + (N - 1) * 8 + D - 1)), "overlaps"), ("grad_data", dict(dx=at(4096 + 63)), "overlaps"),
             ("grad_weights", dict(dw=at(2048 + (M - 1) * 8 + N - 1)), "overlaps"), ("grad_weights", dict(dbias=at(1024 + N * 8 - 1)), "overlaps")]


def test_header_symbols_are_the_dense_prototypes():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ktf_dense.h")).read()
    protos = re.findall(r"^(?:int|int32_t|int64_t) (ktf_[a-z0-9_]+)\(([^;]*)\);", hdr[hdr.index("#ifndef KTF_DENSE_H_"):], flags=re.M)
    assert {n for n, _ in protos} == set(L.DENSE_PROTOTYPES) and all(n.startswith("ktf_dense_") for n in L.DENSE_PROTOTYPES)
    ctype = {"const float*": L._P, "float*": L._P, "void*": L._P, "int64_t": L._i64, "int32_t": L._i32, "size_t": C.c_size_t}
    for name, args in protos:
        args = [a.strip() for a in args.replace("\n", " ").split(",")]
        assert L.DENSE_PROTOTYPES[name][1] == ([] if args == ["void"] else [ctype[a.rsplit(" ", 1)[0]] for a in args]), name
    assert L.load().ktf_dense_slot_cols() == int(re.search(r"#define KTF_DENSE_SLOT_COLS (\d+)", hdr).group(1))


@pytest.mark.parametrize("name,kw,text", REFUSALS)
def test_refused_before_any_launch(name, kw, text):
    _refused(call(name, **kw), text)


def test_workspace_size_is_its_formula():
    lib = L.load()
    slot = lib.ktf_dense_slot_cols()
    for m, n, d in [(0, 1, 1), (64, 7323, 512), (19, slot, 64), (19, slot + 1, 64), (33, 2 * slot + 3, 31), (1000, 60000 * 8, 512)]:
        want = (-(-n // slot) * max(m, 1) * d * 4 + 255) & ~255
        assert lib.ktf_dense_workspace_bytes(m, n, d) == want > 0, (m, n, d)
    for bad in ((-1, 4, 4), (4, 0, 4), (4, 4, 0), (BIG, 4, 4), (4, BIG, 4), (4, 4, BIG), (BIG - 1, BIG - 1, BIG - 1)):
        assert lib.ktf_dense_workspace_bytes(*bad) == -1, bad


def test_host_side_of_the_autograd_functions():
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="affine"):
        A.ClassifierHead(6, 9, affine="nope", device=cpu)
    head = A.ClassifierHead(6, 9, sub_centers=2, affine="dense", device=cpu)
    assert head.affine == head.dominant().affine == "dense"
    with pytest.raises(ktf.KtfBackendError):
        A.dense_affine(torch.zeros((3, 6)), torch.zeros((9, 6)))
    with pytest.raises(ktf.KtfBackendError):
        head(torch.zeros((3, 6)), torch.tensor([0, 1, 2]))
