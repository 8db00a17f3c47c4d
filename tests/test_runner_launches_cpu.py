"""Sequential.run_ragged's launch sequence, pinned on the CPU: the native library is replaced by a recorder (the pure host size helpers
still answer from the real libktf_hip.so), the runner runs on CPU tensors, and every library call (name, integer / float arguments,
every KtfTdnnDesc field), every workspace request (role, shape, dtype, `padded`) and what run_ragged returns is written out. The grid
of cases reaches every branch of the runner; tests/golden/runner_launches.txt is the expected record.

    python tests/test_runner_launches_cpu.py --write      # regenerate the golden file (only for a deliberate change of behaviour)
"""

import contextlib
import difflib
import os
import re
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "kaldi-tflite_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import synth  # noqa: E402
import kaldi_tflite_amd as ktf  # noqa: E402
from kaldi_tflite_amd import _lib as L, models  # noqa: E402
from _recorder import STREAM, Recorder  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "runner_launches.txt")
HOST_HELPERS = re.compile(r"ktf_(\w+_)?(stats_slots|slot_rows)|ktf_flat_row_map_rows|ktf_tdnn_out_len")
EVERY_LAUNCH = {
    "ktf_tdnn", "ktf_tdnn_stats",
    "ktf_tdnn_split", "ktf_tdnn_split_flat", "ktf_tdnn_split_stats", "ktf_tdnn_split_flat_stats",
    "ktf_tdnn_mx", "ktf_tdnn_mx_flat", "ktf_tdnn_mx_stats", "ktf_tdnn_mx_flat_stats",
    "ktf_mx_planes", "ktf_split_bf16_rows", "ktf_flat_row_map", "ktf_tdnn_out_lens",
    "ktf_stats_finalize", "ktf_stats_finalize_slots", "ktf_stats_finalize_flat", "ktf_stats_pool",
}


# ----------------------------------------------------------------------------- topologies
def _odd_config():
    """VALID padding, subsampling, a narrow and a tanh layer between wide ones (both leave the reduced-precision kernels), pooling, a tail."""
    rows = [(256, [-2, 0, 2], "SAME", 1, "bn"), (256, [-1, 0, 1], "VALID", 1, "bn"), (300, [-3, 0, 3], "SAME", 2, "relu"),
            (96, [0], "SAME", 1, "bn"), (256, [-1, 0, 1], "SAME", 1, "tanh"), (512, [0], "SAME", 1, "bn")]
    layers = [{"name": "input", "type": "input", "shape": [None, None, 40]}]
    for i, (u, ctx, pad, sub, form) in enumerate(rows):
        cfg = {"units": u, "context": ctx, "padding": pad, "subsampling_factor": sub}
        kinds = {"bn": ["affine", "relu", "batchnorm"], "relu": ["affine", "relu"]}.get(form, "affine")
        if form == "tanh":
            cfg["activation"] = "tanh"
        layers.append({"name": f"t{i}", "type": kinds, "cfg": cfg})
    layers.append({"name": "stats", "type": "stats",
                   "cfg": {"left_context": 0, "right_context": 10000, "include_std": True, "reduce_time_axis": True}})
    layers.append({"name": "t6", "type": "affine", "cfg": {"units": 64, "context": [0]}})
    return {"type": "sequential", "layers": layers}


TOPOLOGIES = {"xvec": (synth.model_config(), 30), "odd": (_odd_config(), 40)}
FREE = {"min_tiles": {}, "min_frames": {}}          # routing floors off: the batch runs the model's own mode and kernels

# (name, topology, gemm, knobs, B, T, ragged (False: lens None), defer_tail, run mode)
CASES = [
    ("mx_tiles", "xvec", "f16mx", dict(FREE, mx_loader=False), 4, 256, True, False, None),
    ("mx_tiles_defer", "xvec", "f16mx", dict(FREE, mx_loader=False), 4, 256, True, True, None),
    ("mx_tiles_nondet", "xvec", "f16mx", dict(FREE, mx_loader=False, deterministic=False), 4, 256, True, False, None),
    ("mx_tiles_nondet_defer", "xvec", "f16mx", dict(FREE, mx_loader=False, deterministic=False), 4, 256, True, True, None),
    ("mx_flat", "xvec", "f16mx", dict(FREE, mx_loader=False), 4, 300, True, False, None),
    ("mx_flat_defer", "xvec", "f16mx", dict(FREE, mx_loader=False), 4, 300, True, True, None),
    ("mx_flat_nondet", "xvec", "f16mx", dict(FREE, mx_loader=False, deterministic=False), 4, 300, True, False, None),
    ("mx_flat_nondet_defer", "xvec", "f16mx", dict(FREE, mx_loader=False, deterministic=False), 4, 300, True, True, None),
    ("mx_flat_no_flat_pooling", "xvec", "f16mx", dict(FREE, mx_loader=False, flat_pooling=False), 4, 300, True, True, None),
    ("mx_no_flat_rows", "xvec", "f16mx", dict(FREE, mx_loader=False, mx_flat_rows=False), 4, 300, True, False, None),
    ("mx_loader", "xvec", "f16mx", dict(FREE, mx_loader=True), 4, 300, True, False, None),
    ("mx_loader_defer", "xvec", "f16mx", dict(FREE, mx_loader=True), 4, 300, True, True, None),
    ("mx_loader_auto", "xvec", "f16mx", dict(FREE), 8, 998, True, True, None),
    ("mx_dense", "xvec", "f16mx", dict(FREE), 2, 300, False, False, None),
    ("mx_no_fuse_stats", "xvec", "f16mx", dict(FREE, mx_loader=False, fuse_stats=False), 4, 256, True, True, None),
    ("mx_odd", "odd", "f16mx", dict(FREE), 3, 300, True, False, None),
    ("mx_odd_defer", "odd", "f16mx", dict(FREE), 3, 300, True, True, None),
    ("mx_odd_dense", "odd", "f16mx", dict(FREE), 3, 300, False, False, None),
    ("mx_short_pass", "xvec", "f16mx", dict(FREE), 4, 300, True, True, "bf16x3"),
    ("mx_short_mode", "xvec", "f16mx", dict(min_tiles={}), 4, 300, True, True, None),
    ("x3_tiles", "xvec", "bf16x3", dict(FREE), 4, 256, True, False, None),
    ("x3_tiles_defer", "xvec", "bf16x3", dict(FREE), 4, 256, True, True, None),
    ("x3_tiles_nondet", "xvec", "bf16x3", dict(FREE, deterministic=False), 4, 256, True, False, None),
    ("x3_flat", "xvec", "bf16x3", dict(FREE), 4, 148, True, False, None),
    ("x3_flat_defer", "xvec", "bf16x3", dict(FREE), 4, 148, True, True, None),
    ("x3_flat_nondet", "xvec", "bf16x3", dict(FREE, deterministic=False), 4, 148, True, True, None),
    ("x3_flat_long", "xvec", "bf16x3", dict(FREE), 4, 300, True, False, None),
    ("x3_no_flat_rows_long", "xvec", "bf16x3", dict(FREE, flat_rows_long=False), 4, 300, True, False, None),
    ("x3_no_flat_pooling", "xvec", "bf16x3", dict(FREE, flat_pooling=False), 4, 148, True, False, None),
    ("x3_no_flat_rows", "xvec", "bf16x3", dict(FREE, flat_rows=False), 4, 148, True, False, None),
    ("x3_no_planes", "xvec", "bf16x3", dict(FREE, split_planes=False), 4, 300, True, False, None),
    ("x3_no_planes_defer", "xvec", "bf16x3", dict(FREE, split_planes=False), 4, 300, True, True, None),
    ("x3_no_fuse_stats", "xvec", "bf16x3", dict(FREE, fuse_stats=False), 4, 148, True, False, None),
    ("x3_odd", "odd", "bf16x3", dict(FREE), 3, 300, True, True, None),
    ("x3_odd_dense", "odd", "bf16x3", dict(FREE), 3, 300, False, False, None),
    ("x3_dense", "xvec", "bf16x3", dict(FREE), 2, 148, False, True, None),
    ("bf16_pooled", "xvec", "bf16", dict(FREE), 4, 300, True, False, None),
    ("bf16_pooled_defer", "xvec", "bf16", dict(FREE, deterministic=False), 4, 300, True, True, None),
    ("bf16_odd", "odd", "bf16", dict(FREE), 3, 300, True, False, None),
    ("pair", "xvec", "f16mx", {}, 1, 998, True, False, None),
    ("pair_defer", "xvec", "f16mx", {}, 2, 300, True, True, None),
    ("pair_nondet", "xvec", "bf16x3", dict(deterministic=False), 2, 300, True, False, None),
    ("pair_no_fuse_stats", "xvec", "f16mx", dict(fuse_stats=False), 2, 300, True, True, None),
    ("pair_odd", "odd", "bf16x3", {}, 2, 300, True, True, None),
    ("no_pairs", "xvec", "f16mx", dict(small_tile_pairs=False), 2, 300, True, True, None),
    ("f32", "xvec", "f32", {}, 2, 300, True, False, None),
    ("f32_defer", "xvec", "f32", {}, 2, 300, True, True, None),
    ("f32_odd_dense", "odd", "f32", {}, 2, 200, False, True, None),
]


# ----------------------------------------------------------------------------- what the recorder's lines name
def _pointer_names(mdl, x_buf, lens):
    """address -> what it points into: a workspace role + offset, a layer's weight set, the caller's input; "tmp" for a fresh tensor."""
    def spans():
        for (role, *_), slot in mdl._ws_own._arenas.items():
            yield f"ws:{role}", slot[0]
        for l in mdl.layers:
            if isinstance(l, ktf.layers.BatchNorm) and l._dev is not None:
                yield from ((f"{l.name}.{part}", t) for part, t in zip(("scale", "shift"), l._dev))
            if isinstance(l, ktf.layers.TDNN):
                for key, ts in l._dev.items():
                    if key[0] == "mx":
                        fold = next((f.name for f in mdl.layers if key[2] is not None and id(f) == key[2][0]), None)
                        tag, parts = f"mx[{key[3]},fold={fold}]", ("wh", "wq", "bias")
                    else:
                        tag, parts = f"w[gemm={key[1]},kint={int(key[2])},tiled={int(key[3])}]", ("w", "w_lo", "bias")
                    yield from ((f"{l.name}.{tag}.{part}", t) for part, t in zip(parts, ts) if t is not None)
        yield "x", x_buf
        if lens is not None:
            yield "lens", lens

    def name(addr):
        if addr is None:
            return "null"
        for tag, t in spans():
            base = t.data_ptr()
            if base <= addr < base + t.numel() * t.element_size():
                return f"{tag}+{addr - base}"
        return "tmp"
    return name


def _tensor(names, t):
    return "null" if t is None else f"{names(t.data_ptr())}{list(t.shape)}{list(t.stride())}{str(t.dtype)[6:]}"


def run_case(monkeypatch, case):
    name, topo, gemm, knobs, B, T, ragged, defer, mode = case
    cfg, D = TOPOLOGIES[topo]
    mdl = ktf.models.SequentialFromConfig(cfg, None, name, gemm=gemm)
    for k, v in knobs.items():
        setattr(mdl, k, v)
    x_buf = torch.zeros((B, T, 32 * -(-D // 32)), dtype=torch.float32)
    lens = torch.tensor([max(1, T - 37 * i) for i in range(B)], dtype=torch.int32) if ragged else None
    rec = Recorder(L.load(), HOST_HELPERS, _pointer_names(mdl, x_buf, lens))
    get = models._Workspace.get

    def recorded_get(ws, role, shape, dtype, device, padded=True):
        rec.lines.append(f"get({role}, {list(shape)}, {str(dtype)[6:]}, padded={padded})")
        return get(ws, role, shape, dtype, device, padded)
    with monkeypatch.context() as m:
        m.setattr(L, "_lib", rec)
        m.setattr(L, "load", lambda: rec)
        m.setattr(L, "require_gpu", lambda: None)
        m.setattr(L, "stream_ptr", lambda: STREAM)
        m.setattr(L, "on_device", lambda device: contextlib.nullcontext())
        m.setattr(models._Workspace, "enter", lambda ws, device: setattr(ws._tl, "where", (str(device), 0, 0)))
        m.setattr(models._Workspace, "get", recorded_get)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out = mdl.run_ragged(x_buf[:, :, :D], lens, defer_tail=defer, mode=mode)
        if isinstance(out, models.DeferredTail):
            rec.lines.append(f"-> DeferredTail(layer={out.layer.name}, B={out.B}, D={out.D}, include_std={out.include_std}, eps={out.eps!r}, "
                             f"pooled={_tensor(rec.names, out.pooled)}, sums={_tensor(rec.names, out.sums)}, slots={out.slots}, "
                             f"lens={_tensor(rec.names, out.lens)}, T={out.T}, slot_rows={out.slot_rows})")
        else:
            rec.lines.append(f"-> {_tensor(rec.names, out)}")
    return [f"== {name}: {topo} {gemm} {knobs} B={B} T={T} ragged={ragged} defer_tail={defer} mode={mode}"] + rec.lines, rec.called


def record(monkeypatch):
    lines, called = [], set()
    for case in CASES:
        ls, c = run_case(monkeypatch, case)
        lines += ls
        called |= c
    return lines, called


def test_runner_launches_match_golden(monkeypatch):
    lines, called = record(monkeypatch)
    assert not EVERY_LAUNCH - called, f"the grid no longer reaches {sorted(EVERY_LAUNCH - called)}"
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    if lines != want:
        diff = list(difflib.unified_diff(want, lines, "golden", "run_ragged", lineterm="", n=2))
        raise AssertionError("run_ragged's launches changed:\n" + "\n".join(diff[:80]))


if __name__ == "__main__":
    if "--write" not in sys.argv:
        sys.exit(__doc__)
    mp = __import__("pytest").MonkeyPatch()
    try:
        lines, called = record(mp)
    finally:
        mp.undo()
    missing = EVERY_LAUNCH - called
    if missing:
        sys.exit(f"the grid does not reach {sorted(missing)}")
    with open(GOLDEN, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{GOLDEN}: {len(lines)} lines, {len(CASES)} cases")
