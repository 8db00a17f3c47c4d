"""Every kernel instance the front-end launchers can start -- fifteen of frontend512_kernel, six of frontend_kernel -- against the fp64
oracle, on the smallest shapes that still reach every path, called the way XvectorExtractor._features calls ops.frontend. Before each
launch the plan query must name the instance the case is there for; the bound is _frontend_ref.py's (4 x the rms, 8 x the maximum of
what an fp32 restatement of the same chain loses against the oracle, per case and per output). Outputs are filled with NaN before the
call and followed by a guard band: every element of (B, T, last) is written, nothing behind it is.

Run with -s to see the ratios per case and, from the last test, the worst per instance (the table in DESIGN.md)."""

import types

import numpy as np
import pytest
import torch

import _frontend_ref as R
from kaldi_tflite_amd import _lib as L, ops

pytestmark = pytest.mark.gpu

GUARD = 1024                    # elements of guard band behind the output
CASES = R.fast_cases() + R.generic_cases()
_ran = {}                       # case name -> (instance, {output: (rms ratio, max ratio, rms error, max error)}, speech)


def _tables(c, mf, dev):
    tables = mf.tables(dev)
    if c.fast or tables.fast_tw is None:
        return tables
    s = L.FrontendTables.from_buffer_copy(tables.struct)        # the same device tables without the fast ones: the generic kernel at nfft 512
    s.fast_tw = s.fast_mel_meta = s.fast_mel_w = None
    s.reserved = 0
    return types.SimpleNamespace(struct=s, keep=tables)


def _device_input(c, buf, dev):
    dt = torch.int16 if c.kind == "i16" else torch.float32
    x = torch.as_tensor(buf.astype(np.int16 if c.kind == "i16" else np.float32), dtype=dt).to(dev)
    if c.row_stride:
        x = x.unfold(0, c.n, c.row_stride)                      # (B, n) overlapping windows of one recording, read in place
        assert x.shape == (c.B, c.n) and x.stride() == (c.row_stride, 1)
    return x


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_instance_against_the_oracle(c):
    dev = torch.device("cuda", 0)
    mf, cfg = R.frontend_cfg(c)
    tables = _tables(c, mf, dev)
    buf, rows = R.samples(c)
    if c.dither:
        assert 6 * c.dither < 2.0 ** -25 * np.abs(buf).min()     # x + g * dither rounds back to x (|g| < 5.9): the dither-free oracle holds
    x = _device_input(c, buf, dev)
    kind, stage, T = R.KINDS[c.kind], R.STAGES[c.out], c.frames_per_row()

    plan = ops.frontend_plan(c.B, c.n, kind, cfg, tables, stage)
    assert R.plan_key(plan) == c.want and plan.T == T, (R.plan_key(plan), c.want, plan.T, T)
    if c.want[0] == "fast512" and c.fast:
        items = R.mel_items(c)
        assert tables.struct.reserved == items[1] and np.array_equal(tables.fast_mel_meta.cpu().numpy(), items[0])

    last = {L.OUT_WINDOWED: c.M, L.OUT_FBANK: c.num_mels, L.OUT_MFCC: c.num_ceps}[stage]
    numel = c.B * T * last
    flat = torch.full((numel + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    out = flat[:numel].view(c.B, T, last)
    want_energy = c.out == "windowed" and c.use_energy
    r = ops.frontend(x, kind, cfg, tables, stage, c.n, c.B, T, seed=0xD17E, want_energy=want_energy, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(flat[numel:]).all()), "the guard band behind the output was written"
    feats = flat[:numel].view(c.B, T, last).cpu().numpy()
    assert np.isfinite(feats).all(), "an element of the output was not written"
    got = R._split(c, feats, r[1].cpu().numpy()[..., None] if want_energy else None)

    r64, r32 = R.ref64(c, rows), R.ref32(c, rows)
    ratios = R.ratios(got, r64, r32)
    for k, (rr, mr, gr, gm) in ratios.items():
        print(f"\n  {c.name} {c.want} {k}: rms {gr:.3e} = {rr:.2f} x yardstick, max {gm:.3e} = {mr:.2f} x yardstick", end="")
    _ran[c.name] = (c.want, ratios, c.speech)
    # the recording has near-silent frames, where the maximum is a statement about 1 / energy: rms, plus the suite's 1e-3 maximum
    bad = R.violations(got, r64, r32, rms_only=c.speech, max_abs=1e-3 if c.speech else None)
    assert not bad, (c.name, c.want, bad)


def test_the_cases_cover_every_instance():
    assert {c.want for c in CASES} == R.INSTANCES
    if len(_ran) < len(CASES):
        return                                                   # a selection of the cases ran: the table above is the whole claim
    assert {v[0] for v in _ran.values()} == R.INSTANCES
    worst = {}
    for name, (inst, ratios, speech) in _ran.items():
        for k, (rr, mr, _, _) in ratios.items():
            w = worst.setdefault(inst, [0.0, "", 0.0, ""])
            if rr > w[0]:
                w[0], w[1] = rr, f"{name}:{k}"
            if not speech and mr > w[2]:                         # (the recording is held to the rms bound and 1e-3)
                w[2], w[3] = mr, f"{name}:{k}"
    print("\nworst ratio to the fp32 yardstick per instance (rms, bound 4 | max, bound 8):")
    for inst in sorted(worst, key=str):
        w = worst[inst]
        print(f"  {inst}: rms {w[0]:.2f} ({w[1]}) | max {w[2]:.2f} ({w[3]})")
