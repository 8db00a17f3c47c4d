"""What test_gpu_frontend_instances.py rests on, checked without a GPU: the fp32 yardstick of _frontend_ref.py is itself pinned (Kaldi
goldens; a second fp32 restatement and reversed sums sit inside the bound), the bound rejects eleven ways a kernel can be subtly wrong,
the launcher's plan query reaches exactly the instances the GPU cases cover, and the plan refuses what the launch refuses."""

import ctypes as C
import dataclasses
import itertools

import numpy as np
import pytest

import _frontend_ref as R
import _golden as G
from kaldi_tflite_amd import _lib as L, ops


def _golden_case(cfg, mf=None, fb=None, wd=None):
    f = cfg["framing"]
    M, shift = int(f["frame_length_ms"] / 1000.0 * f["sample_frequency"]), int(f["frame_shift_ms"] / 1000.0 * f["sample_frequency"])
    kw = dict(sf=f["sample_frequency"], M=M, shift=shift, pad=not cfg["snip_edges"], B=1)
    if mf is not None:
        kw.update(out="mfcc", num_mels=mf["num_mels"], num_ceps=mf["num_mfccs"], lifter=mf["cepstral_lifter"], use_energy=mf["use_energy"],
                  low=mf["low_freq_cutoff"], high=mf["high_freq_cutoff"], use_log=mf["use_log_fbank"], use_power=mf["use_power"])
        wd = mf
    else:
        kw.update(out="fbank", num_mels=fb["num_bins"], low=fb["low_freq_cutoff"], high=fb["high_freq_cutoff"], use_log=fb["use_log_fbank"],
                  use_power=fb["use_power"], use_energy=False)
    assert wd["dither"] == 0.0
    kw.update(window=wd["window_type"], raw_energy=wd["raw_energy"], remove_dc=wd["remove_dc_offset"], preemph=wd["preemphasis_coefficient"],
              energy_floor=wd["energy_floor"], eps=wd["epsilon"])
    return kw


# ----------------------------------------------------------------------------- the yardstick is itself pinned
def test_yardstick_meets_the_kaldi_mfcc_goldens():
    # layers/dsp/mfcc_test.py:32  RMSE < 2.25e-4 on 54 Kaldi cases
    for name in G.mfcc_case_names():
        cfg, wav, want = G.mfcc_case(name)
        c = R.Case(name=name, n=wav.shape[-1], **_golden_case(cfg, mf=cfg["mfcc"]))
        r = R.ref32(c, wav)
        got = np.concatenate([r["c0"][..., None], r["ceps"]], -1) if c.use_energy else r["ceps"]
        assert got.shape == want.shape and got.dtype == np.float32, name
        assert G.rmse(want, got) < 2.25e-4, (name, G.rmse(want, got))


def test_yardstick_meets_the_kaldi_fbank_goldens():
    # layers/dsp/filterbank_test.py:32  RMSE < 2.25e-5
    for name in G.fbank_case_names():
        cfg, wav, want = G.fbank_case(name)
        c = R.Case(name=name, n=wav.shape[-1], **_golden_case(cfg, fb=cfg["fbank"], wd=cfg["windowing"]))
        got = R.ref32(c, wav)["fbank"]
        assert got.shape == want.shape and got.dtype == np.float32, name
        assert G.rmse(want, got) < 2.25e-5, (name, G.rmse(want, got))


# cases the CPU checks of the bound run on: every nfft, frames of 34 .. 2048 samples, 64 frames of sigma = 1000 integer noise
def _bound_cases():
    mels = {64: 5, 128: 8, 256: 23, 512: 30, 1024: 40, 2048: 40}
    out = []
    for lg in range(6, 12):
        nf = 1 << lg
        for M in (nf, nf // 2 + 2):
            for stage in ("mfcc", "fbank"):
                out.append(R.Case(name=f"bound_{nf}_{M}_{stage}", M=M, kind="frames", out=stage, num_mels=mels[nf], num_ceps=min(13, mels[nf]),
                                  high=0.0, use_log=(stage == "mfcc" or lg % 2 == 0), B=1, n=64))
    return out


@pytest.fixture(scope="module")
def bound_refs():
    refs = {}
    for c in _bound_cases():
        _, rows = R.samples(c)
        refs[c.name] = (c, rows, R.ref64(c, rows), R.ref32(c, rows))
    return refs


def test_other_fp32_restatements_sit_inside_the_bound(bound_refs):
    worst = {}
    for c, rows, r64, r32 in bound_refs.values():
        for label, kw in (("numpy_fft", dict(fft="numpy")), ("reversed_sums", dict(reverse=True)),
                          ("numpy_fft_reversed", dict(fft="numpy", reverse=True))):
            got = R.ref32(c, rows, **kw)
            assert not R.violations(got, r64, r32), (c.name, label, R.violations(got, r64, r32))
            for rr, mr, _, _ in R.ratios(got, r64, r32).values():
                w = worst.setdefault(label, [0.0, 0.0])
                w[0], w[1] = max(w[0], rr), max(w[1], mr)
    print("worst (rms, max) ratio of other fp32 restatements:", {k: (round(a, 2), round(b, 2)) for k, (a, b) in worst.items()})


# ----------------------------------------------------------------------------- the bound has teeth
_DEFAULT = dict(B=2, n=400 + 20 * 160)
_TEETH = {
    "mel_tail": R.Case(name="teeth_mel_tail", **_DEFAULT),                      # 10-bin items: the last 4 weights of one of them
    "twiddle": R.Case(name="teeth_twiddle", **_DEFAULT),
    "window_shift": R.Case(name="teeth_window_shift", **_DEFAULT),
    "preemph_first": R.Case(name="teeth_preemph_first", window="hamming", **_DEFAULT),   # (the povey window is zero at sample 0)
    "pad_left": R.Case(name="teeth_pad_left", pad=True, B=2, n=1000),
    "dc_nfft": R.Case(name="teeth_dc_nfft", **_DEFAULT),
    "bf16_spectrum": R.Case(name="teeth_bf16_spectrum", **_DEFAULT),
    "post_energy": R.Case(name="teeth_post_energy", **_DEFAULT),
    "no_lifter": R.Case(name="teeth_no_lifter", **_DEFAULT),
    "magnitude": R.Case(name="teeth_magnitude", **_DEFAULT),
    "frame_start": R.Case(name="teeth_frame_start", **_DEFAULT),
}


@pytest.mark.parametrize("corruption", R.CORRUPTIONS)
def test_the_bound_rejects(corruption):
    c = _TEETH[corruption]
    _, rows = R.samples(c)
    r64, r32 = R.ref64(c, rows), R.ref32(c, rows)
    assert not R.violations(R.ref32(c, rows, fft="numpy"), r64, r32)            # the same case passes when nothing is wrong
    bad = R.violations(R.ref32(c, rows, corrupt=corruption), r64, r32)
    print(corruption, bad)
    assert bad, f"{corruption} went unnoticed"
    # ... by both halves of the bound (the rms alone would do: no corruption hides in the average)
    assert any("rms" in b for b in bad) and any("max" in b for b in bad), bad


def test_the_bound_rejects_a_dropped_tail_in_every_nq_bank():
    """The mel-tail corruption on the banks of the NQ = 4 (13-bin) and NQ = 5 instances too (6-bin items fit two pieces: nothing to drop)."""
    for bank in (R.BANK_NQ4_SPLIT, R.BANK_NQ5):
        c = R.Case(name=f"teeth_tail_{bank['num_mels']}", num_ceps=bank["num_mels"], **bank, **_DEFAULT)
        _, rows = R.samples(c)
        assert R.violations(R.ref32(c, rows, corrupt="mel_tail"), R.ref64(c, rows), R.ref32(c, rows))


def test_tiny_dither_cannot_change_a_sample():
    """x + g * dither rounds back to x: |g| < 5.9 for the generic kernel's Box-Muller (sqrt(-2 ln 2^-25)), < 4.85 for the fast kernel's."""
    assert np.sqrt(-2.0 * np.log(2.0 ** -25)) < 5.9
    for c in R.fast_cases() + R.generic_cases():
        if c.dither:
            buf, _ = R.samples(c)
            assert c.dither == R.TINY_DITHER and 6 * c.dither < 2.0 ** -25 * np.abs(buf).min()
            x = buf.astype(np.float32)
            assert np.array_equal(x + np.float32(6 * c.dither), x) and np.array_equal(x - np.float32(6 * c.dither), x)


# ----------------------------------------------------------------------------- instance coverage
def test_mel_banks_give_the_pieces_the_nq_instances_read():
    for bank, items, nq in R.BANK_ITEMS:
        c = R.Case(name="bank", num_ceps=bank["num_mels"], **bank)
        meta, longest = R.mel_items(c)
        assert longest == items == meta[:, 1].max() and (longest + 6) // 4 == nq, (bank, longest)
    assert int((R.mel_items(R.Case(name="b", num_ceps=23, **R.BANK_NQ4_SPLIT))[0][:, 2] >= 0).sum()) == 46


def test_plan_scan_reaches_exactly_the_instance_table():
    """Every call the launcher can tell apart -> the set of instances it starts. The GPU test must cover this set, no more, no less."""
    seen = set()
    for M in (34, 100, 200, 258, 320, 400, 512, 600, 1102):
        base = R.Case(name="scan", M=M, shift=M // 2 - 1, num_mels=5 if M < 100 else 30, num_ceps=5, high=0.0)
        _, base_cfg = R.frontend_cfg(base)
        tables = {fast: R.host_tables(dataclasses.replace(base, fast=fast)) for fast in ((True, False) if base.nfft == 512 else (False,))}
        for kind, pad, dither, std, reserved, fast in itertools.product(R.KINDS, (False, True), (0.0, 1.0), (True, False), range(1, 17), tables):
            if not fast and reserved > 1:
                continue                              # no fast tables: nothing to vary
            is_wav = kind in ("wav", "i16")
            c = dataclasses.replace(base, kind=kind, pad=pad and is_wav, dither=dither, raw_energy=std, fast=fast, B=2,
                                    out="fbank" if kind == "windowed" else "mfcc", n=5 * M if is_wav else 5)
            cfg = L.FrontendCfg.from_buffer_copy(base_cfg)
            cfg.frame_shift, cfg.pad_mode, cfg.dither, cfg.raw_energy = (c.shift if is_wav else M), int(c.pad), dither, int(std)
            tab = tables[fast]
            if fast:
                assert tab.fast_tw and tab.fast_mel_meta and tab.fast_mel_w
                tab.reserved = reserved
            p = R.plan(c, tab, cfg)
            key = R.plan_key(p)
            seen.add(key)
            assert p.T == c.frames_per_row() and p.lds_bytes > 0 and p.grid_x >= 1
            dith = dither != 0 and kind != "windowed"
            if fast:
                want_std = M == 400 and is_wav and not c.pad and not dith and std
                assert key == ("fast512", dith, 0 if c.pad else 2 if kind == "i16" else 1, 400 if (M == 400 and not dith) else 0, want_std,
                               (3 if reserved <= 9 else 4 if reserved <= 13 else 5) if want_std else 5), (c, reserved, key)
                assert (p.grid_x, p.grid_y, p.log2_nfft) == (min(2048 // c.B, -(-p.T // 8)), c.B, 9)
            else:
                assert key == ("generic", c.nfft.bit_length() - 1) and (p.grid_x, p.grid_y) == (min(2048, -(-c.B * p.T // R.FE_WAVES)), 1)
    # every switch of the shipped configuration, on its own, leaves the STD instances
    c = R.Case(name="scan", B=2, n=2000)
    _, cfg0 = R.frontend_cfg(c)
    tab = R.host_tables(c)
    assert R.plan_key(R.plan(c, tab, cfg0)) == ("fast512", False, 1, 400, True, 4)
    for field, off in (("remove_dc", 0), ("use_energy", 0), ("raw_energy", 0), ("preemph", 0.0), ("use_power", 0), ("use_log", 0)):
        cfg = L.FrontendCfg.from_buffer_copy(cfg0)
        setattr(cfg, field, off)
        assert R.plan_key(R.plan(c, tab, cfg)) == ("fast512", False, 1, 400, False, 5), field
    assert R.plan_key(ops.frontend_plan(2, 2000, L.IN_WAV, cfg0, tab, L.OUT_FBANK)) == ("fast512", False, 1, 400, False, 5)
    # more mel bins or cepstra than a lane each, or sizes past the kernel's 32-bit offsets: the generic kernel at nfft 512
    c33 = dataclasses.replace(c, num_mels=33, num_ceps=33, high=0.0)
    t33 = R.host_tables(c33)
    t33.fast_tw = t33.fast_mel_meta = t33.fast_mel_w = 1
    t33.reserved = 10
    assert R.plan_key(R.plan(c33, t33)) == ("generic", 9)
    assert R.plan_key(ops.frontend_plan(65536, 2000, L.IN_WAV, cfg0, tab, L.OUT_MFCC)) == ("generic", 9)
    assert R.plan_key(ops.frontend_plan(1, 1 << 22, L.IN_FRAMES, cfg0, tab, L.OUT_MFCC)) == ("generic", 9)
    assert seen == R.INSTANCES, (sorted(seen - R.INSTANCES), sorted(R.INSTANCES - seen))
    assert len([k for k in seen if k[0] == "fast512"]) == 15 and len([k for k in seen if k[0] == "generic"]) == 6


def test_gpu_cases_cover_the_instance_table():
    cases = R.fast_cases() + R.generic_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        p = R.plan(c, R.host_tables(c))
        assert R.plan_key(p) == c.want and p.T == c.frames_per_row(), (c.name, R.plan_key(p), c.want)
    assert {c.want for c in cases} == R.INSTANCES
    # and the shapes are the ones that reach the paths they are there for
    by = {c.name: (c, R.plan(c, R.host_tables(c))) for c in cases}
    c, p = by["std_f32_nq4_two_passes"]
    assert (p.grid_x, p.grid_y, p.T) == (2, 1024, 17)             # three groups of 8 frames on two workgroups: a second pass, one live wave
    c, p = by["nfft64_grid_stride"]
    assert c.B * p.T == 2048 * R.FE_WAVES + 5 and p.grid_x == 2048
    lib = L.load()
    c, _ = by["f400_pad_f32_smallest_n"]
    assert lib.ktf_num_frames_padded(c.n, c.M, c.shift, 1) >= 1 and all(lib.ktf_num_frames_padded(n, c.M, c.shift, 1) < 1 for n in range(c.n))
    c, _ = by["f400_pad_f32_both_edges_mirror"]
    assert c.frames_per_row() == 1 and (c.M - c.shift) // 2 > 0 and c.M - c.n - (c.M - c.shift) // 2 > 0
    assert all(c.n % 2 == 1 and c.B == 3 for c in cases if c.kind == "i16")
    c, _ = by["std_f32_nq5_overlapping_rows"]
    assert 0 < c.row_stride < c.n


# ----------------------------------------------------------------------------- refusals
def test_reserved_outside_1_to_16_is_refused():
    lib = L.load()
    c = R.Case(name="refuse", B=1, n=16000)
    _, cfg = R.frontend_cfg(c)
    buf = (C.c_float * 4)()
    plan = L.FrontendPlan()
    for reserved in (0, -1, 17, 1 << 20):
        tab = R.host_tables(c, reserved=reserved)
        for rc in (lib.ktf_frontend_plan(1, 16000, L.IN_WAV, C.byref(cfg), C.byref(tab), L.OUT_MFCC, C.byref(plan)),
                   lib.ktf_frontend_f32(buf, 1, 16000, L.IN_WAV, C.byref(cfg), C.byref(tab), L.OUT_MFCC, buf, None, 0, None)):
            assert rc == -1 and "reserved" in L.last_error(), (reserved, rc, L.last_error())
        with pytest.raises(ValueError):
            ops.frontend_plan(1, 16000, L.IN_WAV, cfg, tab, L.OUT_MFCC)
    for reserved in (1, 16):
        assert lib.ktf_frontend_plan(1, 16000, L.IN_WAV, C.byref(cfg), C.byref(R.host_tables(c, reserved=reserved)), L.OUT_MFCC,
                                     C.byref(plan)) == 0 and plan.kernel == L.FE_FAST512
    # without the fast tables the field means nothing and is not looked at
    tab = R.host_tables(dataclasses.replace(c, fast=False))
    tab.reserved = 99
    assert lib.ktf_frontend_plan(1, 16000, L.IN_WAV, C.byref(cfg), C.byref(tab), L.OUT_MFCC, C.byref(plan)) == 0 and plan.kernel == L.FE_GENERIC


def test_plan_and_launch_refuse_alike():
    """Invalid calls: the same return code and the same message from the query and from the launch (given buffers it never touches)."""
    lib = L.load()
    c = R.Case(name="refuse", B=1, n=16000)
    _, good = R.frontend_cfg(c)
    tab = R.host_tables(c)
    buf = (C.c_float * 4)()
    plan = L.FrontendPlan()

    def cfg(**kw):
        v = L.FrontendCfg.from_buffer_copy(good)
        for k, x in kw.items():
            setattr(v, k, x)
        return v

    def tabs(**kw):
        t = R.host_tables(c)
        for k, x in kw.items():
            setattr(t, k, x)
        return t

    bad = [
        (dict(B=-1), "negative size"), (dict(n=-1), "negative size"), (dict(in_kind=4), "bad in_kind"), (dict(out_stage=4), "bad out_stage"),
        (dict(cfg=cfg(pad_mode=2)), "bad pad_mode"), (dict(cfg=cfg(row_stride=-1)), "negative row_stride"),
        (dict(cfg=cfg(nfft=500)), "power of two"), (dict(cfg=cfg(nfft=4096, frame_size=4000)), "power of two"),
        (dict(cfg=cfg(nfft=32, frame_size=30)), "power of two"), (dict(cfg=cfg(frame_size=600)), "> nfft"),
        (dict(cfg=cfg(frame_shift=0)), "must be > 0"), (dict(cfg=cfg(num_mels=129)), "num_mels"), (dict(cfg=cfg(num_ceps=31)), "num_ceps"),
        (dict(cfg=cfg(num_ceps=0)), "num_ceps"), (dict(n=399), "shorter than a frame"), (dict(cfg=cfg(pad_mode=1), n=100), "mirror padding"),
        (dict(in_kind=L.IN_WINDOWED, out_stage=L.OUT_WINDOWED), "windowed input"), (dict(in_kind=L.IN_FRAMES, out_stage=L.OUT_FRAMES), "KTF_IN_WAV"),
        (dict(tab=tabs(dct=None)), "DCT"), (dict(tab=tabs(window=None)), "window table"), (dict(tab=tabs(mel_w=None)), "FFT/mel"),
        (dict(tab=tabs(mel_stride=0)), "FFT/mel"), (dict(tab=tabs(reserved=0)), "reserved"), (dict(cfg=None), "null"), (dict(tab=None), "null"),
        (dict(in_kind=L.IN_WAV_I16, n=(1 << 31) - 4096), "n < 2^31"),
        # 128 mels of 1024 bins each beside the tables of nfft 2048: more LDS than a workgroup has
        (dict(cfg=cfg(nfft=2048, frame_size=2048, num_mels=128, num_ceps=13), tab=tabs(mel_stride=1024, fast_tw=None), n=16000), "LDS"),
    ]
    for kw, text in bad:
        a = dict(B=1, n=16000, in_kind=L.IN_WAV, cfg=good, tab=tab, out_stage=L.OUT_MFCC)
        a.update(kw)
        ref = lambda v: None if v is None else C.byref(v)  # noqa: E731
        rc_p = lib.ktf_frontend_plan(a["B"], a["n"], a["in_kind"], ref(a["cfg"]), ref(a["tab"]), a["out_stage"], C.byref(plan))
        msg_p = L.last_error()
        rc_l = lib.ktf_frontend_f32(buf, a["B"], a["n"], a["in_kind"], ref(a["cfg"]), ref(a["tab"]), a["out_stage"], buf, None, 0, None)
        msg_l = L.last_error()
        assert rc_p == rc_l == -1 and text in msg_p and msg_p == msg_l, (kw, rc_p, msg_p, rc_l, msg_l)
    assert lib.ktf_frontend_plan(1, 16000, L.IN_WAV, C.byref(good), C.byref(tab), L.OUT_MFCC, None) == -1 and "null plan" in L.last_error()
    # nothing to launch is not an error, for either
    for B, n, kind in ((0, 16000, L.IN_WAV), (3, 0, L.IN_FRAMES)):
        assert lib.ktf_frontend_plan(B, n, kind, C.byref(good), C.byref(tab), L.OUT_MFCC, C.byref(plan)) == 0 and plan.kernel == L.FE_NONE
        assert lib.ktf_frontend_f32(buf, B, n, kind, C.byref(good), C.byref(tab), L.OUT_MFCC, buf, None, 0, None) == 0
    p = ops.frontend_plan(2, 1000, L.IN_WAV, good, tab, L.OUT_FRAMES)
    assert (p.kernel, p.T, p.grid_x) == (L.FE_FRAMING, 4, -(-2 * 4 * 400 // 256))
