"""Scans of the LDS placements the fused VAD / CMVN launcher (`ktf_vad_cmvn`) and the stand-alone CMVN launcher (`ktf_cmvn_f32`) choose,
through the launchers' own plan queries (`ktf_vad_cmvn_plan`, `ktf_cmvn_plan`: host arithmetic, no GPU). Shared by the CPU test that
pins the plans and the GPU tests that take their T from them, so that a retuned limit moves the tested sizes with it."""

import functools

from kaldi_tflite_amd import ops

T_SCAN = 45000              # beyond the last change of plan of every width in use (the frame map leaves the LDS at 38,401 frames)
LDS_LIMIT = 160 * 1024      # what the launchers opt their kernels in to
VC_GM = 2048                # floats of fixed scratch in front of the placed arrays (csrc/vad_cmvn_common.h)


def placement(p):
    """(map in LDS, rows in LDS, block sums, energy column in LDS, LDS-form instantiation) of a VcPlan."""
    return (p.pos_ints > 0, p.stage_floats > 0, p.bs_floats > 0, p.col_floats > 0, bool(p.lds_form))


def _runs(query):
    """[(first T, last T, placement)] of the maximal runs of T = 1 .. T_SCAN with one placement; every plan is checked for size on the
    way: the LDS bytes are the placed arrays plus the fixed scratch, and within what the kernels are opted in to."""
    runs = []
    for T in range(1, T_SCAN + 1):
        p = query(T)
        assert p.lds_bytes == 4 * (VC_GM + p.pos_ints + p.stage_floats + p.bs_floats + p.col_floats) <= LDS_LIMIT, (T, p.lds_bytes)
        k = placement(p)
        if runs and runs[-1][2] == k:
            runs[-1][1] = T
        else:
            runs.append([T, T, k])
    return tuple(tuple(r) for r in runs)


@functools.lru_cache(maxsize=None)
def fused_runs(D, ldo, B=5):
    return _runs(lambda T: ops.vad_cmvn_plan(B, T, D, ldo))


@functools.lru_cache(maxsize=None)
def cmvn_runs(D, ldo):
    return _runs(lambda T: ops.cmvn_plan(T, D, ldo))


def first_of_each(runs):
    return [r[0] for r in runs]


def both_sides(runs):
    """For every change of plan the last T of the old plan and the first T of the new one."""
    ts = []
    for a, b in zip(runs, runs[1:]):
        ts += [a[1], b[0]]
    return ts


def plan_number(runs, T):
    """1-based number of the run T falls in (the row of INTEGRATION.md's table of placements)."""
    return next(i + 1 for i, r in enumerate(runs) if r[0] <= T <= r[1])
