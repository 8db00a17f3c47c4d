"""fp64 reference, error bounds and comparisons for the 16-bit TDNN kernels (numpy only; no GPU, no torch).

A `case` is a dict of tests/test_gpu_tdnn16_bits.py (ctx, T, units, ldy, act, affine, lens, padding, sub, gemm, mode, y_view, atomic).
`reference(case, x, W, bias, scale, shift)` returns a `Ref`: for every utterance b and output row t < out_len[b] the fp64 value
`want[b, t, u]` the call must produce and a bound `bound[b, t, u]` on |fp32 value the kernel holds - want|. `check(case, ref, raw,
finalized)` compares an output buffer with it in the manner of the case's output form and returns a `Result` (failures, largest
|got - want| / allowed).

The reference.  include/ktf_hip.h:  y = post(act(bias + sum x W)),  row(t, k) clipped per utterance; the rows of utterance b are those of
oracle/ktf_oracle.py::tdnn on x[b, :lens[b]] (VALID padding and subsampling included). The operands are the ones the kernel sees:
KTF_GEMM_BF16 -- x and W rounded to bf16, round to nearest even (also where the kernel rounds fp32 x in registers); KTF_GEMM_BF16X3 -- the
exact fp32 x and W (the hi / lo split is part of the error budget). Everything else is fp64.

The bound.  u = 2^-24 (fp32 unit roundoff), v = 2^-8 (bf16 unit roundoff), A = sum |x W| over the Ktot products of the element, all
from the reference's own terms; no constant is fitted to what a kernel returns.

 1. Accumulation.  bf16 x bf16 products are exact in fp32 (8 + 8 significand bits). A sum of n fp32 terms a_i, in ANY order and
    grouping, is off by at most (n - 1) u sum|a_i| to first order (every one of the n - 1 additions rounds a partial sum that is at most
    sum|a_i|); with the bias among the terms n = Ktot + 1, and  (Ktot + 1) u (A + |bias|)  also pays the second-order terms
    ((1 + u)^n - 1 < (n + 1) u for n u < 0.01). KTF_GEMM_BF16X3 adds three products per (x, w) pair: n = 3 Ktot + 1 terms whose
    magnitudes sum to at most (1 + v)^2 (1 + 2 v (1 + v)) A < 1.02 A:  (3 Ktot + 1) u (1.02 A + |bias|).  (The fp64 reference's own
    error, Ktot 2^-53 A, is 2^-29 of that.)
 2. Operands, KTF_GEMM_BF16X3 only.  hi = bf16(a), lo = bf16(a - hi): |a - hi| <= v |a|, |a - hi - lo| <= v |a - hi| <= v^2 |a|, and
    |lo| <= v (1 + v) |a|. The kernel adds xh wh + xl wh + xh wl = (x - ex)(w - ew) - xl wl with |ex| <= v^2 |x|, |ew| <= v^2 |w|:
    |error| <= (2 v^2 + v^4) |x w| + v^2 (1 + v)^2 |x w| < (3 + 2^-6) 2^-16 |x w|.  Multiple: 3 + 2^-6.
 3. Epilogue.  dz = (1) + (2) bounds the pre-activation z. a = act(z): |da| <= Lip dz + e_act with Lip = 1 (none, ReLU, tanh), 1/4
    (sigmoid); e_act = 0 for none / ReLU (exact in fp32) and item 4 for sigmoid / tanh. With the BatchNorm affine, y = a s + h in fp32
    as a multiply and an add (or one fma, which rounds less): |dy| <= |s| da + u (|a| + da) |s| + u (|y| + |s| da + u (|a| + da) |s|).
    Without it the kernels multiply by 1.0f and add 0.0f: exact, dy = da.
 4. Device expf / tanhf (apply_act, csrc/tdnn_common.h: 1 / (1 + expf(-z)), tanhf(z)).  No accuracy statement for the device library is
    installed with the toolchain, so the figure is MEASURED on the MI355X: the largest deviation of ops.activation_ (same apply_act) from
    fp64, in fp32 ulps of the result, over the pre-activation values of the sigmoid / tanh cases (tests/test_gpu_tdnn16_values.py::
    test_device_activation_ulps measures it and asserts the allowance):  sigmoid 2.09 ulp, tanh 1.38 ulp (the rounding of the result
    included; ROCm 7.2 device library, 759,296 and 1,166,336 values: the cases' own and their fp32 neighbours).
    e_act = ACT_ULPS[act] ulp32(|a|), ACT_ULPS = twice the measured figure.

Comparisons.  fp32 rows: |got - want| <= dy.  bf16 rows: |got - want| <= dy + HALF a bf16 ulp at max(|got|, |want|) (round to nearest;
truncation is off by up to a whole one).  hi / lo planes: hi as a bf16 row; |hi + lo - want| <= dy + 2^-16 |want| (lo = bf16(y - hi)
rounds y - hi, at most v |y|, to v^2 |y| = 2^-16 |y|); |lo| <= half a bf16 ulp of hi (y - hi is at most that, and that is a bf16 number).
Rows at or beyond out_len[b] and columns outside [y_view, y_view + units) keep the sentinel bit for bit.

Pooled sums (pooled_sums16 and flat_stats_runs, csrc/pooled_stats.h).  A slot holds S = sum y, Q = sum y^2 over the
rows of one 128-row block (of the utterance, or of the flat row space) that belong to the utterance. From the rows' values:
|sum y - sum want| <= sum dy and |sum y^2 - sum want^2| <= sum (2 |want| dy + dy^2). The 16x16 kernels sum in fp32 relative to the
pivot p = the slot's first row: each of a column's four lanes takes 32 rows or fewer, u_i = fl(y_i - p) (one rounding), s = sum u_i
(at most 31 additions), q = fma chain of u_i^2 (32 roundings, and u_i^2 carries twice u_i's), then S = s + n p and Q = q + 2 p s + n p^2
in fp64. With d_i = |want_i - want_p| + dy_i + dy_p >= |y_i - p|:  |dS| <= 33 u sum d_i  and  |dQ| <= 35 u sum d_i^2 + 2 (|want_p| +
dy_p) 33 u sum d_i  (a hundredth more for the second order; the fp64 steps add 2^-50 of the magnitudes). The 32x32 kernels add in fp64
and stay inside. The atomic layout's totals are the sum of the same partial sums: the bounds add.
Finalize: mean = S / n, std = sqrt(max(Q / n - mean^2, 0) + eps), both rounded to fp32 once: |d mean| <= dS / n + u |mean|; with
dvar = dQ / n + (2 |mean| + dS / n) dS / n, |d std| <= min(dvar / sqrt(var + eps), sqrt(dvar)) + u |std|.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))

from oracle import ktf_oracle as O  # noqa: E402

GEMM_BF16, GEMM_BF16X3 = 1, 2           # KTF_GEMM_* of include/ktf_hip.h
U32 = 2.0 ** -24
ACT_ULPS = {"sigmoid": 2 * 2.10, "tanh": 2 * 1.38}      # twice the figure measured on the MI355X (docstring, item 4)
X3_OPERANDS = (3 + 2.0 ** -6) * 2.0 ** -16
SENTINEL = 7.0
SLOT_ROWS = 128
POOLED_MODES = ("pooled", "split_pooled", "flat_pooled")
FLAT_MODES = ("flat", "flat_pooled")


# ----------------------------------------------------------------------------- number formats
def bf16_rne(a):
    """fp32 values rounded to bf16 (round to nearest even), as fp32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_trunc(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_bits(a):
    """The 16 bits of values that ARE bf16 numbers."""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_from_bits(b):
    return (np.ascontiguousarray(b).view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def half_ulp_bf16(v):
    """Half a bf16 ulp at |v| (0 at 0): 2^(floor(log2 |v|) - 8)."""
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(v)
    return np.where(v > 0, np.ldexp(1.0, e - 9), 0.0)


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def act64(z, act):
    return O.keras_activation(z, act) if act else z


# ----------------------------------------------------------------------------- the reference
class Ref:
    """want / bound: (B, Tout, units) fp64, rows t >= out_len[b] are NaN. z: the pre-activation values, a: the activation's."""

    def __init__(self, want, bound, out_len, z, a, Tout):
        self.want, self.bound, self.out_len, self.z, self.a, self.Tout = want, bound, out_len, z, a, Tout


def is_x3(c):
    """The plane entry points (ktf_tdnn_split*) are KTF_GEMM_BF16X3 whatever the case's `gemm` field says."""
    return c["gemm"] == GEMM_BF16X3 or c["mode"] in ("split", "split_pooled", "flat", "flat_pooled")


def lens_of(c, B):
    return np.array(c["lens"], np.int64) if c["lens"] else np.full(B, c["T"], np.int64)


def out_rows(c, n):
    return 0 if n <= 0 else O.tdnn_eval_indices(int(n), list(c["ctx"]), c["sub"], c["padding"]).shape[0]


def reference(c, x, W, bias, scale=None, shift=None):
    x3 = is_x3(c)
    xq = np.asarray(x, np.float32) if x3 else bf16_rne(x)
    Wq = np.asarray(W, np.float32) if x3 else bf16_rne(W)
    if x3:
        return reference_on(c, xq, Wq, bias, scale, shift, lambda A, b, ktot: (3 * ktot + 1) * U32 * (1.02 * A + b) + X3_OPERANDS * A)
    return reference_on(c, xq, Wq, bias, scale, shift, lambda A, b, ktot: (ktot + 1) * U32 * (A + b))


def reference_on(c, xq, Wq, bias, scale, shift, dz_of, mag=None):
    """The Ref of case c on the operands xq, Wq as the kernel sees them. dz_of(A, |bias|, Ktot): the bound on the pre-activation value
    (items 1 and 2 of the docstring; tests/_tdnn32_ref.py passes the fp32 families' own), the epilogue's share (items 3 and 4) is added here.
    mag: the (x, W) magnitudes that A is the sum of products of, where they are not |xq|, |Wq| themselves."""
    xq, Wq = np.asarray(xq, np.float64), np.asarray(Wq, np.float64)
    xa, Wa = (np.abs(xq), np.abs(Wq)) if mag is None else mag
    B, T, D = xq.shape
    U, ktot = Wq.shape
    lens = lens_of(c, B)
    Tout = out_rows(c, T)
    kw = dict(context=list(c["ctx"]), subsampling_factor=c["sub"], padding=c["padding"], activation=None, dtype=np.float64)
    z = np.full((B, Tout, U), np.nan)
    A = np.full((B, Tout, U), np.nan)
    out_len = np.zeros(B, np.int64)
    b64 = np.asarray(bias, np.float64)
    for b in range(B):
        n = int(lens[b])
        out_len[b] = out_rows(c, n)
        if out_len[b] == 0:
            continue
        z[b, :out_len[b]] = O.tdnn(xq[b:b + 1, :n], Wq, b64, **kw)[0]
        A[b, :out_len[b]] = O.tdnn(xa[b:b + 1, :n], Wa, None, **kw)[0]
    dz = dz_of(A, np.abs(b64), ktot)
    act = c["act"]
    with np.errstate(invalid="ignore"):
        a = act64(z, act)
        lip = 0.25 if act == "sigmoid" else 1.0
        da = lip * dz + (ACT_ULPS[act] * ulp32(np.nan_to_num(a)) if act in ACT_ULPS else 0.0)
        if scale is None:
            want, bound = a, da
        else:
            s, h = np.asarray(scale, np.float64), np.asarray(shift, np.float64)
            want = a * s + h
            mul = U32 * (np.abs(a) + da) * np.abs(s)
            bound = np.abs(s) * da + mul + U32 * (np.abs(want) + np.abs(s) * da + mul)
    return Ref(want, bound, out_len, z, a, Tout)


# ----------------------------------------------------------------------------- slots of the pooled forms
def slot_rows(c, out_len):
    """[(b, slot, first row, end row)] of the partial sums the finalize reads: 128-row blocks of the utterance, or -- flat modes -- of the
    flat row space (utterance b starts at flat row sum(out_len[:b]))."""
    res = []
    s0 = 0
    rows = c.get("slot_rows", SLOT_ROWS)                  # (the pair kernel's slots hold 64 rows: tests/_tdnn32_ref.py)
    for b, n in enumerate(int(v) for v in out_len):
        base = s0 if c["mode"] in FLAT_MODES else 0
        if n > 0:
            first = base // rows
            for blk in range(first, (base + n - 1) // rows + 1):
                lo, hi = max(blk * rows, base) - base, min((blk + 1) * rows, base + n) - base
                res.append((b, blk - first, lo, hi))
        s0 += n
    return res


def slot_sums(ref, lo, hi, b):
    """fp64 S, Q of rows [lo, hi) of utterance b and their bounds (docstring: pooled sums)."""
    w, d = ref.want[b, lo:hi], ref.bound[b, lo:hi]
    S, Q = w.sum(0), (w * w).sum(0)
    di = np.abs(w - w[0]) + d + d[0]
    eS = 1.01 * 33 * U32 * di.sum(0)
    eQ = 1.01 * 35 * U32 * (di * di).sum(0) + 2 * (np.abs(w[0]) + d[0]) * eS
    bS = d.sum(0) + eS + 2.0 ** -50 * np.abs(w).sum(0)
    bQ = (2 * np.abs(w) * d + d * d).sum(0) + eQ + 2.0 ** -50 * Q
    return S, Q, bS, bQ


def finalize64(S, Q, n, eps):
    mean = S / n
    return mean, np.sqrt(np.maximum(Q / n - mean * mean, 0.0) + eps)


# ----------------------------------------------------------------------------- comparisons
class Result:
    def __init__(self):
        self.failures, self.ratio = [], 0.0

    @property
    def ok(self):
        return not self.failures

    def close(self, what, got, want, allowed):
        got, want, allowed = (np.asarray(v, np.float64) for v in (got, want, allowed))
        err = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(allowed > 0, err / allowed, np.where(err > 0, np.inf, 0.0))
        bad = ~(err <= allowed)                                  # (a NaN fails)
        if r.size:
            self.ratio = max(self.ratio, float(np.nanmax(np.where(np.isnan(r), np.inf, r))))
        if bad.any():
            i = np.unravel_index(int(np.argmax(np.where(bad, np.where(np.isnan(r), np.inf, r), -1.0))), bad.shape)
            self.failures.append(f"{what}: {int(bad.sum())} of {bad.size} outside the bound; worst at {tuple(int(k) for k in i)}: got "
                                 f"{got[i]!r}, want {want[i]!r}, allowed {allowed[i]:.3e}")

    def true(self, what, cond):
        cond = np.asarray(cond)
        if not cond.all():
            i = np.unravel_index(int(np.argmin(cond)), cond.shape) if cond.shape else ()
            self.failures.append(f"{what}: {int((~cond).sum())} of {cond.size} elements, first at {tuple(int(k) for k in i)}")


def _untouched(res, what, buf, c, ref):
    """Rows at or beyond out_len[b] and columns outside [col0, col0 + units) of (B, Tout, ld) `buf` hold the sentinel's bits."""
    if buf.dtype == np.uint16:
        keep = buf == bf16_bits(np.float32(SENTINEL))
    else:
        keep = buf.view(np.uint32) == np.float32(SENTINEL).view(np.uint32)
    col0 = c["y_view"] or 0
    written = np.zeros(buf.shape, bool)
    for b, n in enumerate(ref.out_len):
        written[b, :n, col0:col0 + c["units"]] = True
    res.true(f"{what}: rows beyond out_len and pad columns keep the sentinel", keep | written)


def _valid(ref):
    m = np.zeros(ref.want.shape[:2], bool)
    for b, n in enumerate(ref.out_len):
        m[b, :n] = True
    return m


def check(c, ref, raw, finalized=None, eps=1e-10):
    """raw: the whole output buffer as numpy -- fp32 rows (B, Tout, ld) float32; bf16 rows (B, Tout, ld) uint16 bits; planes (2, B, Tout,
    ld) uint16 bits; pooled (B, slots, 2, units) or (B, 2, units) float64. finalized: (B, >= 2 units) mean | std of the pooled forms."""
    res = Result()
    U = c["units"]
    if c["mode"] in POOLED_MODES:
        _check_pooled(res, c, ref, raw, finalized, eps)
        return res
    col0 = c["y_view"] or 0
    m = _valid(ref)
    want, bound = ref.want[m], ref.bound[m]
    if raw.dtype == np.float32:
        assert raw.shape == (ref.want.shape[0], ref.Tout, c["ldy"]), raw.shape
        _untouched(res, "y", raw, c, ref)
        res.close("fp32 rows", raw[:, :, col0:col0 + U][m], want, bound)
        return res
    assert raw.dtype == np.uint16
    planes = raw.ndim == 4
    hi_bits = raw[0] if planes else raw
    _untouched(res, "y", hi_bits, c, ref)
    hi = bf16_from_bits(hi_bits)[:, :, col0:col0 + U][m].astype(np.float64)
    res.close("bf16 rows", hi, want, bound + half_ulp_bf16(np.maximum(np.abs(hi), np.abs(want))))
    if planes:
        _untouched(res, "y_lo", raw[1], c, ref)
        lo = bf16_from_bits(raw[1])[:, :, col0:col0 + U][m].astype(np.float64)
        res.close("hi + lo", hi + lo, want, bound + 2.0 ** -16 * np.abs(want))
        res.true("|lo| <= half a bf16 ulp of hi", np.abs(lo) <= half_ulp_bf16(hi))
    return res


def _check_pooled(res, c, ref, raw, finalized, eps):
    B, U = ref.want.shape[0], c["units"]
    det = raw.ndim == 4
    tot = np.zeros((B, 2, U))
    tot_b = np.zeros((B, 2, U))
    for b, k, lo, hi in slot_rows(c, ref.out_len):
        S, Q, bS, bQ = slot_sums(ref, lo, hi, b)
        if det:
            res.close(f"sum, utterance {b} slot {k}", raw[b, k, 0], S, bS)
            res.close(f"sum of squares, utterance {b} slot {k}", raw[b, k, 1], Q, bQ)
        tot[b] += (S, Q)
        tot_b[b] += (bS, bQ)
    tot_b += 2.0 ** -50 * np.abs(tot)
    if not det:
        res.close("atomic sums", raw, tot, tot_b)
    if finalized is None:
        return
    for b, n in enumerate(int(v) for v in ref.out_len):
        if n == 0:
            continue                                                      # 0 / 0: no statement
        mean, std = finalize64(tot[b, 0], tot[b, 1], n, eps)
        dS, dQ = tot_b[b, 0] / n, tot_b[b, 1] / n
        dvar = dQ + (2 * np.abs(mean) + dS) * dS
        res.close(f"mean, utterance {b}", finalized[b, :U], mean, dS + U32 * np.abs(mean))
        res.close(f"std, utterance {b}", finalized[b, U:2 * U], std, np.minimum(dvar / std, np.sqrt(dvar)) + U32 * std)
