"""fp64 reference, error bounds and comparisons for the KTF_GEMM_F16MX TDNN kernels (csrc/tdnn_mx.hip, csrc/tdnn_mxl.hip, csrc/tdnn_mx_epilogue.inc,
csrc/tdnn_mx_common.h, csrc/pooled_stats.h), on top of tests/_tdnn16_ref.py (numpy only; no GPU, and no torch until a function needs the codecs of
kaldi_tflite_amd/mx.py): the same `case` dicts, Ref, Result, `check` vocabulary, SENTINEL and the lens pattern (T, 1, 0, T - 1, T // 2 + 1).

A `case` (`case()` below) names one launch: the kernel `family` ("tile": tdnn_mx_kernel on per-utterance 256-row tiles, "flat":
tdnn_mx_kernel<flat>, "loader": tdnn_mxl_kernel), the output form `out` ("f32" rows, "planes", "pooled"; `atomic`: the (B, 2, units) totals
instead of the reproducible slots), the layer (ctx, din, units, act, affine, padding, sub), the batch (T, lens) and the kind of `inputs`.

The reference.  The operands are what the MFMAs see, as fp64: from the activations mx.encode_activations / mx.decode_e2m1 give x_h (half),
x_l4 (e2m1 image of x - x_h), x_4 (e2m1 image of x_h); from the weights mx.weight_images(...)[2] (the same numbers as
mx.weight_images_loader's) gives w_h, w_4, w_l6 in the K-step layout of the kernels (din padded to 32, units to 256, K-step = (32-feature
chunk, context offset)). The value a call must produce is the kernels' own three products

    z = bias + sum x_h w_h + x_l4 w_4 + x_4 w_l6,      y = post(act(z)),

NOT x . w: what the three-term arithmetic costs against the exact layer is measured in tests/test_gpu_mx.py. The three products are ONE
GEMM over a K three times as long ([x_h | x_l4 | x_4] against [w_h | w_4 | w_l6] per context offset), so _tdnn16_ref.reference_on is
used as it is: rows, clamping, VALID padding and subsampling are those of oracle/ktf_oracle.py::tdnn.

The bound on z.  u = 2^-24, Ktot = 32 nk (nk = din_pad / 32 * contexts), A3 = sum |x_h||w_h| + |x_l4||w_4| + |x_4||w_l6| from the
reference's own terms; nothing is fitted to what a kernel returns.
 1. Products.  half x half products are exact in fp32 (11 + 11 significand bits). e2m1 x e2m1 and e2m1 x e2m3 products have at most
    2 + 4 significand bits and the E8M0 block scales are powers of two: exact, unless the sum of the two scale exponents leaves fp32's
    range at the bottom; such a product is smaller than 2^-126 and is allowed as an absolute 2^-126 (item 3).
 2. Accumulation.  The order inside v_mfma_f32_16x16x32_f16 and v_mfma_scale_f32_16x16x128_f8f6f4 is not documented, so every one of
    the 3 Ktot products and the bias counts as one fp32 term added in ANY order and grouping (as tests/_tdnn32_ref.py does for the pair
    kernel): n = 3 Ktot + 1 terms, at most n - 1 roundings of partial sums that never exceed A3 + |bias|, and (1 + u)^n - 1 < (n + 1) u
    for n u < 0.01 pays the second order:  (3 Ktot + 2) u (A3 + |bias|).  (The 256-row kernel adds the bias in the epilogue, the loader
    kernel starts its accumulators at it: both are one of the n terms. Zero-padded K-steps add exact zeros.)
 2a. SUBNORMAL halves count at the magnitude their exponent field names:  in A3, |x_h| and |w_h| are max(|h|, 2^-14) for h != 0.
    "One fp32 rounding per term" presumes that a product enters the sum with 24 bits below ITS OWN leading bit. The adder of
    v_mfma_f32_16x16x32_f16 places a product by the operands' exponent FIELDS; a subnormal half (field 0 = 2^-14, z leading zero
    bits in the mantissa) yields a product that sits z bits lower in that window and loses z bits. Found by this harness, not assumed:
    with weight rows of 2^-26 .. 2^-15 (every w_h subnormal) the fp32 output of tdnn_mx_kernel left the bound of item 2 by up to 2.32 x,
    the error a constant ~1e-10 from w ~ 2^-25 to w ~ 2^-15 (relative to the products: 2^-14 where z = 10). Launched with single terms
    switched off, the half-precision pass alone reproduced that error to the last digit while both block-scaled passes stayed
    within 1e-14 of their fp64 sums -- it is the instruction, not the kernel. Measured against the magnitudes the fields name, those
    units sit at 0.004 of the bound, where units with normal weights sit (0.002 - 0.006). Halves of 2^-14 and above are not affected:
    this term changes no bound unless an operand is a non-zero subnormal half. Models keep weights far above 2^-14; the case
    "tile_f32_wide" of tests/test_gpu_tdnn_mx_values.py is there to hold this statement.
 3. dz = (3 Ktot + 2) u (A3 + |bias|) + 3 Ktot 2^-126.   (The fp64 reference's own error, 3 Ktot 2^-53 A3, is 2^-29 of that.)
 4. Epilogue.  ReLU is exact; the BatchNorm affine is a multiply and an add (or one fma); the pivot-relative pooled sums and the finalize:
    item 3 and "pooled sums" of tests/_tdnn16_ref.py, unchanged. Both kernels give a lane at most 32 rows of a slot (8 x 4 in the
    128-row blocks of the 256-row kernel, 6 x 4 in the loader kernel's 96-row blocks), which is what the 33 u / 35 u there count:
    `slot_rows` is 128, or 96 with KTF_TDNN_MX_LOADER; the flat forms cut the slots along the flat row space (FLAT_MODES).
 5. Exact cases (`inputs` "exact").  If all 3 Ktot products, the bias, and the affine's product and shift are multiples of one power of
    two q, and the sums of their magnitudes stay below 2^24 q, every partial sum in every order is an fp32 number: no rounding happens
    anywhere and the bound is ZERO (`exact_condition` certifies this from the decoded operands; tests/test_tdnn_mx_ref_cpu.py asserts it).

Comparisons.  fp32 rows and the pooled forms: `check` of tests/_tdnn16_ref.py (every element inside its own bound; rows beyond out_len[b]
and pad columns keep the sentinel). Plane outputs: `check_planes`. Call y32 the fp32 value the kernel held, |y32 - want_c| <= bound with
want_c = clip(want, +-65504) (clipping is a contraction):
 (a) half plane: x_h = half(y32), round to nearest: |x_h - want_c| <= bound + half an fp16 ulp at max(|x_h|, |want_c|) (below 2^-14 the
     spacing is the subnormal 2^-24).
 (b) the value image is a function of the half plane alone: the x_4 codes and the value-scale byte equal mx.encode_e2m1 / mx.scale_bytes of
     the OBSERVED x_h block bit for bit (+0 and -0 codes are one number).
 (c) residual image. The residual y32 - x_h is exact in fp32 and its code is the nearest e2m1 number on the block's scale 2^(sl - 127):
     |x_h + decode(x_l4) - want_c| <= bound + (half the e2m1 spacing at the decoded magnitude: 1/4 below 2, 1/2 at 2 and 3, 1 at 4 and 6)
     2^(sl - 127) -- no saturation term, because |residual| <= half an fp16 ulp of the block's largest |x_h| and the scale rule keeps
     the block maximum at or below 6; and a trivially large scale does not pass: sl <= scale_bytes(largest bound of the block + half an
     fp16 ulp of the block's largest |x_h|).
 (d) units units .. 32 nch_out - 1 of the last chunk decode to exact zero in all three images (a non-zero pad unit would change the
     block's scales).
 (e) records of rows at or beyond out_len[b] keep the fill byte in all four planes.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "kaldi-tflite_amd"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _tdnn16_ref as R  # noqa: E402
from _tdnn16_ref import SENTINEL, Ref, Result  # noqa: E402,F401

U32 = R.U32
HALF_MAX = 65504.0
FILL = 0x5A                                   # plane outputs are pre-filled with this byte
B = 5
EPS = 1e-10
FAMILY = {"tile": "tdnn_mx_kernel", "flat": "tdnn_mx_kernel<flat>", "loader": "tdnn_mxl_kernel"}
DEAD_UNIT, CONST_UNIT = 5, 6                  # weights 0: bias -1 (dead behind a ReLU) and 0.7 ("gauss" and "wide" inputs)
E2M1_HALF_SPACING = np.array([0.25, 0.25, 0.25, 0.25, 0.5, 0.5, 1.0, 1.0])        # by magnitude code: 0 .5 1 1.5 | 2 3 | 4 6


def _mx():
    from kaldi_tflite_amd import mx
    return mx


def lens_for(T):
    return (T, 1, 0, T - 1, T // 2 + 1)


def cdiv(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------- cases
def case(name, family, out, K, T, units=260, ldy=None, act="relu", affine=False, lens="ragged", padding="SAME", sub=1, atomic=False,
         inputs="gauss", zeros=False, seed=1, batch=B):
    """K = (context offsets, din). lens: "ragged" = lens_for(T), None = no lens argument, or the lengths. zeros: ReLU-like inputs (negative
    values replaced by 0) instead of signed ones."""
    assert family in FAMILY and out in ("f32", "planes", "pooled") and inputs in ("gauss", "wide", "exact")
    lens = lens_for(T) if lens == "ragged" else (tuple(int(n) for n in lens) if lens is not None else None)
    nb = len(lens) if lens is not None else batch
    mode = ("flat_pooled" if family == "flat" else "pooled") if out == "pooled" else ("flat" if family == "flat" else "store")
    return dict(name=name, family=family, kernel=FAMILY[family], out=out, ctx=list(K[0]), din=K[1], T=T, units=units,
                ldy=(units if ldy is None else ldy) if out == "f32" else None, act=act, affine=affine, lens=lens, B=nb, padding=padding, sub=sub,
                atomic=atomic, inputs=inputs, zeros=zeros, seed=seed, mode=mode, y_view=None, gemm="f16mx",
                slot_rows=96 if family == "loader" else 128)


def nk_of(c):
    return cdiv(c["din"], 32) * len(c["ctx"])


def instance_of(c):
    """(kernel, ACT, OUT, PADK or None, flat) of the instantiation the launchers pick for the case (mx_launch, csrc/tdnn_mx.hip; mxl_launch,
    csrc/tdnn_mxl.hip): PADK = (nk & 3) != 0 on the 256-row kernel, the loader kernel from the flag, flat tiles from the entry point."""
    loader = c["family"] == "loader"
    out = {"f32": "F32", "planes": "PLANES", "pooled": "STATS"}[c["out"]]
    return ("tdnn_mxl_kernel" if loader else "tdnn_mx_kernel", "RELU" if c["act"] == "relu" else "NONE", out,
            None if loader else (nk_of(c) & 3) != 0, c["family"] == "flat")


def all_instances():
    """The 26 kernels the launchers choose among."""
    acts = ("RELU", "NONE")
    return ({("tdnn_mx_kernel", a, o, k, False) for a in acts for o in ("STATS", "F32", "PLANES") for k in (True, False)}
            | {("tdnn_mx_kernel", a, o, k, True) for a in acts for o in ("STATS", "PLANES") for k in (True, False)}
            | {("tdnn_mxl_kernel", a, o, None, False) for a in acts for o in ("STATS", "F32", "PLANES")})


def inputs(c):
    """x (B, T, din), W (units, contexts, din), bias, scale, shift (None without the affine) of a case, all float32.
    "gauss": signed Gaussian features with a per-feature power-of-two spread (zeros: ReLU-like), one all-zero 32-feature block, a dead and
    a constant unit. "wide": the same, weight rows and biases scaled per unit by 2^-28 .. 2^15 (outputs from subnormal halves to beyond
    65504). "exact": item 5 of the docstring -- x = m (1 + c 2^-14 / |m|) with m in {0, +-1, +-2} and c in {2, 4, 6};
    w = m' (1 + e 2^-14 / |m'|) with m' in {+-1, +-2}, e in {4, 6}; integer bias, scale and shift: x_h = m, x - x_h on the e2m1 grid, w_h = m',
    w - w_h on the e2m3 grid, and all three products are non-zero multiples of 2^-13."""
    rng = np.random.default_rng([c["seed"], c["T"], c["din"], len(c["ctx"]), c["units"]])
    nb, T, D, U, K = c["B"], c["T"], c["din"], c["units"], len(c["ctx"])
    if c["inputs"] == "exact":
        m = rng.choice([0, 0, 0, 0, 1, -1, 2, -2], (nb, T, D)).astype(np.float64)
        x = m + np.sign(m) * rng.choice([2, 4, 6], (nb, T, D)) * 2.0 ** -14          # (away from zero: m is a power of two, the half
        W = rng.choice([1, -1, 2, -2], (U, K, D)).astype(np.float64)                  # spacing below it is half of the one above)
        W = W + np.sign(W) * rng.choice([4, 6], (U, K, D)) * 2.0 ** -14
        bias = rng.integers(-3, 4, U).astype(np.float64)
        scale, shift = rng.choice([1, -1, 2, -2], U).astype(np.float64), rng.integers(-2, 3, U).astype(np.float64)
    else:
        x = rng.standard_normal((nb, T, D)) * np.exp2(rng.integers(-3, 3, (1, 1, D)))
        if c["zeros"]:
            x = np.maximum(x, 0.0)
        x[min(1, nb - 1), min(3, T - 1), :min(D, 32)] = 0.0                   # an all-zero 32-block
        W = rng.standard_normal((U, K, D)) / np.sqrt(K * D)
        bias = rng.standard_normal(U) * 0.1
        W[DEAD_UNIT], bias[DEAD_UNIT] = 0.0, -1.0
        W[CONST_UNIT], bias[CONST_UNIT] = 0.0, 0.7
        if c["inputs"] == "wide":
            e = np.exp2((np.arange(U) * 7) % 44 - 28.0)           # (the weights themselves stay below the largest half)
            W, bias = W * e[:, None, None], bias * e
        scale = rng.uniform(0.5, 2.0, U) * rng.choice([1.0, -1.0], U)
        shift = rng.standard_normal(U)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    if not c["affine"]:
        return f(x), f(W), f(bias), None, None
    return f(x), f(W), f(bias), f(scale), f(shift)


# ----------------------------------------------------------------------------- operands
def pad_features(x):
    nb, T, D = x.shape
    xp = np.zeros((nb, T, cdiv(D, 32) * 32), np.float32)
    xp[:, :, :D] = x
    return xp


def kstep_weights(W):
    """(units, contexts, din) -> float64 (units padded to 256, nk, 32) in the K-step order (32-feature chunk, context offset) that
    layers.TDNN.device_weights_mx hands to mx.weight_images / mx.weight_images_loader."""
    U, K, D = W.shape
    Dp, Up = cdiv(D, 32) * 32, cdiv(U, 256) * 256
    Wp = np.zeros((Up, K, Dp))
    Wp[:U, :, :D] = W
    return np.ascontiguousarray(Wp.reshape(Up, K, Dp // 32, 32).transpose(0, 2, 1, 3)).reshape(Up, (Dp // 32) * K, 32)


def _context_major(Wd, U, K, nch):
    """decoded (Up, nkp, 32) in K-step order -> (U, K, nch * 32)."""
    return Wd[:U, :nch * K].reshape(U, nch, K, 32).transpose(0, 2, 1, 3).reshape(U, K, nch * 32)


def operands(c, x, W, decoded=True):
    """xq (B, T, 3 din_pad) = [x_h | x_l4 | x_4] and Wq (units, contexts * 3 din_pad) = per context offset [w_h | w_4 | w_l6], fp64: the
    operands of the one long GEMM. decoded=False: [x | 0 | 0] and [w | 0 | 0] through the same layout code (the exact layer)."""
    mx = _mx()
    xp = pad_features(x)
    nb, T, Dp = xp.shape
    U, K, _ = W.shape
    nch = Dp // 32
    Wi = kstep_weights(W)
    if decoded:
        xh, cl, ch, sl, sh = mx.encode_activations(xp)
        blk = (nb, T, nch, 32)
        xs = [xh.astype(np.float64), mx.decode_e2m1(cl.reshape(blk), sl).reshape(nb, T, Dp), mx.decode_e2m1(ch.reshape(blk), sh).reshape(nb, T, Dp)]
        ws = mx.weight_images(Wi)[2]
    else:
        xs = [xp.astype(np.float64), np.zeros((nb, T, Dp)), np.zeros((nb, T, Dp))]
        ws = [Wi, np.zeros_like(Wi), np.zeros_like(Wi)]
    xq = np.concatenate(xs, -1)
    Wq = np.concatenate([_context_major(w, U, K, nch) for w in ws], -1).reshape(U, K * 3 * Dp)
    return xq, Wq


def nominal_halves(m):
    """In place: magnitudes of non-zero subnormal halves -> 2^-14, the magnitude their exponent field names (item 2a)."""
    m[(m > 0) & (m < 2.0 ** -14)] = 2.0 ** -14
    return m


def dz_mx(A, b, ktot3):
    """Items 2 and 3 of the docstring; ktot3 = 3 Ktot, the K of the long GEMM."""
    return (ktot3 + 2) * U32 * (A + b) + ktot3 * 2.0 ** -126


def reference(c, x, W, bias, scale=None, shift=None, decoded=True):
    """The Ref of the case (want, bound per element); `A3` and `ktot3` are kept on it. Exact cases: the bound is zero (item 5)."""
    xq, Wq = operands(c, x, W, decoded)
    mag = (np.abs(xq), np.abs(Wq))
    if decoded:                                                  # item 2a: the x_h columns, the w_h columns of every context offset
        Dp = xq.shape[-1] // 3
        nominal_halves(mag[0][..., :Dp])
        nominal_halves(mag[1].reshape(Wq.shape[0], -1, 3, Dp)[:, :, 0])
    keep = {}

    def dz_of(A, b, ktot3):
        keep["A3"], keep["ktot3"] = A, ktot3
        return np.zeros_like(A) if c["inputs"] == "exact" else dz_mx(A, b, ktot3)

    ref = R.reference_on(c, xq, Wq, bias, scale, shift, dz_of, mag=mag)
    ref.A3, ref.ktot3 = keep["A3"], keep["ktot3"]
    if c["inputs"] == "exact":
        ref.bound = np.where(np.isnan(ref.want), np.nan, 0.0)
    return ref


def pow2_grid(a):
    """Largest e such that every element of a is a multiple of 2^e (None for all zeros)."""
    a = np.asarray(a, np.float64)
    a = a[a != 0]
    if a.size == 0:
        return None
    mant, ex = np.frexp(np.abs(a))
    m = (mant * 2.0 ** 53).astype(np.uint64)
    tz = np.zeros(m.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        low = (m & np.uint64((1 << s) - 1)) == 0
        tz += np.where(low, s, 0)
        m = np.where(low, m >> np.uint64(s), m)
    return int((ex - 53 + tz).min())


def exact_condition(c, x, W, bias, scale=None, shift=None):
    """(q exponent, largest sum of magnitudes) and whether item 5 of the docstring holds, from the DECODED operands alone."""
    xq, Wq = operands(c, x, W)
    Dp = xq.shape[-1] // 3
    K = len(c["ctx"])
    Wk = Wq.reshape(Wq.shape[0], K, 3, Dp)
    grids = []
    for j in range(3):
        gx, gw = pow2_grid(xq[..., j * Dp:(j + 1) * Dp]), pow2_grid(Wk[:, :, j])
        assert gx is not None and gw is not None, "all three products are non-zero"
        grids.append(gx + gw)
    gb = pow2_grid(bias)
    q = min(grids + ([gb] if gb is not None else []))
    ref = reference(c, x, W, bias, scale, shift)
    with np.errstate(invalid="ignore"):
        top = np.nanmax(ref.A3 + np.abs(np.asarray(bias, np.float64)))
        ok = top < 2.0 ** (24 + q)
        if scale is not None:
            gs, gh = pow2_grid(scale), pow2_grid(shift)
            q2 = min(q + gs, gh if gh is not None else q + gs)
            top2 = np.nanmax(np.abs(ref.a) * np.abs(scale) + np.abs(shift))
            ok = ok and top2 < 2.0 ** (24 + q2)
            top = max(top, top2)
    return q, float(top), bool(ok)


# ----------------------------------------------------------------------------- planes on the host
def pack_planes(xh, cl, ch, sl, sh, lens=None, fill=None):
    """mx.encode_activations' output ((B, T, D) half, l4 codes, x4 codes; (B, T, D / 32) scale bytes) -> the four device layouts of mx.Planes
    as numpy: xh (B, nch, T, 32) uint16 bits, xl4 / x4 (B, nch, T, 16) uint8 (mx.pack4), xs (B, nch, T) uint32 = sl | sh << 8. Rows at or
    beyond lens[b]: every byte `fill`, or -- fill None -- poison: half NaN bit patterns, code bytes 0xFF, scale bytes 0xFF, so that any
    read of such a row turns the output NaN."""
    mx = _mx()
    nb, T, Dp = xh.shape
    nch = Dp // 32
    blk = (nb, T, nch, 32)
    t = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1, 3))
    ph = t(np.ascontiguousarray(xh, np.float16).view(np.uint16).reshape(blk))
    pl, p4 = t(mx.pack4(cl.reshape(blk))), t(mx.pack4(ch.reshape(blk)))
    ps = np.ascontiguousarray((sl.astype(np.uint32) | (sh.astype(np.uint32) << 8)).transpose(0, 2, 1))
    if lens is not None:
        for b, n in enumerate(int(v) for v in lens):
            if fill is None:
                ph[b, :, n:], pl[b, :, n:], p4[b, :, n:], ps[b, :, n:] = 0x7E00, 0xFF, 0xFF, 0xFFFF
            else:
                ph[b, :, n:], pl[b, :, n:], p4[b, :, n:], ps[b, :, n:] = fill * 0x0101, fill, fill, fill * 0x01010101
    return ph, pl, p4, ps


def unpack_planes(ph, pl, p4, ps):
    """The inverse: device layouts -> (x_h float16 (B, T, D), l4 codes, x4 codes, sl, sh (B, T, nch)), as mx.Planes.decode reads them."""
    mx = _mx()
    nb, nch, T, _ = ph.shape
    rows = lambda a: a.transpose(0, 2, 1, 3).reshape(nb, T, nch * 32)
    s = ps.astype(np.uint32).transpose(0, 2, 1)
    return (rows(np.ascontiguousarray(ph).view(np.float16)), rows(mx.unpack4(pl)), rows(mx.unpack4(p4)), (s & 255).astype(np.uint8),
            ((s >> 8) & 255).astype(np.uint8))


def input_planes(c, x):
    """The host-built input planes of a case, rows beyond the lengths poisoned."""
    return pack_planes(*_mx().encode_activations(pad_features(x)), lens=R.lens_of(c, x.shape[0]))


# ----------------------------------------------------------------------------- comparisons
def half_ulp_f16(v):
    """Half an fp16 ulp at |v|: 2^(floor(log2 |v|) - 11), and half the subnormal spacing 2^-24 below 2^-14."""
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(v)
    return np.ldexp(1.0, np.where(v > 0, np.maximum(e - 12, -25), -25))


def _canon(codes):
    """e2m1 codes with -0 folded onto +0."""
    return codes & np.where((codes & 7) == 0, 7, 15).astype(np.uint8)


def check_planes(c, ref, xh_bits, l4_codes, x4_codes, scales, fill=FILL):
    """The four output planes in their device layouts -- xh_bits (B, nch, Tout, 32) uint16, l4_codes / x4_codes (B, nch, Tout, 16) uint8
    (two codes per byte), scales (B, nch, Tout) uint32 words -- against the Ref: comparisons (a) to (e) of the docstring."""
    mx = _mx()
    res = Result()
    U = c["units"]
    nb, nch, Tout, _ = xh_bits.shape
    assert nch == cdiv(U, 32) and Tout == ref.Tout and nb == ref.want.shape[0], (xh_bits.shape, ref.want.shape)
    m = R._valid(ref)
    for what, a in (("x_h", xh_bits), ("x_l4", l4_codes), ("x_4", x4_codes), ("scales", scales)):       # (e)
        by = np.ascontiguousarray(a).view(np.uint8).reshape(nb, nch, Tout, -1)
        res.true(f"(e) {what}: records of rows beyond out_len keep the fill byte", (by == fill) | m[:, None, :, None])
    if not m.any():
        return res
    xh16, cl, c4, sl, sh = unpack_planes(xh_bits, l4_codes, x4_codes, scales)
    xh, cl, c4, sl, sh = xh16[m].astype(np.float64), cl[m], c4[m], sl[m], sh[m]                        # (N, 32 nch) / (N, nch)
    N = xh.shape[0]
    want_c = np.clip(ref.want[m], -HALF_MAX, HALF_MAX)
    bound = ref.bound[m]
    blk = (N, nch, 32)
    finite = np.isfinite(xh)
    xz = np.where(finite, xh, 0.0)
    # (a)
    res.close("(a) half plane", xh[:, :U], want_c, bound + half_ulp_f16(np.maximum(np.abs(xz[:, :U]), np.abs(want_c))))
    # (b)
    sh_want = mx.scale_bytes(np.abs(xz.reshape(blk)).max(-1), "e2m1")
    res.true("(b) value-scale byte == scale_bytes(observed x_h block)", sh == sh_want)
    res.true("(b) x_4 codes == encode_e2m1(observed x_h block)", _canon(c4) == _canon(mx.encode_e2m1(xz.reshape(blk), sh_want).reshape(N, -1)))
    # (c)
    dl = mx.decode_e2m1(cl.reshape(blk), sl).reshape(N, -1)
    quant = (E2M1_HALF_SPACING[cl & 7].reshape(blk) * np.exp2(sl.astype(np.float64) - 127.0)[..., None]).reshape(N, -1)
    res.close("(c) half + residual image", (xh + dl)[:, :U], want_c, bound + quant[:, :U])
    bpad = np.zeros((N, nch * 32))
    bpad[:, :U] = np.nan_to_num(bound, nan=np.inf)
    room = bpad.reshape(blk).max(-1) + half_ulp_f16(np.abs(xz.reshape(blk)).max(-1))
    res.true("(c) residual scale byte <= scale_bytes(bound + half an fp16 ulp of the block's largest |x_h|)",
             sl.astype(np.int64) <= mx.scale_bytes(np.minimum(room, 2.0 ** 120), "e2m1").astype(np.int64))
    # (d)
    if nch * 32 > U:
        res.true("(d) pad units: half plane is zero", xh[:, U:] == 0)
        res.true("(d) pad units: residual codes are zero", (cl[:, U:] & 7) == 0)
        res.true("(d) pad units: value codes are zero", (c4[:, U:] & 7) == 0)
    return res


def check(c, ref, raw, finalized=None, eps=EPS):
    """raw: fp32 rows (B, Tout, ldy) float32; planes: the tuple (xh_bits, l4_codes, x4_codes, scales); pooled: (B, slots, 2, units) or
    (B, 2, units) float64 with `finalized` (B, >= 2 units) mean | std."""
    if c["out"] == "planes":
        return check_planes(c, ref, *raw)
    res = R.check(c, ref, raw, finalized, eps)
    if c["out"] == "pooled" and not c["atomic"] and c["inputs"] != "exact":
        _check_constant_units(res, c, ref, raw)
    return res


def _check_constant_units(res, c, ref, raw):
    """The dead ReLU unit and the constant unit: every row of a slot equals its pivot, so the fp32 sums relative to the pivot are exactly
    0 and the slot holds S = n v, Q = n v^2 for ONE fp32 number v, formed in fp64 (2^-50: the roundings of those products)."""
    for b, k, lo, hi in R.slot_rows(c, ref.out_len):
        n = hi - lo
        for u in (DEAD_UNIT, CONST_UNIT):
            S, Q = raw[b, k, 0, u], raw[b, k, 1, u]
            v = S / n
            res.true(f"constant unit {u}, utterance {b} slot {k}: S = n v for an fp32 v", np.float64(np.float32(v)) == v)
            res.true(f"constant unit {u}, utterance {b} slot {k}: Q = n v^2", abs(Q - n * v * v) <= 2.0 ** -50 * n * v * v)
