"""What lies behind the TDNN stack, restated in fp64 NumPy with exact sums where they cancel: the statistics pooling
(ktf_stats_pool, ktf_stats_pool_windowed_f32), the finalize of the fused pooling's fp64 sums (ktf_stats_finalize{,_slots,_flat}), the
x-vector post-processing (ktf_xvec_post_f32) and the fused tail (ktf_xvec_tail_f32). Every function returns the expected values and,
per element, a bound on what a correct kernel may deviate; below them the tables of cases test_gpu_pool_post.py runs and
test_pool_ref_cpu.py checks on the CPU, each with the kernel instance or path the launcher's rule -- restated here -- picks for it.

U = 2^-24 is the unit roundoff of fp32, E = 2^-53 that of fp64.

Pooling and finalize. The kernels sum in fp64 and round once, so
    mean   |got - ref| <= U |mean| + (n + 2) E mean|x|
    std    |got - ref| <= U std + (n + 4) E (E[x^2] + mean^2) / (2 std)
(n terms: the sums, one division, the product and the difference; the second term of the std bound is the cancellation of
E[x^2] - mean^2 in fp64, passed through the concave square root: sqrt(v + d) - sqrt(v) <= d / (2 sqrt(v))). The finalize adds
`used` slot sums instead of n rows: `used` takes the place of n and sum |s_k| / n that of mean|x|.

Post and tail, in the (terms + 2) U sum |a_i b_i| convention of test_gpu_tdnn_grad.py, to first order through the three steps
    h = W x + b            e_h = (in_dim + 2) U (|W| |x| + |b|)  [+ |W| e_x when x itself is only known to e_x]
    t = (h - m) A + off    e_t = (e_h + U |h - m|) |A| + (units + 2) U (|h - m| |A| + |off|)
    y = t sqrt(od) / |t|   e_y = sqrt(od) (e_t / |t| + |t_c| sum |t| e_t / |t|^3) + 4 U |y|
For the post-processing alone the first step is x - mean with error U |x - mean|, and in_dim takes the place of units."""

import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
E = 2.0 ** -53
NAN = float("nan")


def cdiv(a, b):
    return -(-a // b)


def to_bf16(a):
    """fp32 values rounded to the nearest bf16 (ties to even), still as float32: what a bf16 buffer holds, exactly."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(a))


# ----------------------------------------------------------------------------- pooling
def _moments(rows, exact=True):
    """rows (n, C) fp64, n >= 1 -> (mean, var, mean|x|) per column. The sum is math.fsum (correctly rounded); the variance is taken
    about that mean, mean(d^2) - mean(d)^2 with d = x - mean, so that nothing of the size of mean^2 cancels: its error is a few E
    of the variance itself. exact=False: the same with NumPy's pairwise fp64 sums about the first row (n E of the variance), for
    tables too large for a Python loop per column."""
    n = rows.shape[0]
    if exact:
        mean = np.array([math.fsum(c) for c in rows.T.tolist()]) / n
    else:
        mean = rows[0] + (rows - rows[0]).sum(0) / n
    d = rows - mean
    if exact:
        m1 = np.array([math.fsum(c) for c in d.T.tolist()]) / n
        m2 = np.array([math.fsum(c) for c in (d * d).T.tolist()]) / n
    else:
        m1, m2 = d.sum(0) / n, (d * d).sum(0) / n
    return mean, np.maximum(m2 - m1 * m1, 0.0), np.abs(rows).mean(0)


def _stat_row(rows, include_std, eps, exact=True):
    """-> (values, bounds) of one pooled row (D or 2 D) from its sampled rows (n, D); NaN where there is none."""
    n, D = rows.shape
    od = 2 * D if include_std else D
    if n == 0:
        return np.full(od, NAN), np.zeros(od)
    mean, var, absmean = _moments(rows.astype(np.float64), exact)
    e_mean = U * np.abs(mean) + (n + 2) * E * absmean
    if not include_std:
        return mean, e_mean
    std = np.sqrt(var + float(np.float32(eps)))             # (the library takes eps as a float)
    with np.errstate(divide="ignore", invalid="ignore"):       # (std == 0: eps == 0 and a constant column, exact in the kernel too)
        e_std = np.where(std > 0, U * std + (n + 4) * E * (var + 2 * mean * mean) / (2 * std), 0.0)
    return np.concatenate([mean, std]), np.concatenate([e_mean, e_std])


def clamp_len(n, T):
    return T if n is None else max(0, min(int(n), T))


def pool(x, lens=None, period=1, include_std=True, eps=1e-10, exact=True):
    """x (B, T, D) fp32 (a bf16 input already converted, exactly) -> (want, bound), both (B, D or 2 D) fp64: the statistics over
    rows 0, period, 2 period, .. below min(len, T)."""
    x = np.asarray(x)
    B, T, D = x.shape
    out = [_stat_row(x[b, 0:clamp_len(None if lens is None else lens[b], T):period], include_std, eps, exact) for b in range(B)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def window_steps(T, left, right, output_period, padding):
    """(start, T_out) of the windowed pooling's output rows, layers/stats/stats_pooling.py:186-215 of the reference as
    oracle/ktf_oracle.py restates it."""
    start, end = 0, T
    if padding.upper() != "SAME":
        if left < 0:
            start = -left
        if right > 0 and (right - left + 1) < T:
            end = T - right
        end += 1
    return start, len(range(start, end, output_period))


def pool_windowed(x, left, right, input_period, output_period, start, T_out, include_std=True, eps=1e-10, exact=True):
    """x (B, T, D) -> (want, bound) (B, T_out, D or 2 D): output row j pools the frames start + j output_period + o inside [0, T),
    o = left, left + input_period, .. < min(right + 1, T)."""
    x = np.asarray(x)
    B, T, D = x.shape
    od = 2 * D if include_std else D
    want, bound = np.zeros((B, T_out, od)), np.zeros((B, T_out, od))
    offs = range(left, min(right + 1, T), input_period)
    for j in range(T_out):
        ts = [start + j * output_period + o for o in offs]
        ts = [t for t in ts if 0 <= t < T]
        for b in range(B):
            want[b, j], bound[b, j] = _stat_row(x[b, ts], include_std, eps, exact)
    return want, bound


# ----------------------------------------------------------------------------- finalize
def slot_sums(x, lens, slots, slot_rows):
    """The fp64 sums the fused pooling leaves: (B, 2, D) [slots == 0] or (B, slots, 2, D), slot k = rows [k slot_rows, (k + 1)
    slot_rows) below len; slots without a row are NaN. -> (sums, used)."""
    x = np.asarray(x, dtype=np.float64)
    B, T, D = x.shape
    S = max(slots, 1)
    rows = slot_rows if slots else max(T, 1)
    sums = np.full((B, S, 2, D), NAN)
    used = []
    for b in range(B):
        n = clamp_len(lens[b], T)
        used.append(cdiv(n, rows) if slots else 1)
        if not slots:
            sums[b, 0] = 0.0
        for k in range(cdiv(n, rows)):
            seg = x[b, k * rows:min((k + 1) * rows, n)]
            sums[b, k, 0], sums[b, k, 1] = seg.sum(0), (seg * seg).sum(0)
    return (sums if slots else sums[:, 0]), used


def flat_sums(x, lens, slots):
    """The same on flat row tiles: the utterances' valid rows laid end to end, slot k of an utterance = its rows inside the k-th
    128-row block of the flat row space that it touches. -> (sums (B, slots, 2, D), used, row_starts (B + 1,))."""
    x = np.asarray(x, dtype=np.float64)
    B, T, D = x.shape
    starts = np.concatenate([[0], np.cumsum([clamp_len(n, T) for n in lens])]).astype(np.int64)
    sums = np.full((B, slots, 2, D), NAN)
    used = []
    for b in range(B):
        s, n = int(starts[b]), int(starts[b + 1] - starts[b])
        first, last = s >> 7, (s + n - 1) >> 7
        used.append(last - first + 1 if n > 0 else 0)
        for k in range(used[-1]):
            lo, hi = max(s, (first + k) * 128), min(s + n, (first + k + 1) * 128)
            seg = x[b, lo - s:hi - s]
            sums[b, k, 0], sums[b, k, 1] = seg.sum(0), (seg * seg).sum(0)
    return sums, used, starts


def finalize(sums, lens, used, include_std=True, eps=1e-10):
    """sums (B, S, 2, D) fp64 (or (B, 2, D)), lens[b] rows and used[b] slots per utterance -> (want, bound) (B, D or 2 D), in exact
    rational arithmetic on the fp64 sums."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums.ndim == 3:
        sums = sums[:, None]
    B, _, _, D = sums.shape
    od = 2 * D if include_std else D
    want, bound = np.full((B, od), NAN), np.zeros((B, od))
    eps = Fraction(float(np.float32(eps)))
    for b in range(B):
        n, k = int(lens[b]), int(used[b])
        if n <= 0:
            continue
        for c in range(D):
            s, q = (sum((Fraction(v) for v in sums[b, :k, i, c]), Fraction(0)) for i in (0, 1))
            mean = s / n
            want[b, c] = float(mean)
            bound[b, c] = U * abs(want[b, c]) + (k + 2) * E * float(np.abs(sums[b, :k, 0, c]).sum()) / n
            if include_std:
                var = max(q / n - mean * mean, Fraction(0))
                std = math.sqrt(float(var + eps))
                want[b, D + c] = std
                bound[b, D + c] = U * std + (k + 4) * E * float(q / n + mean * mean) / (2 * std) if std > 0 else 0.0
    return want, bound


# ----------------------------------------------------------------------------- post and tail
def _length_norm(t, e_t):
    od = t.shape[-1]
    nrm = np.sqrt((t * t).sum(-1, keepdims=True))
    y = t * math.sqrt(od) / nrm
    e_y = math.sqrt(od) * (e_t / nrm + np.abs(t) * (np.abs(t) * e_t).sum(-1, keepdims=True) / nrm ** 3) + 4 * U * np.abs(y)
    return y, e_y


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def post(x, mean, A, off):
    """x (B, in_dim), A (in_dim, out_dim) -> dict t, e_t, y, e_y (B, out_dim)."""
    x, mean, A, off = _f64(x), _f64(mean), _f64(A), _f64(off)
    in_dim = A.shape[0]
    d = x if mean is None else x - mean
    e_d = np.zeros_like(d) if mean is None else U * np.abs(d)
    o = np.zeros(A.shape[1]) if off is None else off
    t = d @ A + o
    e_t = e_d @ np.abs(A) + (in_dim + 2) * U * (np.abs(d) @ np.abs(A) + np.abs(o))
    y, e_y = _length_norm(t, e_t)
    return dict(t=t, e_t=e_t, y=y, e_y=e_y)


def tail(x, W, bias, mean, A, off, e_x=None):
    """x (B, in_dim) the pooled rows, W (units, in_dim), A (units, out_dim) -> dict h, e_h (B, units), y, e_y (B, out_dim). A row of
    x with a NaN (an utterance without a frame) is a NaN row of both."""
    x, W, bias, mean, A, off = _f64(x), _f64(W), _f64(bias), _f64(mean), _f64(A), _f64(off)
    units, in_dim = W.shape
    b = np.zeros(units) if bias is None else bias
    o = np.zeros(A.shape[1]) if off is None else off
    h = x @ W.T + b
    e_h = (in_dim + 2) * U * (np.abs(x) @ np.abs(W).T + np.abs(b))
    if e_x is not None:
        e_h = e_h + e_x @ np.abs(W).T
    d = h if mean is None else h - mean
    t = d @ A + o
    e_t = (e_h + U * np.abs(d)) @ np.abs(A) + (units + 2) * U * (np.abs(d) @ np.abs(A) + np.abs(o))
    with np.errstate(invalid="ignore"):
        y, e_y = _length_norm(t, e_t)
    return dict(h=h, e_h=e_h, y=y, e_y=e_y)


EXACT_Y = 4 * U * (1 + 4 * U)       # exact t and sum t^2: two square roots and two divisions, each rounded once, (1 + U)^2 / (1 - U)^2 - 1


def ratio(got, want, bound):
    """max |got - want| / bound over the elements, compared in float64; where `want` is NaN, `got` must be NaN and nothing else
    may be; a zero bound asks for equality. inf where any of that fails."""
    got, want, bound = np.asarray(got).astype(np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    nan = np.isnan(want)
    if (np.isnan(got) != nan).any():
        return float("inf")
    err = np.abs(got - want)[~nan]
    bound = np.broadcast_to(bound, want.shape)[~nan]
    if (err[bound == 0] != 0).any():
        return float("inf")
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


# ----------------------------------------------------------------------------- data
BIG = 32768.0


def columns(rng, shape, first=1):
    """(.., D) fp32: column c is of kind (c + first) mod 5 -- 0: N(0, 1) (pool_data() puts +BIG and -BIG into two of its rows),
    1: 1000 + N(0, 1), 2: 3 + 1e-4 N(0, 1) (E[x^2] - mean^2 cancels six and nine digits), 3: N(0, 1), 4: the constant 1.5."""
    x = rng.standard_normal(shape)
    c = (np.arange(shape[-1]) + first) % 5
    x = np.where(c == 1, 1000.0 + x, np.where(c == 2, 3.0 + 1e-4 * x, np.where(c == 4, 1.5, x)))
    return x.astype(np.float32)


# ----------------------------------------------------------------------------- cases: ktf_stats_pool
POOL_T = 70
POOL_DS = (1, 2, 23, 32, 33, 130)
POOL_LENS = (None, 0, 1, 63, 64, 65, POOL_T, POOL_T + 5, -1)
_LENS3 = (None, (0, 1, 63), (64, 65, POOL_T), (POOL_T + 5, -1, 63))


def pool_instance(B, D, ldx, offset, itemsize):
    """(narrow, vec) as ktf_stats_pool picks them: 32-column workgroups while cdiv(D, 128) * B < 256; 8-byte pair loads when ldx
    is even and the base (`offset` elements into an allocation) is 8-byte aligned."""
    return cdiv(D, 128) * B < 256, ldx % 2 == 0 and (offset * itemsize) % 8 == 0


def _pool_cases():
    cases, k = {}, 0

    def add(tag, B, D, dtype, ldx, offset, lens):
        nonlocal k
        narrow, vec = pool_instance(B, D, ldx, offset, 4 if dtype == "f32" else 2)
        c = dict(name=f"{tag}_{dtype}_B{B}_D{D}_ld{ldx}_o{offset}", B=B, T=POOL_T, D=D, dtype=dtype, ldx=ldx, offset=offset, lens=lens,
                 period=(1, 3)[k % 2], include_std=k % 3 != 2, ld_out_extra=(0, 3)[(k // 2) % 2], narrow=narrow, vec=vec, seed=1000 + k)
        cases[c["name"]] = c
        k += 1

    def ragged(B):
        """Every length of POOL_LENS but None, in an order that does not repeat with the workgroup index."""
        return tuple(POOL_LENS[1:][(b * 7 + b // 8) % 8] for b in range(B))

    for dtype in ("f32", "bf16"):
        for i, D in enumerate(POOL_DS):
            even = D + D % 2
            pad = 2 if D % 2 == 0 and (i // 2 + (dtype == "bf16")) % 2 else 0
            add("n", 3, D, dtype, even + pad, 0, _LENS3[k % 4])                                    # pairs: ldx = D even, D + 2, or D + 1
            add("n", 3, D, dtype, D if D % 2 else D + 1, 0, _LENS3[k % 4])                         # scalar: odd ldx
            add("n", 3, D, dtype, even + 2, 1, _LENS3[k % 4])                                      # scalar: even ldx, base one element off
        for B, D in ((256, 33), (128, 130)):
            add("w", B, D, dtype, D + D % 2, 0, ragged(B))
            add("w", B, D, dtype, D + 1 - D % 2, 0, ragged(B))
    for B, D, ldx, off in ((256, 1, 2, 0), (256, 2, 4, 1), (256, 32, 32, 0), (256, 23, 23, 0)):
        add("w", B, D, "f32", ldx, off, None if D == 32 else ragged(B))
    return cases


POOL_CASES = _pool_cases()


def pool_data(c):
    """-> x (B, T, D) fp32 (bf16 cases: values a bf16 holds), lens as a list or None. Columns 0, 5, .. hold +BIG in the first and
    -BIG in the last sampled row of every utterance with two or more: their mean is that of the rows between, which a sum carried
    in fp32 loses to the rounding at BIG."""
    x = columns(np.random.default_rng(c["seed"]), (c["B"], c["T"], c["D"]), first=0)
    for b in range(c["B"]):
        n = len(range(0, clamp_len(None if c["lens"] is None else c["lens"][b], c["T"]), c["period"]))
        if n >= 2:
            x[b, 0, 0::5], x[b, (n - 1) * c["period"], 0::5] = BIG, -BIG
    return (to_bf16(x) if c["dtype"] == "bf16" else x), (None if c["lens"] is None else list(c["lens"]))


# ----------------------------------------------------------------------------- cases: ktf_stats_pool_windowed_f32
WINDOWS = ((0, 0), (-3, 6), (-4, 5))
GRID_CAP = 4096 * 256


def _windowed_cases():
    cases, k = {}, 0
    for left, right in WINDOWS:
        for T in sorted({1, 2, right, right + 1, 61} - {0}):
            for padding in ("SAME", "VALID"):
                if padding == "VALID" and T <= right - left + 1:
                    continue                                    # (the layer pools all frames there: ktf_stats_pool)
                ip = 3 if (left, right) == (-4, 5) or k % 4 == 3 else 1          # (the reference wants output_period a multiple of it)
                c = dict(name=f"win_{-left}_{right}_T{T}_{padding}", B=2, T=T, D=(1, 23)[k % 2], left=left, right=right, input_period=ip,
                         output_period=3 if ip == 3 else (1, 3)[(k // 2) % 2], padding=padding, include_std=True, exact=True, seed=2000 + k)
                cases[c["name"]] = c
                k += 1
    cases["win_above_the_grid_cap"] = dict(name="win_above_the_grid_cap", B=2, T=2100, D=256, left=-1, right=1, input_period=1,
                                           output_period=1, padding="SAME", include_std=True, exact=False, seed=2999)
    return cases


WINDOWED_CASES = _windowed_cases()


def windowed_data(c):
    rng = np.random.default_rng(c["seed"])
    shape = (c["B"], c["T"], c["D"])
    return columns(rng, shape) if c["exact"] else rng.standard_normal(shape).astype(np.float32)


# ----------------------------------------------------------------------------- cases: ktf_stats_finalize{,_slots,_flat}
FIN_T = 300
FIN_LENS = (300, 0, 1, 129, 64, 200)


def _finalize_cases():
    cases, k = {}, 0
    for form, slot_rows in (("sums", 0), ("slots", 64), ("slots", 128), ("flat", 128)):
        for D in (1, 33):
            c = dict(name=f"fin_{form}{slot_rows or ''}_D{D}", form=form, slot_rows=slot_rows, B=len(FIN_LENS), T=FIN_T, D=D, lens=FIN_LENS,
                     include_std=k % 3 != 1, ld_out_extra=(0, 5)[k % 2], seed=3000 + k)
            cases[c["name"]] = c
            k += 1
    return cases


FINALIZE_CASES = _finalize_cases()


def finalize_data(c, flat_slots=None):
    """-> dict x, sums, used, lens (the rows per utterance), slots, starts (flat form). `flat_slots`: ktf_flat_stats_slots(T), which
    the GPU test asks the library for; the default restates it."""
    x = columns(np.random.default_rng(c["seed"]), (c["B"], c["T"], c["D"]))
    lens = [clamp_len(n, c["T"]) for n in c["lens"]]
    if c["form"] == "flat":
        slots = flat_slots or (c["T"] + 254) // 128
        sums, used, starts = flat_sums(x, lens, slots)
        return dict(x=x, sums=sums, used=used, lens=lens, slots=slots, starts=starts)
    slots = cdiv(c["T"], c["slot_rows"]) + 1 if c["slot_rows"] else 0          # (one more than any utterance uses: always a poisoned one)
    sums, used = slot_sums(x, lens, slots, c["slot_rows"] or 128)
    return dict(x=x, sums=sums, used=used, lens=lens, slots=slots, starts=None)


# ----------------------------------------------------------------------------- cases: ktf_xvec_post_f32
POST_LDS_FLOATS = 1024 + 16


def post_eb(B, in_dim, out_dim):
    """Embeddings per workgroup: four beyond one round of the chip (B > 256) if their rows fit 64 KiB of LDS."""
    return 4 if B > 256 and 4 * 4 * (in_dim + out_dim + POST_LDS_FLOATS) <= 64 * 1024 else 1


def post_fits(in_dim, out_dim):
    return 4 * (in_dim + out_dim + POST_LDS_FLOATS) <= 64 * 1024


def _post_cases():
    cases = {}
    for k, (B, in_dim, out_dim, mean, off, regime) in enumerate((
            (1, 1, 1, True, True, "gauss"), (1, 3, 64, True, True, "gauss"), (1, 23, 65, True, False, "gauss"), (1, 512, 150, True, True, "gauss"),
            (1, 23, 1000, False, True, "gauss"), (1, 3, 1025, True, True, "gauss"), (1, 512, 1025, True, True, "gauss"),
            (257, 23, 65, True, True, "gauss"), (258, 1, 64, False, False, "gauss"), (259, 3, 150, True, True, "gauss"),
            (257, 512, 150, True, True, "gauss"), (257, 512, 2600, True, True, "gauss"), (259, 23, 150, True, True, "int"),
            (1, 512, 1025, True, True, "int"))):
        c = dict(name=f"post_{regime}_B{B}_{in_dim}_{out_dim}{'' if mean else '_nomean'}{'' if off else '_nooff'}", B=B, in_dim=in_dim,
                 out_dim=out_dim, mean=mean, off=off, regime=regime, eb=post_eb(B, in_dim, out_dim), seed=4000 + k)
        cases[c["name"]] = c
    return cases


POST_CASES = _post_cases()


def _sparse_ints(rng, rows, cols, per_col):
    """(rows, cols) of -1 / 0 / +1 with at most `per_col` non-zeros in each column and at least one in each row when
    cols * per_col >= rows: row r sits in column r mod cols."""
    M = np.zeros((rows, cols), dtype=np.float32)
    for j in range(per_col):
        r = np.arange(j * cols, min((j + 1) * cols, rows))
        M[r, r % cols] = rng.choice([-1.0, 1.0], len(r))
    return M


def post_data(c):
    """-> x (B, in_dim), mean, A (in_dim, out_dim), off, fp32 (mean / off None as the case says). Integer regime: every product and
    every partial sum in any order is an integer below 2^24, and so is sum t^2."""
    rng = np.random.default_rng(c["seed"])
    B, I, O = c["B"], c["in_dim"], c["out_dim"]
    if c["regime"] == "int":
        x = rng.integers(-3, 4, (B, I)).astype(np.float32)
        mean = rng.integers(-2, 3, I).astype(np.float32)
        A = _sparse_ints(rng, I, O, cdiv(I, O) + 1)
        A[rng.integers(0, I, 4 * O), rng.integers(0, O, 4 * O)] = 1.0
        off = rng.integers(-2, 3, O).astype(np.float32)
        worst = (np.abs(x).max(0) + np.abs(mean)) @ np.abs(A) + np.abs(off)
        assert (worst * worst).sum() < 2 ** 24
    else:
        x = rng.standard_normal((B, I)).astype(np.float32)
        mean = (0.5 * rng.standard_normal(I)).astype(np.float32)
        A = (rng.standard_normal((I, O)) / math.sqrt(I)).astype(np.float32)
        off = (0.3 * rng.standard_normal(O)).astype(np.float32)
        if O == 1:          # y = +-1 whatever t is: an offset of the other sign than the product, so that a lost input shows
            off = (-0.25 * ((x[0] - mean) @ A)).astype(np.float32)
    return x, (mean if c["mean"] else None), A, (off if c["off"] else None)


# ----------------------------------------------------------------------------- cases: ktf_xvec_tail_f32
TAIL_T = 150            # rows of the utterances behind the sums sources
TAIL_SOURCES = ("pooled", "pooled_ld5", "sums", "slots64", "slots128")


def _tail_cases():
    cases = {}

    def add(name, D, std, units, out_dim, source, B, group, regime="gauss", lens=None, skip_empty=False, ldw_extra=4, **none):
        in_dim = (2 if std else 1) * D
        if lens is None and source not in ("pooled", "pooled_ld5"):
            lens = tuple((TAIL_T, 1, 77, 128, 129, 64, 65)[b % 7] for b in range(B))
        c = dict(name=name, D=D, include_std=std, in_dim=in_dim, units=units, out_dim=out_dim, source=source, B=B, group=group, regime=regime,
                 lens=lens, skip_empty=skip_empty, ldw_extra=ldw_extra, two_phase=group > 1, seed=5000 + len(cases),
                 bias=none.get("bias", True), mean=none.get("mean", True), off=none.get("off", True), h_out=none.get("h_out", True))
        cases[name] = c

    add("t2_u1_o1_pooled", 1, True, 1, 1, "pooled", 1, 1)
    add("t2_u7_o33_sums", 2, False, 7, 33, "sums", 5, 1, ldw_extra=0)
    add("t6_u63_o33_ld5_g2", 3, True, 63, 33, "pooled_ld5", 5, 2)
    add("t70_u65_o33_slots64", 35, True, 65, 33, "slots64", 5, 1)
    add("t70_u64_o150_slots128_g2", 70, False, 64, 150, "slots128", 5, 2, ldw_extra=8)
    add("t301_u130_o150_pooled", 301, False, 130, 150, "pooled", 5, 1, ldw_extra=8)
    add("t301_u130_o256_ld5_g32", 301, False, 130, 256, "pooled_ld5", 37, 32)
    add("t70_u65_o33_pooled_g1024", 35, True, 65, 33, "pooled", 1030, 1024)
    add("t70_u65_o33_sums_g32", 35, True, 65, 33, "sums", 37, 32)
    for what in ("bias", "mean", "off", "h_out"):
        add(f"t70_u65_o33_no_{what}", 35, True, 65, 33, "pooled", 5, (1, 2)[what in ("mean", "h_out")], **{what: False})
    # lens holding zeros: without skip_empty an empty utterance is a NaN row on the sums path ...
    add("t70_u65_o33_slots128_empty_nan", 35, True, 65, 33, "slots128", 5, 1, lens=(TAIL_T, 0, 77, 0, 1))
    add("t70_u65_o33_sums_empty_nan_g2", 35, True, 65, 33, "sums", 5, 2, lens=(0, 40, 0, 0, 9))
    # ... and with it: a whole group empty (b 0, 1), a mixed group (b 2, 3), a single empty utterance in a group of its own
    add("t70_u65_o33_slots64_skip_g2", 35, True, 65, 33, "slots64", 7, 2, lens=(0, 0, 70, 0, 33, 5, 0), skip_empty=True)
    add("t70_u65_o33_pooled_skip_g1", 35, True, 65, 33, "pooled", 5, 1, lens=(9, 0, 5, 1, 0), skip_empty=True)
    add("t70_u65_o33_sums_skip_g32", 35, True, 65, 33, "sums", 37, 32, lens=tuple((0, 12, 0, 0, 150)[b % 5] if b < 32 else 0 for b in range(37)),
        skip_empty=True)
    # the limits, on integer data
    add("t3072_u512_o150_pooled_int", 1536, True, 512, 150, "pooled", 5, 1, regime="int")
    add("t3072_u512_o256_slots128_int_g2", 1536, True, 512, 256, "slots128", 3, 2, regime="int")
    add("t2_u512_o1_sums_int", 1, True, 512, 1, "sums", 5, 1, regime="int")
    add("t3072_u1_o33_ld5_int", 1536, True, 1, 33, "pooled_ld5", 2, 1, regime="int")
    add("t6_u7_o33_slots64_int_g2", 3, True, 7, 33, "slots64", 5, 2, regime="int")
    return cases


TAIL_CASES = _tail_cases()


def tail_data(c):
    """-> dict W (units, in_dim), bias, mean, A (units, out_dim), off (None as the case says), eps, and the source: `pooled` (B,
    in_dim) fp32, or `sums` / `used` / `slots` / `slot_rows` / `lens` with `pooled` = what their finalize gives (fp64) and `e_pooled`
    its bound. Integer regime: pooled rows of small integers (the sums are made for them: s = n m, q = n (m^2 + d^2), eps = 0), W
    and A of -1 / 0 / +1 with every column of W used, so that every product and partial sum, in any order, and sum t^2 are exact."""
    rng = np.random.default_rng(c["seed"])
    B, D, I, Un, O = c["B"], c["D"], c["in_dim"], c["units"], c["out_dim"]
    integer = c["regime"] == "int"
    d = dict(eps=0.0 if integer else 1e-10)
    if integer:
        W = _sparse_ints(rng, I, Un, cdiv(I, Un)).T.copy()              # every input column in exactly one unit
        bias = rng.integers(-2, 3, Un).astype(np.float32)
        mean = rng.integers(-2, 3, Un).astype(np.float32)
        A = _sparse_ints(rng, Un, O, min(cdiv(Un, O), 8))
        off = rng.integers(-2, 3, O).astype(np.float32)
    else:
        W = (rng.standard_normal((Un, I)) / math.sqrt(I)).astype(np.float32)
        bias = (0.3 * rng.standard_normal(Un)).astype(np.float32)
        mean = (0.3 * rng.standard_normal(Un)).astype(np.float32)
        A = (rng.standard_normal((Un, O)) / math.sqrt(Un)).astype(np.float32)
        off = (0.3 * rng.standard_normal(O)).astype(np.float32)
    d.update(W=W, bias=bias if c["bias"] else None, mean=mean if c["mean"] else None, A=A, off=off if c["off"] else None)
    lens = None if c["lens"] is None else list(c["lens"])
    d["lens"] = lens
    if c["source"] in ("pooled", "pooled_ld5"):
        if integer:
            pooled = rng.choice([-1.0, 1.0] if Un == 1 else [-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], (B, I)).astype(np.float32)
        else:
            pooled = np.concatenate([rng.standard_normal((B, D)), np.abs(rng.standard_normal((B, I - D))) + 0.1], 1).astype(np.float32)
        d.update(pooled=pooled, e_pooled=None)
    else:
        slot_rows = {"sums": 0, "slots64": 64, "slots128": 128}[c["source"]]
        slots = cdiv(TAIL_T, slot_rows) + 1 if slot_rows else 0
        n = [clamp_len(v, TAIL_T) for v in lens]
        if integer:
            m = rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], (B, D))
            sd = rng.integers(1, 4, (B, D)).astype(np.float64) if c["include_std"] else np.zeros((B, D))
            sums = np.full((B, max(slots, 1), 2, D), NAN)
            used = []
            for b in range(B):
                k = cdiv(n[b], slot_rows) if slots else 1
                used.append(k)
                rows = [min(slot_rows, n[b] - j * slot_rows) for j in range(k)] if slots else [n[b]]
                for j, r in enumerate(rows):
                    sums[b, j, 0], sums[b, j, 1] = r * m[b], r * (m[b] * m[b] + sd[b] * sd[b])
            sums = sums if slots else sums[:, 0]
        else:
            sums, used = slot_sums(columns(rng, (B, TAIL_T, D)), n, slots, slot_rows or 128)
        want, bound = finalize(sums, n, used, c["include_std"], d["eps"])
        d.update(sums=sums, used=used, slots=slots, slot_rows=slot_rows or 128, lens=n, pooled=want, e_pooled=bound)
    if integer:
        p = np.nan_to_num(np.asarray(d["pooled"], dtype=np.float64))
        h_max = np.abs(p).max(0) @ np.abs(W).T.astype(np.float64) + np.abs(bias)
        t_max = (h_max + np.abs(mean)) @ np.abs(A).astype(np.float64) + np.abs(off)
        assert h_max.max() < 2 ** 24 and (t_max * t_max).sum() < 2 ** 24, (c["name"], h_max.max(), (t_max * t_max).sum())
    return d


def tail_reference(c, d):
    """-> tail() of the case's data; on a sums source the pooled row the kernel builds is its own fp64 finalize rounded to fp32,
    within twice the finalize bound of the exact one rounded."""
    pooled = np.asarray(d["pooled"], dtype=np.float64).astype(np.float32)
    e_x = None if d["e_pooled"] is None or c["regime"] == "int" else 2 * d["e_pooled"]
    with np.errstate(invalid="ignore"):
        return tail(pooled, d["W"], d["bias"], d["mean"], d["A"], d["off"], e_x=e_x)
