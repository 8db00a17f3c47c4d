"""fp64 NumPy oracle of the gradients declared in include/ktf_grad.h, written as plain loops over (utterance, output row, context)
with the clamp, and the cases the CPU and the GPU tests share. For every element of a TDNN gradient it also returns the number of
terms n and S = the sum of the terms' magnitudes: |fp32 result - this| <= (n + 2) 2^-24 S is the a-priori bound of an fp32 dot
product summed in any order plus one final rounding."""

import itertools

import numpy as np

CONTEXTS = ([0], [-1, 2], [-3, 0, 3], [-2, -1, 0, 1, 2])
DIMS = list(itertools.product((23, 30, 64), (40, 130, 256)))           # (din, units)
# lengths: empty, one row, shorter than every multi-offset context's span, the weight kernel's 16-row step and the data kernel's 64-row
# tile -1 / exactly / +1, the weight kernel's 128-row tile around 129 / 130, and some in between
LENS = (0, 1, 3, 15, 16, 17, 63, 64, 65, 130, 97, 129, 33, 2)
T = max(LENS)


def out_len(n, context, sub, valid):
    """-> (rows of output, first input row) of an utterance of n rows."""
    start, end = 0, n
    if valid:
        start = -min(context[0], 0)
        end = n - max(context[-1], 0)
    m = end - start
    return (0 if m <= 0 else (m + sub - 1) // sub), start


def cases():
    """Every context x padding x subsampling (16), the (din, units) pairs dealt round: each of the 9 pairs occurs."""
    out = []
    for i, (ctx, padding, sub) in enumerate(itertools.product(CONTEXTS, ("SAME", "VALID"), (1, 3))):
        din, units = DIMS[i % len(DIMS)]
        out.append(dict(context=list(ctx), padding=padding, sub=sub, din=din, units=units))
    return out


def case_id(c):
    return f"ctx{'_'.join(str(v) for v in c['context'])}-{c['padding']}-sub{c['sub']}-{c['din']}x{c['units']}"


def lens_for(c, slot_rows):
    """LENS rotated so that the valid output rows of some utterance lie on both sides of a multiple of `slot_rows` in the flat row
    space b * T_out + t (an utterance whose rows two partial sums of the weight gradient share)."""
    valid = c["padding"] == "VALID"
    Tout = out_len(T, c["context"], c["sub"], valid)[0]
    for rot in range(len(LENS)):
        lens = LENS[rot:] + LENS[:rot]
        for b, n in enumerate(lens):
            ol = out_len(n, c["context"], c["sub"], valid)[0]
            if ol > 1 and (b * Tout) // slot_rows != (b * Tout + ol - 1) // slot_rows:
                return list(lens)
    raise AssertionError(f"no rotation of LENS straddles a slot of {slot_rows} rows for {case_id(c)}")


def tdnn_grads(x, W, g, lens, context, sub=1, padding="SAME"):
    """x (B, T, D), W (units, nctx, D), g (B, T_out, units), lens (B,) -> dict of fp64 arrays dx (B, T, D), dW (units, nctx, D),
    db (units,), each with its term count `*_n` and magnitude sum `*_S`. Rows of x / g beyond an utterance's lengths are not read."""
    x, W, g = (np.asarray(a, np.float64) for a in (x, W, g))
    B, Tm, D = x.shape
    units, nctx, _ = W.shape
    valid = padding.upper() == "VALID"
    aW = np.abs(W)
    r = {k: np.zeros(s) for k, s in (("dx", x.shape), ("dW", W.shape), ("db", (units,)))}
    r.update({k + suffix: np.zeros_like(r[k]) for k in ("dx", "dW", "db") for suffix in ("_n", "_S")})
    for b in range(B):
        n = int(lens[b])
        ol, start = out_len(n, context, sub, valid)
        for t in range(ol):
            gt = g[b, t]
            agt = np.abs(gt)
            r["db"] += gt
            r["db_S"] += agt
            r["db_n"] += 1
            for k in range(nctx):
                row = min(max(start + t * sub + context[k], 0), n - 1)
                r["dx"][b, row] += gt @ W[:, k, :]
                r["dx_S"][b, row] += agt @ aW[:, k, :]
                r["dx_n"][b, row] += units
                r["dW"][:, k, :] += np.outer(gt, x[b, row])
                r["dW_S"][:, k, :] += np.outer(agt, np.abs(x[b, row]))
                r["dW_n"][:, k, :] += 1
    return r


def tdnn_forward(x, W, bias, lens, context, sub=1, padding="SAME"):
    """z (B, T_out, units) fp64 by the same loops; rows at and beyond an utterance's output length are zero."""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    B, Tm, D = x.shape
    valid = padding.upper() == "VALID"
    z = np.zeros((B, out_len(Tm, context, sub, valid)[0], W.shape[0]))
    for b in range(B):
        n = int(lens[b])
        ol, start = out_len(n, context, sub, valid)
        for t in range(ol):
            if bias is not None:
                z[b, t] += bias
            for k in range(len(context)):
                z[b, t] += W[:, k, :] @ x[b, min(max(start + t * sub + context[k], 0), n - 1)]
    return z


def pool_forward(x, lens, include_std=True, eps=1e-10, period=1):
    x = np.asarray(x, np.float64)
    B, Tm, D = x.shape
    out = np.full((B, 2 * D if include_std else D), np.nan)
    for b in range(B):
        rows = x[b, 0:int(lens[b]):period]
        if len(rows) == 0:
            continue
        mean = rows.sum(0) / len(rows)
        out[b, :D] = mean
        if include_std:
            out[b, D:] = np.sqrt(np.maximum((rows * rows).sum(0) / len(rows) - mean * mean, 0.0) + eps)
    return out


def pool_grad(x, lens, gout, include_std=True, eps=1e-10, period=1):
    """-> (dx (B, T, D) fp64, M (B, T, D) = |gm| / n + |gs| |x - mean| / (n std), the magnitudes of dx's two terms)."""
    x, gout = np.asarray(x, np.float64), np.asarray(gout, np.float64)
    B, Tm, D = x.shape
    dx, M = np.zeros(x.shape), np.zeros(x.shape)
    for b in range(B):
        n = len(range(0, int(lens[b]), period))
        if n == 0:
            continue
        rows = x[b, 0:int(lens[b]):period]
        mean = rows.sum(0) / n
        var = (rows * rows).sum(0) / n - mean * mean
        gm = gout[b, :D]
        d = np.broadcast_to(gm / n, rows.shape).copy()
        m = np.broadcast_to(np.abs(gm) / n, rows.shape).copy()
        if include_std:
            live = var > 0.0                                      # the relu clipped elsewhere: no second term
            coef = np.where(live, gout[b, D:] / (n * np.sqrt(np.maximum(var, 0.0) + eps)), 0.0)
            d += coef * (rows - mean)
            m += np.abs(coef) * np.abs(rows - mean)
        dx[b, 0:int(lens[b]):period] = d
        M[b, 0:int(lens[b]):period] = m
    return dx, M
