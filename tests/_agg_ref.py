"""Multi-layer feature aggregation (include/ktf_agg.h) restated in fp64 NumPy, one utterance at a time, straight from the header's
formula; the exactly representable inputs that tests/test_gpu_agg.py compares bit for bit; and the small training model of that file
with its fp64 torch restatement (tests/test_agg_cpu.py checks the exactness and that the model's ReLU inputs stay away from zero)."""

import numpy as np
import torch

EXACT_SHAPES = [((32, 32), 1), ((32, 64), 17), ((64, 32, 32), 128), ((32, 32, 32, 32), 129), ((96, 96, 96), 288)]      # (C_s ..., units)


def clamp_len(n, T):
    return int(min(max(int(n), 0), T))


def conv(xs, w, bias=None, nscale=None, nshift=None, relu=False):
    """xs: S arrays (n, C_s); w (units, K) -> y (n, units) fp64: z = sum_s x_s w[:, off_s : off_s + C_s]^T, y = act(z + bias) nscale + nshift."""
    w, off, z = np.asarray(w, np.float64), 0, 0.0
    for x in xs:
        C = x.shape[1]
        z = z + np.asarray(x, np.float64) @ w[:, off:off + C].T
        off += C
    assert off == w.shape[1]
    z = z + (0.0 if bias is None else np.asarray(bias, np.float64))
    a = np.maximum(z, 0.0) if relu else z
    return a if nscale is None else a * np.asarray(nscale, np.float64) + np.asarray(nshift, np.float64)


def batch(xs, lens, w, **kw):
    """xs: S arrays (B, T, C_s), lens (B,) or None -> the list of conv() over every utterance's valid rows ((0, units) for an empty one)."""
    B, T = xs[0].shape[:2]
    ns = [T if lens is None else clamp_len(lens[b], T) for b in range(B)]
    return [conv([x[b, :n] for x in xs], w, **kw) if n else np.zeros((0, np.shape(w)[0])) for b, n in enumerate(ns)]


def exact_lens(R):
    return [0, 1, 2, R - 1, R, R + 1, 2 * R + 1]


def exact_case(widths, units, lens, seed=0):
    """xs of integers in [-8, 8] with max(lens) + 3 rows, w in {-1, 0, 1} with four non-zeros per unit and source, integer bias and nshift
    in [-3, 3], nscale = 2^-2: dict(xs, w, bias, nscale, nshift), all fp32."""
    rng = np.random.default_rng(seed + 7 * sum(widths) + units)
    xs = [rng.integers(-8, 9, (len(lens), max(lens) + 3, C)).astype(np.float32) for C in widths]
    w, off = np.zeros((units, sum(widths)), np.float32), 0
    for C in widths:
        for u in range(units):
            w[u, off + rng.choice(C, 4, replace=False)] = rng.choice([-1.0, 1.0], 4)
        off += C
    ints = lambda: rng.integers(-3, 4, units).astype(np.float32)      # noqa: E731
    return dict(xs=xs, w=w, bias=ints(), nscale=np.full(units, 0.25, np.float32), nshift=ints())


# ---- the training model of tests/test_gpu_agg.py: TDNN a (relu) -> TDNN b (relu) -> TDNN c -> Aggregate([a, b], relu) -> pooling -> TDNN
TRAIN = dict(D=24, C=32, U=64, EMB=8, B=3, T=40, lens=[40, 17, 1], seed=4)


def train_model(ktf):
    t = TRAIN
    layers = [ktf.layers.TDNN(t["C"], name="a", activation="relu"), ktf.layers.TDNN(t["C"], name="b", activation="relu"), ktf.layers.TDNN(t["C"], name="c"),
              ktf.layers.Aggregate(t["U"], ["a", "b"], activation="relu", name="mfa"), ktf.layers.StatsPooling(0, 10000, reduce_time_axis=True),
              ktf.layers.TDNN(t["EMB"], name="out")]
    mdl = ktf.models.Sequential([ktf.models.Input(shape=(None, t["D"]))] + layers, name="mfa_net")
    feats = np.random.default_rng(t["seed"]).standard_normal((t["B"], t["T"], t["D"])).astype(np.float32)
    return mdl, feats


def train_params(mdl):
    """The fp32 parameters in TrainableSequential's order, as numpy: TDNN [u, k, d] and bias; the Aggregate's (units, K) and bias."""
    out = []
    for l in mdl.layers:
        if hasattr(l, "context"):
            out += [l.kernel[0].transpose(2, 0, 1), l.bias]
        elif hasattr(l, "sources"):
            out += [l.kernel.T, l.bias]
    return out


def restated(mdl, params, feats, lens, pre=None):
    """The model in torch ops on `feats`' dtype, the aggregation as torch.cat and a matrix product; `pre` receives every ReLU's input."""
    from test_tdnn_grad_cpu import restated_pool, restated_tdnn
    x, it, kept = feats, iter(params), {}
    rows = torch.arange(feats.shape[1])[None, :, None] < torch.tensor(lens)[:, None, None]
    for l in mdl.layers:
        if hasattr(l, "context") and x.dim() == 3:
            x = restated_tdnn(x, next(it), next(it), lens, [0], 1, "SAME")
        elif hasattr(l, "context"):
            x = x @ next(it)[:, 0, :].T + next(it)
        elif hasattr(l, "sources"):
            x = (torch.cat([kept[n] for n in l.sources] + [x], 2) @ next(it).T + next(it)) * rows
        else:
            x = restated_pool(x, lens, l.includeStd, l.epsilon, l.inputPeriod)
        if getattr(l, "activation", None) == "relu":
            if pre is not None:
                pre.append(torch.cat([x[b, :n].reshape(-1) for b, n in enumerate(lens)]))
            x = torch.relu(x)
        kept[l.name] = x
    return x
