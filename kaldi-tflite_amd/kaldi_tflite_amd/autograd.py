"""
ktf.autograd -- training the x-vector network on the GPU: the TDNN affine and the reducing statistics pooling as
`torch.autograd.Function`s over the library's kernels (forward: ktf_tdnn with KTF_GEMM_F32 / ktf_stats_pool, backward: the calls of
include/ktf_grad.h), batch normalisation in training mode, and `TrainableSequential`, a `torch.nn.Module` made from a
`ktf.models.Sequential` whose trained weights `export()` hands back to the inference kernels in every `gemm=` mode.

The GEMMs and the pooling run in the HIP kernels on fp32; padding to the kernels' operand layouts, ReLU and the batch normalisation
are torch ops on the same device, or -- `relu_batch_norm`, `TrainableSequential(fused_norm=True)` -- the kernels of
include/ktf_norm.h. `ClassifierHead` is the speaker classification head and its loss -- softmax, additive-margin and
additive-angular-margin cosine softmax -- over `row_inv_norm` and `margin_softmax_loss`, the kernels of include/ktf_loss.h around
a `tdnn_affine` GEMM; with sub-centres, an inter-top-k penalty or label smoothing switched on, the kernels of include/ktf_head.h.
There is no CPU path for the kernels: tensors that are not on the GPU are refused.

`gemm=` selects the matrix pipe of the TDNN GEMMs, forward and backward: "f32" (the exact-fp32 MFMA), "bf16" (operands rounded to
bf16 in the kernels, fp32 accumulation) or "bf16x3" (hi / lo split operands, three products: near-fp32 values). Parameters,
activations and gradients are fp32 tensors in every mode (include/ktf_grad.h rules 6 - 9).
"""

import torch

from . import _lib as L, layers as _layers, ops


def _desc(units, din, context, subsampling_factor, padding):
    context = [int(c) for c in context]
    if not 1 <= len(context) <= 16 or any(b <= a for a, b in zip(context, context[1:])):
        raise ValueError(f"context must be 1 to 16 strictly ascending offsets, got {context}")
    padding = str(padding).upper()
    if padding not in ("SAME", "VALID"):
        raise ValueError("padding should be either 'VALID' or 'SAME'")
    if int(subsampling_factor) <= 0:
        raise ValueError("subsampling_factor should be > 0")
    d = L.TdnnDesc()
    d.units, d.din, d.din_pad, d.nctx = int(units), int(din), ops.round_up(int(din), 32), len(context)
    for i, c in enumerate(context):
        d.ctx[i] = c
    d.subsampling, d.valid = int(subsampling_factor), int(padding == "VALID")
    d.act, d.gemm, d.flags = L.ACT_NONE, L.GEMM_F32, 0
    d.x_dtype = d.w_dtype = d.y_dtype = L.KTF_F32
    return d


_GEMMS = {"f32": L.GEMM_F32, "bf16": L.GEMM_BF16, "bf16x3": L.GEMM_BF16X3}


def _gemm_code(gemm):
    if gemm not in _GEMMS:
        raise ValueError(f"gemm must be one of {sorted(_GEMMS)}, got {gemm!r}")
    return _GEMMS[gemm]


def _on_gpu(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise L.KtfBackendError(f"{what} must be a tensor on the GPU: these functions run the library's kernels (no CPU fallback)")


def _lens(lens, B, device):
    if lens is None:
        return None
    lens = torch.as_tensor(lens, device=device).to(torch.int32).contiguous()
    if lens.shape != (B,):
        raise ValueError(f"lens must hold one length per utterance ({B}), got shape {tuple(lens.shape)}")
    return lens


def tdnn_out_lens(lens, context, subsampling_factor=1, padding="SAME"):
    """Valid output rows of a TDNN layer per utterance (the rule of ktf_tdnn_out_len) as torch integer arithmetic; None stays None."""
    if lens is None:
        return None
    start, end = 0, lens
    if str(padding).upper() == "VALID":
        start = -min(int(context[0]), 0)
        end = lens - max(int(context[-1]), 0)
    n = end - start + (int(subsampling_factor) - 1)
    return torch.clamp(torch.div(n, int(subsampling_factor), rounding_mode="floor"), min=0).to(torch.int32)


class _TdnnAffine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, lens, context, subsampling_factor, padding, gemm=L.GEMM_F32):
        B, T, D = x.shape
        units, nctx = weight.shape[0], weight.shape[1]
        d = _desc(units, D, context, subsampling_factor, padding)
        Dp, Up = d.din_pad, ops.round_up(units, 256)
        xp = torch.nn.functional.pad(x, (0, Dp - D)).contiguous()                # pad columns zero: finite, as the kernels ask
        wp = torch.zeros((Up, nctx, Dp), dtype=torch.float32, device=x.device)
        wp[:units, :, :D] = weight
        Tout = ops.tdnn_out_len(T, d)
        y = torch.zeros((B, Tout, units), dtype=torch.float32, device=x.device)  # rows at and beyond an utterance's output length stay zero
        if B > 0 and Tout > 0:
            b = None if bias is None else bias.contiguous()
            if gemm == L.GEMM_F32:
                ops.tdnn(xp, lens, d, wp.view(Up, nctx * Dp), None, b, None, None, y)
            else:                                                                # the 16-bit operand(s) of this call's fp32 parameter
                fd = _desc(units, D, context, subsampling_factor, padding)
                fd.gemm, fd.w_dtype = gemm, L.KTF_BF16
                wh = wp.view(Up, nctx * Dp).to(torch.bfloat16)                   # round to nearest even
                wl = (wp.view(Up, nctx * Dp) - wh.to(torch.float32)).to(torch.bfloat16) if gemm == L.GEMM_BF16X3 else None
                ops.tdnn(xp, lens, fd, wh, wl, b, None, None, y)
        ctx.save_for_backward(xp, wp, lens)
        ctx.desc, ctx.dims, ctx.has_bias, ctx.gemm = d, (D, units, nctx), bias is not None, gemm
        return y

    @staticmethod
    def backward(ctx, gy):
        xp, wp, lens = ctx.saved_tensors
        d = ctx.desc
        D, units, nctx = ctx.dims
        B, T, Dp = xp.shape
        Up = wp.shape[0]
        g = gy.to(torch.float32).contiguous()
        dx = dw = db = None
        need_w = ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])
        if B == 0 or g.shape[1] == 0:                       # no output row: nothing reaches the inputs
            if ctx.needs_input_grad[0]:
                dx = torch.zeros((B, T, D), dtype=torch.float32, device=xp.device)
            if need_w:
                dw = torch.zeros((units, nctx, D), dtype=torch.float32, device=xp.device)
                db = torch.zeros((units,), dtype=torch.float32, device=xp.device) if ctx.has_bias else None
            return dx, dw, db, None, None, None, None, None
        f32 = ctx.gemm == L.GEMM_F32
        ws = ops.grad_tdnn_workspace(B, T, d, xp.device) if f32 else ops.grad_tdnn16_workspace(B, T, d, ctx.gemm, xp.device)
        if ctx.needs_input_grad[0]:
            dxp = torch.empty_like(xp)
            if f32:
                ops.grad_tdnn_data(g, lens, d, wp.view(Up, nctx * Dp), dxp, ws)
            else:
                ops.grad_tdnn16_data(g, lens, d, wp.view(Up, nctx * Dp), dxp, ws, ctx.gemm)
            dx = dxp[:, :, :D]
        if need_w:
            dwp = torch.empty_like(wp)
            db = torch.empty((units,), dtype=torch.float32, device=xp.device) if ctx.has_bias else None
            if f32:
                ops.grad_tdnn_weights(xp, lens, d, g, dwp.view(Up, nctx * Dp), db, ws)
            else:
                ops.grad_tdnn16_weights(xp, lens, d, g, dwp.view(Up, nctx * Dp), db, ws, ctx.gemm)
            dw = dwp[:units, :, :D]
        return dx, dw, db, None, None, None, None, None


def tdnn_affine(x, weight, bias, context, lens=None, subsampling_factor=1, padding="SAME", gemm="f32"):
    """z[b,t,u] = bias[u] + sum_k sum_d x[b, row(t,k), d] * weight[u,k,d], row(t,k) = clip(start + t * subsampling_factor + context[k],
    0, len_b - 1), differentiable in x, weight and bias. x (B, T, D) fp32 on the GPU; weight (units, nctx, D) -- the [u, k, d] order of
    TDNN.device_weights; bias (units,) or None; lens (B,) or None (every utterance has T rows). Returns (B, T_out, units) with zero rows
    at and beyond an utterance's output length (`tdnn_out_lens`); gradients arriving for those rows are ignored. gemm: "f32", "bf16" or
    "bf16x3" -- the forward is ktf_tdnn in that mode on the fp32 x (its 16-bit weight operand made from `weight` on every call), the
    backward the ktf_grad_tdnn16_* calls on the fp32 x, weight and gradient."""
    code = _gemm_code(gemm)
    _on_gpu(x, "x")
    _on_gpu(weight, "weight")
    if x.dim() != 3 or weight.dim() != 3 or weight.shape[2] != x.shape[2] or weight.shape[1] != len(context):
        raise ValueError(f"expected x (B, T, D) and weight (units, {len(context)}, D), got {tuple(x.shape)} and {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError(f"bias shape {tuple(bias.shape)} != ({weight.shape[0]},)")
    return _TdnnAffine.apply(x.to(torch.float32), weight.to(torch.float32), None if bias is None else bias.to(torch.float32),
                             _lens(lens, x.shape[0], x.device), list(context), subsampling_factor, padding, code)


class _StatsPooling(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lens, include_std, epsilon, input_period):
        B, T, D = x.shape
        x = x.contiguous()
        out = torch.empty((B, 2 * D if include_std else D), dtype=torch.float32, device=x.device)
        ops.stats_pool(x, D, lens, input_period, include_std, epsilon, out)
        ctx.save_for_backward(x, lens)
        ctx.cfg = (include_std, epsilon, input_period)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, lens = ctx.saved_tensors
        include_std, epsilon, input_period = ctx.cfg
        dx = torch.empty_like(x)
        ops.grad_stats_pool(x, x.shape[2], lens, input_period, include_std, epsilon, gout.to(torch.float32).contiguous(), dx)
        return dx, None, None, None, None


def stats_pooling(x, lens=None, include_std=True, epsilon=1e-10, input_period=1):
    """The reducing StatsPooling, differentiable in x: (B, T, D) fp32 on the GPU -> (B, D or 2 D), mean and
    sqrt(relu(E[x^2] - mean^2) + epsilon) over the rows 0, input_period, ... below each utterance's length."""
    _on_gpu(x, "x")
    if x.dim() != 3:
        raise ValueError(f"expected a (batch, time, feat) input, got shape {tuple(x.shape)}")
    if int(input_period) <= 0:
        raise ValueError("'input_period' must be > 0")
    return _StatsPooling.apply(x.to(torch.float32), _lens(lens, x.shape[0], x.device), bool(include_std), float(epsilon), int(input_period))


class _AttentiveStatsPooling(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, e, lens, include_std, epsilon):
        B, T, D = x.shape
        H = e.shape[2]
        x, e = x.contiguous(), e.contiguous()
        out = torch.empty((B, 2 * D if include_std else D), dtype=torch.float32, device=x.device)
        norm = torch.empty((B, H, 2), dtype=torch.float64, device=x.device)
        stats = torch.empty((B, 2, D), dtype=torch.float64, device=x.device)
        ops.attn_pool(x, e, lens, include_std, epsilon, out, norm, stats)
        ctx.save_for_backward(x, e, lens, norm, stats)           # of the activation's size: x and e alone
        ctx.cfg = (include_std, epsilon)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, e, lens, norm, stats = ctx.saved_tensors
        include_std, epsilon = ctx.cfg
        dx, de = torch.empty_like(x), torch.empty_like(e)
        ops.attn_pool_backward(x, e, lens, include_std, epsilon, norm, stats, gout.to(torch.float32).contiguous(), dx, de,
                               ops.attn_pool_backward_workspace(x.shape[0], x.shape[2], e.shape[2], x.device))
        return dx, de, None, None, None


def attentive_stats_pooling(x, e, lens=None, include_std=True, epsilon=1e-10):
    """Attentive statistics pooling (include/ktf_attn.h), differentiable in x and e: x (B, T, D) and the attention logits e (B, T, H)
    fp32 on the GPU, 1 <= H <= D and D % H == 0 (channel c is weighted by head c // (D / H)) -> (B, D or 2 D): the mean and
    sqrt(relu(E[x^2] - mean^2) + epsilon) of x under w = softmax of e over the rows below each utterance's length. For the backward
    pass it keeps x, e, lens and two small fp64 tensors ((B, H, 2) and (B, 2, D)), nothing else of the activation's size."""
    if not (isinstance(x, torch.Tensor) and isinstance(e, torch.Tensor)) or x.dim() != 3 or e.dim() != 3 or x.shape[:2] != e.shape[:2]:
        raise ValueError(f"expected x (B, T, D) and e (B, T, H), got shapes {tuple(getattr(x, 'shape', ()))} and {tuple(getattr(e, 'shape', ()))}")
    D, H = x.shape[2], e.shape[2]
    if H < 1 or H > D or D % H:
        raise ValueError(f"the {H} heads of e must divide the {D} channels of x")
    if not 0.0 <= float(epsilon) < float("inf"):
        raise ValueError(f"epsilon must be finite and not negative, got {epsilon!r}")
    _on_gpu(x, "x")
    _on_gpu(e, "e")
    return _AttentiveStatsPooling.apply(x.to(torch.float32), e.to(torch.float32), _lens(lens, x.shape[0], x.device), bool(include_std),
                                        float(epsilon))


def batch_norm(x, lens, moving_mean, moving_var, gamma, momentum=0.99, epsilon=0.001, training=False):
    """BatchNorm as the project mirrors it (keras BatchNormalization(center=False, scale=True)): y = gamma (x - mean) / sqrt(var +
    epsilon) per feature. Training: mean and (biased) variance over the valid rows of the whole batch, and
    moving <- moving * momentum + batch * (1 - momentum), in place, for both statistics. Evaluation: the moving statistics.
    x (..., D); lens (B,) for a (B, T, D) input or None; rows at and beyond an utterance's length are not read and come out as zero.
    Elementwise torch ops: it runs wherever its tensors are."""
    mask = None
    if lens is not None:
        if x.dim() != 3:
            raise ValueError("lens goes with a (batch, time, feat) input")
        mask = (torch.arange(x.shape[1], device=x.device)[None, :] < lens.to(x.device)[:, None]).unsqueeze(-1)
        x = torch.where(mask, x, torch.zeros((), dtype=x.dtype, device=x.device))
    if training:
        dims = tuple(range(x.dim() - 1))
        if mask is None:
            n = x.numel() // x.shape[-1]
            mean = x.sum(dims) / n
            var = ((x - mean) ** 2).sum(dims) / n
        else:
            n = mask.sum().to(x.dtype)
            mean = x.sum(dims) / n
            var = (torch.where(mask, x - mean, torch.zeros((), dtype=x.dtype, device=x.device)) ** 2).sum(dims) / n
        with torch.no_grad():
            moving_mean.mul_(momentum).add_(mean.detach().to(moving_mean.dtype), alpha=1.0 - momentum)
            moving_var.mul_(momentum).add_(var.detach().to(moving_var.dtype), alpha=1.0 - momentum)
    else:
        mean, var = moving_mean, moving_var
    y = gamma * (x - mean) * torch.rsqrt(var + epsilon)
    return y if mask is None else torch.where(mask, y, torch.zeros((), dtype=y.dtype, device=y.device))


class _ReluBatchNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, gamma, lens, moving, momentum, epsilon, training, relu):
        B, T, D = z.shape
        z = z.contiguous()
        gamma = gamma.contiguous()
        y = torch.empty_like(z)
        saved = torch.empty((2, D), dtype=torch.float64, device=z.device)
        ops.norm_relu_bn_forward(z, D, lens, relu, training, gamma, moving[0], moving[1], momentum, epsilon, y, saved,
                                 ops.norm_workspace(B, T, D, z.device))
        ctx.save_for_backward(z, saved, gamma, lens)         # of the activation's size: z alone
        ctx.cfg = (training, relu)
        return y

    @staticmethod
    def backward(ctx, gy):
        z, saved, gamma, lens = ctx.saved_tensors
        training, relu = ctx.cfg
        B, T, D = z.shape
        dz = torch.empty_like(z)
        dgamma = torch.empty((D,), dtype=torch.float32, device=z.device) if ctx.needs_input_grad[1] else None
        ops.norm_relu_bn_backward(gy.to(torch.float32).contiguous(), z, D, lens, relu, training, gamma, saved, dz, dgamma,
                                  ops.norm_workspace(B, T, D, z.device))
        return dz if ctx.needs_input_grad[0] else None, dgamma, None, None, None, None, None, None


def relu_batch_norm(z, lens, moving_mean, moving_var, gamma, momentum=0.99, epsilon=0.001, training=False, relu=True):
    """`batch_norm(torch.relu(z), ...)` (relu=False: `batch_norm(z, ...)`) as one pair of the library's kernels (include/ktf_norm.h),
    differentiable in z and gamma: y = gamma (a - mean) / sqrt(var + epsilon) per feature with a = max(z, 0). z (B, T, D) with lens
    (B,) or None, or (N, D) without lens, fp32 on the GPU; moving_mean / moving_var (D,) fp32 on the GPU, updated in place when
    training; sums, statistics and every output value are fp64 arithmetic rounded once. Rows at and beyond an utterance's length are
    not read and come out as zero. For the backward pass it keeps z and the (2, D) fp64 mean / inverse deviation, no other tensor of
    the activation's size."""
    _on_gpu(z, "z")
    _on_gpu(gamma, "gamma")
    _on_gpu(moving_mean, "moving_mean")
    _on_gpu(moving_var, "moving_var")
    if z.dim() not in (2, 3) or (z.dim() == 2 and lens is not None):
        raise ValueError(f"expected z (B, T, D) with lens or None, or (N, D) without lens, got shape {tuple(z.shape)}")
    D = z.shape[-1]
    for name, t in (("moving_mean", moving_mean), ("moving_var", moving_var)):
        if t.dtype != torch.float32 or tuple(t.shape) != (D,) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous fp32 tensor of shape ({D},): it is updated in place")
    if tuple(gamma.shape) != (D,):
        raise ValueError(f"gamma shape {tuple(gamma.shape)} != ({D},)")
    z3 = z.to(torch.float32) if z.dim() == 3 else z.to(torch.float32).unsqueeze(0)
    y = _ReluBatchNorm.apply(z3, gamma.to(torch.float32), _lens(lens, z3.shape[0], z.device), (moving_mean, moving_var), float(momentum),
                             float(epsilon), bool(training), bool(relu))
    return y if z.dim() == 3 else y.squeeze(0)


class TrainableSequential(torch.nn.Module):
    """A `ktf.models.Sequential` (or an XvectorExtractor, whose TDNN stack is taken) as a torch module: TDNN -> ReLU -> BatchNorm ...
    -> reducing StatsPooling or AttentiveStatsPooling (its two affines and `attentive_stats_pooling`) -> TDNN (context [0]) ... Parameters start from the layers' current weights; `forward(feats, lens)`
    returns the last layer's output -- (B, T_out, units), or (B, units) behind the pooling -- for `ClassifierHead` (below) or a head and a loss written in torch;
    `export()` writes parameters and moving statistics back into the layers. The layers must be built (a Sequential with an Input, or
    one that has run or loaded weights). gemm: the mode of every TDNN GEMM, forward and backward ("f32", "bf16", "bf16x3": `tdnn_affine`),
    the (B, units) affines behind the pooling included; parameters are fp32 and `export()` is the same in every mode.
    fused_norm=True runs every BatchNorm as `relu_batch_norm`, on both sides of the pooling: together with a ReLU (a ReLU layer, or
    a TDNN's activation="relu") that stands immediately in front of it, with relu=False otherwise; a ReLU that no BatchNorm follows
    stays torch.relu. Parameters, buffers, their names and `export()` are the same either way."""

    def __init__(self, seq, device=None, gemm="f32", fused_norm=False):
        super().__init__()
        _gemm_code(gemm)
        if not isinstance(fused_norm, bool):
            raise ValueError(f"fused_norm must be True or False, got {fused_norm!r}")
        self.gemm = gemm
        self.fused_norm = fused_norm
        self.seq = getattr(seq, "xvec", seq)
        dev = ops.default_device() if device is None else torch.device(device)
        self.steps = []                     # (kind, the layer, index into self.params / self.stats)
        self.params = torch.nn.ParameterList()
        pooled = False
        f32 = lambda a: torch.nn.Parameter(torch.as_tensor(a, dtype=torch.float32).to(dev).contiguous().clone())  # noqa: E731
        for l in self.seq.layers:
            if not isinstance(l, (_layers.TDNN, _layers.ReLU, _layers.BatchNorm, _layers.StatsPooling, _layers.AttentiveStatsPooling)):
                raise NotImplementedError(f"layer '{l.name}' ({type(l).__name__}) has no gradient in ktf.autograd")
            if not l.built and not isinstance(l, (_layers.ReLU, _layers.StatsPooling)):
                raise ValueError(f"layer '{l.name}' is not built: give the Sequential an Input, run it or load its weights first")
            if isinstance(l, _layers.TDNN):
                act = l.activation.lower() if isinstance(l.activation, str) else l.activation
                if act not in (None, "linear", "relu"):
                    raise NotImplementedError(f"layer '{l.name}' (TDNN with activation {l.activation!r}) has no gradient in ktf.autograd")
                if pooled and (list(l.context) != [0] or l.subsamplingFactor != 1):
                    raise NotImplementedError(f"layer '{l.name}' (TDNN with context {l.context} behind the pooling) has no gradient in ktf.autograd")
                at = len(self.params)
                self.params.append(f32(l.kernel[0].transpose(2, 0, 1)))                     # keras (K, D, units) -> [u, k, d]
                if l.useBias:
                    self.params.append(f32(l.bias))
                self.steps.append(("tdnn", l, at))
            elif isinstance(l, _layers.BatchNorm):
                at = len(self.params)
                self.params.append(f32(l.gamma))
                self.register_buffer(f"moving_mean_{at}", torch.as_tensor(l.moving_mean, dtype=torch.float32).to(dev).clone())
                self.register_buffer(f"moving_var_{at}", torch.as_tensor(l.moving_variance, dtype=torch.float32).to(dev).clone())
                self.steps.append(("bn", l, at))
            elif isinstance(l, _layers.StatsPooling):
                if pooled or not l.reduce:
                    raise NotImplementedError(f"layer '{l.name}' (StatsPooling that does not reduce the time axis, or a second one) "
                                              "has no gradient in ktf.autograd")
                pooled = True
                self.steps.append(("stats", l, -1))
            elif isinstance(l, _layers.AttentiveStatsPooling):
                act = l.attentionActivation.lower() if isinstance(l.attentionActivation, str) else l.attentionActivation
                if pooled or act not in ("tanh", "relu"):
                    raise NotImplementedError(f"layer '{l.name}' (AttentiveStatsPooling with activation {l.attentionActivation!r}, or a "
                                              "second pooling) has no gradient in ktf.autograd")
                pooled = True
                at = len(self.params)
                for t in (l.hidden, l.logits):                     # W1 [u, k, d], b1, W2 [u, k, d], b2
                    self.params.append(f32(t.kernel[0].transpose(2, 0, 1)))
                    self.params.append(f32(t.bias))
                self.steps.append(("attn", l, at))
            else:
                self.steps.append(("relu", l, -1))

    def forward(self, feats, lens=None):
        x, pooled = feats, False
        lens = _lens(lens, feats.shape[0], feats.device)
        held = False                                               # a ReLU waiting for the BatchNorm behind it (fused_norm)
        for i, (kind, l, at) in enumerate(self.steps):
            into_bn = self.fused_norm and i + 1 < len(self.steps) and self.steps[i + 1][0] == "bn"
            if kind == "tdnn":
                w, b = self.params[at], self.params[at + 1] if l.useBias else None
                if pooled:                                         # one row per utterance: a single sequence of B rows
                    x = tdnn_affine(x.unsqueeze(0), w, b, l.context, gemm=self.gemm).squeeze(0)
                else:
                    x = tdnn_affine(x, w, b, l.context, lens, l.subsamplingFactor, l.padding, self.gemm)
                    lens = tdnn_out_lens(lens, l.context, l.subsamplingFactor, l.padding)
                if isinstance(l.activation, str) and l.activation.lower() == "relu":
                    held = into_bn
                    x = x if held else torch.relu(x)
            elif kind == "relu":
                held = into_bn
                x = x if held else torch.relu(x)
            elif kind == "bn" and self.fused_norm:
                x = relu_batch_norm(x, None if pooled else lens, getattr(self, f"moving_mean_{at}"), getattr(self, f"moving_var_{at}"),
                                    self.params[at], l.momentum, l.epsilon, self.training, relu=held)
                held = False
            elif kind == "bn":
                x = batch_norm(x, None if pooled else lens, getattr(self, f"moving_mean_{at}"), getattr(self, f"moving_var_{at}"),
                               self.params[at], l.momentum, l.epsilon, self.training)
            elif kind == "attn":
                h = tdnn_affine(x, self.params[at], self.params[at + 1], [0], lens, gemm=self.gemm)
                h = torch.tanh(h) if l.attentionActivation.lower() == "tanh" else torch.relu(h)
                e = tdnn_affine(h, self.params[at + 2], self.params[at + 3], [0], lens, gemm=self.gemm)
                x = attentive_stats_pooling(x, e, lens, l.includeStd, l.epsilon)
                pooled = True
            else:
                x = stats_pooling(x, lens, l.includeStd, l.epsilon, l.inputPeriod)
                pooled = True
        return x

    def export(self):
        """Write parameters and moving statistics back into the Sequential's layers (set_weights(..., fmt="tensorflow")): their
        version counters invalidate device operand sets and captured graphs, and the model then runs in any gemm mode."""
        for kind, l, at in self.steps:
            if kind == "tdnn":
                kernel = self.params[at].detach().permute(1, 2, 0).unsqueeze(0).cpu().numpy()        # [u, k, d] -> keras (1, K, D, units)
                l.set_weights([kernel] + ([self.params[at + 1].detach().cpu().numpy()] if l.useBias else []), fmt="tensorflow")
            elif kind == "bn":
                l.set_weights([self.params[at].detach().cpu().numpy(), getattr(self, f"moving_mean_{at}").cpu().numpy(),
                               getattr(self, f"moving_var_{at}").cpu().numpy()], fmt="tensorflow")
            elif kind == "attn":
                w1, b1, w2, b2 = (self.params[at + k].detach().cpu().numpy() for k in range(4))
                l.set_weights([w1[:, 0, :].T, b1, w2[:, 0, :].T, b2], fmt="tensorflow")
        return self.seq


# ----------------------------------------------------------------------------- the classification head and its loss (include/ktf_loss.h)
class _RowInvNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        x = x.contiguous()
        inv = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
        ops.loss_row_inv_norm(x, eps, inv)
        ctx.save_for_backward(x, inv)
        ctx.eps = eps
        return inv

    @staticmethod
    def backward(ctx, ginv):
        x, inv = ctx.saved_tensors
        dx = torch.empty_like(x)
        ops.loss_row_inv_norm_backward(x, ctx.eps, inv, ginv.to(torch.float32).contiguous(), dx)
        return dx, None


def row_inv_norm(x, eps=1e-12):
    """1 / max(|x[r]|, eps) per row of x (rows, D) fp32 on the GPU -> (rows,), differentiable in x (zero gradient for a row that eps
    clamped): the kernels of include/ktf_loss.h, the sum of squares in fp64 and every value rounded once."""
    if not float(eps) > 0.0 or float(eps) == float("inf"):
        raise ValueError(f"eps must be positive and finite, got {eps!r}")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] < 1:
        raise ValueError(f"expected x (rows, D) with D >= 1, got shape {tuple(getattr(x, 'shape', ()))}")
    _on_gpu(x, "x")
    return _RowInvNorm.apply(x.to(torch.float32), float(eps))


class _MarginSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, labels, inv_x, inv_w, kind, margin, scale):
        B, N = z.shape
        z = z.contiguous()
        loss = torch.empty((B,), dtype=torch.float32, device=z.device)
        pred = torch.empty((B,), dtype=torch.int32, device=z.device)
        lse = torch.empty((B,), dtype=torch.float64, device=z.device)
        ops.loss_margin_softmax_forward(z, labels, inv_x, inv_w, kind, margin, scale, loss, pred, lse, ops.loss_workspace(B, N, z.device))
        ctx.save_for_backward(z, labels, lse, inv_x, inv_w)      # of the logits' size: z alone
        ctx.cfg = (kind, margin, scale)
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    def backward(ctx, gloss, _gpred):
        z, labels, lse, inv_x, inv_w = ctx.saved_tensors
        kind, margin, scale = ctx.cfg
        B, N = z.shape
        dz = torch.empty_like(z)
        dix = diw = None
        if inv_x is not None:
            dix = torch.empty((B,), dtype=torch.float32, device=z.device)
            diw = torch.empty((N,), dtype=torch.float32, device=z.device)
        ops.loss_margin_softmax_backward(z, labels, inv_x, inv_w, kind, margin, scale, lse, gloss.to(torch.float32).contiguous(), dz, dix, diw,
                                         ops.loss_workspace(B, N, z.device))
        return dz, None, dix, diw, None, None, None


def _loss_args(kind, margin, scale, cosine):
    if kind not in ops.LOSS_KINDS:
        raise ValueError(f"kind must be one of {sorted(ops.LOSS_KINDS)}, got {kind!r}")
    margin, scale = float(margin), float(scale)
    if not 0.0 < scale < float("inf"):
        raise ValueError(f"scale must be positive and finite, got {scale!r}")
    if not 0.0 <= margin < float("inf"):
        raise ValueError(f"margin must be finite and not negative, got {margin!r}")
    if kind == "softmax" and margin != 0.0:
        raise ValueError(f"margin must be 0 with kind='softmax', got {margin!r}")
    if kind == "aam" and margin >= 1.5707963267948966:
        raise ValueError(f"margin must be below pi / 2 with kind='aam', got {margin!r}")
    if kind != "softmax" and not cosine:
        raise ValueError(f"kind={kind!r} needs a cosine head: give inv_norm_x and inv_norm_w (normalize=True)")
    return margin, scale


class _HeadLoss(torch.autograd.Function):
    """include/ktf_head.h: sub-centres, the inter-top-k penalty and label smoothing."""

    @staticmethod
    def forward(ctx, z, labels, inv_x, inv_w, kind, margin, scale, K, topk, penalty, smoothing):
        B = z.shape[0]
        N = z.shape[1] // K
        z = z.contiguous()
        loss = torch.empty((B,), dtype=torch.float32, device=z.device)
        pred = torch.empty((B,), dtype=torch.int32, device=z.device)
        sub_y = torch.empty((B,), dtype=torch.int32, device=z.device)
        lse = torch.empty((B,), dtype=torch.float64, device=z.device)
        hard = torch.empty((B, max(topk, 1)), dtype=torch.int32, device=z.device)
        ops.head_forward(z, K, labels, inv_x, inv_w, kind, margin, scale, topk, penalty, smoothing, loss, pred, lse, hard, sub_y,
                         ops.head_workspace(B, N, K, z.device))
        ctx.save_for_backward(z, labels, lse, hard, inv_x, inv_w)    # of the logits' size: z alone
        ctx.cfg = (kind, margin, scale, K, topk, penalty, smoothing)
        ctx.mark_non_differentiable(pred, sub_y)
        return loss, pred, sub_y

    @staticmethod
    def backward(ctx, gloss, _gpred, _gsub):
        z, labels, lse, hard, inv_x, inv_w = ctx.saved_tensors
        kind, margin, scale, K, topk, penalty, smoothing = ctx.cfg
        B = z.shape[0]
        dz = torch.empty_like(z)
        dix = diw = None
        if inv_x is not None:
            dix = torch.empty((B,), dtype=torch.float32, device=z.device)
            diw = torch.empty((z.shape[1],), dtype=torch.float32, device=z.device)
        ops.head_backward(z, K, labels, inv_x, inv_w, kind, margin, scale, topk, penalty, smoothing, lse, hard,
                          gloss.to(torch.float32).contiguous(), dz, dix, diw, ops.head_workspace(B, z.shape[1] // K, K, z.device))
        return dz, None, dix, diw, None, None, None, None, None, None, None


def _head_args(sub_centers, top_k, penalty, label_smoothing, cosine):
    for name, v, hi in (("sub_centers", sub_centers, L.HEAD_MAX_CENTERS), ("top_k", top_k, L.HEAD_MAX_TOPK)):
        lo = 1 if name == "sub_centers" else 0
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")
    penalty, label_smoothing = float(penalty), float(label_smoothing)
    if not 0.0 <= penalty < float("inf"):
        raise ValueError(f"penalty must be finite and not negative, got {penalty!r}")
    if top_k == 0 and penalty != 0.0:
        raise ValueError(f"penalty must be 0 with top_k=0, got {penalty!r}")
    if not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing!r}")
    if sub_centers > 1 and not cosine:
        raise ValueError(f"sub_centers={sub_centers} needs a cosine head: give inv_norm_x and inv_norm_w (normalize=True)")
    if top_k > 0 and not cosine:
        raise ValueError(f"top_k={top_k} needs a cosine head: give inv_norm_x and inv_norm_w (normalize=True)")
    return penalty, label_smoothing


def _head_loss(z, labels, kind, margin, scale, inv_norm_x, inv_norm_w, sub_centers, top_k, penalty, label_smoothing):
    """margin_softmax_loss with the selected centre of the target class as a third result (None on the path of ktf_loss.h)."""
    if (inv_norm_x is None) != (inv_norm_w is None):
        raise ValueError("inv_norm_x and inv_norm_w go together: both for a cosine head, neither for a plain one")
    margin, scale = _loss_args(kind, margin, scale, inv_norm_x is not None)
    penalty, label_smoothing = _head_args(sub_centers, top_k, penalty, label_smoothing, inv_norm_x is not None)
    if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.shape[1] < 1 or z.shape[1] % sub_centers:
        raise ValueError(f"expected z (B, N * sub_centers) with N >= 1 and sub_centers = {sub_centers}, "
                         f"got shape {tuple(getattr(z, 'shape', ()))}")
    B, N = z.shape[0], z.shape[1] // sub_centers
    labels = torch.as_tensor(labels, device=z.device)
    if tuple(labels.shape) != (B,) or labels.dtype.is_floating_point:
        raise ValueError(f"labels must hold one integer per row ({B}), got {labels.dtype} of shape {tuple(labels.shape)}")
    for name, t, n in (("inv_norm_x", inv_norm_x, B), ("inv_norm_w", inv_norm_w, N * sub_centers)):
        if t is not None and tuple(t.shape) != (n,):
            raise ValueError(f"{name} shape {tuple(t.shape)} != ({n},)")
    _on_gpu(z, "z")
    if inv_norm_x is not None:
        _on_gpu(inv_norm_x, "inv_norm_x")
        _on_gpu(inv_norm_w, "inv_norm_w")
        inv_norm_x, inv_norm_w = inv_norm_x.to(torch.float32).contiguous(), inv_norm_w.to(torch.float32).contiguous()
    labels = labels.clamp(-1, N).to(torch.int32).contiguous()            # int64 labels beyond int32 stay out of range
    if sub_centers == 1 and top_k == 0 and label_smoothing == 0.0:       # the kernels of ktf_loss.h, as before there were others
        return _MarginSoftmax.apply(z.to(torch.float32), labels, inv_norm_x, inv_norm_w, kind, margin, scale) + (None,)
    return _HeadLoss.apply(z.to(torch.float32), labels, inv_norm_x, inv_norm_w, kind, margin, scale, sub_centers, top_k, penalty,
                           label_smoothing)


def margin_softmax_loss(z, labels, kind="softmax", margin=0.0, scale=1.0, inv_norm_x=None, inv_norm_w=None, sub_centers=1, top_k=0,
                        penalty=0.0, label_smoothing=0.0):
    """Softmax cross entropy over the logits of a classification head, with the large-margin cosine variants, as one pair of the
    library's kernels (include/ktf_loss.h) -> (loss (B,) fp32, pred (B,) int32). z (B, N) fp32 on the GPU: the dot products x_b . w_j;
    labels (B,) integers, a label outside [0, N) marks an ignored row (loss 0, no gradient). With inv_norm_x (B,) and inv_norm_w (N,)
    -- `row_inv_norm` of the embeddings and of the weight -- the head is a cosine head, c = z * inv_norm_x[:, None] * inv_norm_w, and
    the logits are scale * c with the target column replaced by scale * psi(c): kind "softmax": psi(c) = c; "am": c - margin; "aam":
    cos(theta + margin), continued by c - margin * sin(margin) beyond theta = pi - margin. Without them the head is plain (logits
    scale * z, kind "softmax" only). pred is the column of the largest cosine without margin. Differentiable in z, inv_norm_x and
    inv_norm_w; fp64 arithmetic rounded once, no atomics; keeps z and the (B,) fp64 log-sum-exp for the backward pass.

    Three switches, separately or together, run the kernels of include/ktf_head.h instead (with all of them off nothing changes):
    sub_centers = K > 1 (cosine head): z is (B, N * K), column j * K + k the centre k of class j, inv_norm_w (N * K,); a class's cosine
    is the largest of its centres', and only that centre gets a gradient. top_k > 0 (cosine head): the top_k classes other than the
    target with the largest cosines (ties: the lower class) get `penalty` added to their cosine. label_smoothing = e in [0, 1): the
    target distribution is (1 - e) on the label plus e / N everywhere. That path keeps z, the log-sum-exp and the (B, top_k) int32
    list of penalised classes, and pred is the class (not the column) of the largest cosine."""
    return _head_loss(z, labels, kind, margin, scale, inv_norm_x, inv_norm_w, sub_centers, top_k, penalty, label_smoothing)[:2]


class ClassifierHead(torch.nn.Module):
    """The speaker classification head of x-vector training and its loss: weight (num_classes, dim) [and bias], the GEMM
    `tdnn_affine(emb.unsqueeze(0), weight.unsqueeze(1), bias, [0], gemm=gemm)`, and `margin_softmax_loss` over it. normalize=True
    (the default for kind "am" and "aam", which need it) makes it a cosine head: `row_inv_norm` of the fp32 embeddings and of the
    fp32 weight in every gemm mode; normalize=False (the default for kind "softmax") a plain affine head, the only one that takes a
    bias. margin defaults to 0.2 (0 for "softmax"), scale to 30 (1 for a plain head); both are plain attributes read at every call,
    so a margin warm-up is one assignment per step. `forward(emb, labels)` -> (the mean loss of the valid rows -- 0 when there is
    none --, pred (B,) int32); labels outside [0, num_classes) mark rows to ignore. No torch op touches a (B, num_classes) or
    (num_classes, dim) tensor in forward or backward.

    sub_centers = K > 1 gives every class K centres: weight is (num_classes * K, dim), class-major (row j * K + k is centre k of class
    j); top_k, penalty and label_smoothing are those of `margin_softmax_loss` and, like margin and scale, plain attributes read at
    every call. With one of them set the loss runs the kernels of include/ktf_head.h; with none, those of include/ktf_loss.h as
    before. A head with K > 1 counts in training mode, in the buffer `center_counts` (num_classes, K) int64, how often each centre
    was the one its class's target rows selected; `dominant()` reduces the head to those centres."""

    def __init__(self, dim, num_classes, kind="aam", margin=None, scale=None, bias=False, gemm="f32", device=None, normalize=None, eps=1e-12,
                 sub_centers=1, top_k=0, penalty=0.0, label_smoothing=0.0):
        super().__init__()
        for name, v in (("dim", dim), ("num_classes", num_classes)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
        if kind not in ops.LOSS_KINDS:
            raise ValueError(f"kind must be one of {sorted(ops.LOSS_KINDS)}, got {kind!r}")
        if normalize is None:
            normalize = kind != "softmax"
        if not isinstance(normalize, bool) or not isinstance(bias, bool):
            raise ValueError(f"normalize and bias must be True or False, got normalize={normalize!r}, bias={bias!r}")
        if bias and normalize:
            raise ValueError("bias goes only with a plain head (kind='softmax', normalize=False)")
        _gemm_code(gemm)
        self.dim, self.num_classes, self.kind, self.normalize, self.gemm, self.eps = dim, num_classes, kind, normalize, gemm, float(eps)
        self.margin = (0.0 if kind == "softmax" else 0.2) if margin is None else margin
        self.scale = (30.0 if normalize else 1.0) if scale is None else scale
        _loss_args(kind, self.margin, self.scale, normalize)
        self.sub_centers, self.top_k, self.penalty, self.label_smoothing = sub_centers, top_k, penalty, label_smoothing
        _head_args(sub_centers, top_k, penalty, label_smoothing, normalize)
        if not self.eps > 0.0:
            raise ValueError(f"eps must be positive, got {eps!r}")
        dev = ops.default_device() if device is None else torch.device(device)
        self.weight = torch.nn.Parameter(torch.randn((num_classes * sub_centers, dim), dtype=torch.float32, device=dev) * dim ** -0.5)
        self.bias = torch.nn.Parameter(torch.zeros((num_classes,), dtype=torch.float32, device=dev)) if bias else None
        if sub_centers > 1:                              # a head with one centre per class keeps the state_dict it always had
            self.register_buffer("center_counts", torch.zeros((num_classes, sub_centers), dtype=torch.int64, device=dev))
        else:
            self.center_counts = None

    def _logits(self, emb):
        if not isinstance(emb, torch.Tensor) or emb.dim() != 2 or emb.shape[1] != self.dim:
            raise ValueError(f"expected emb (B, {self.dim}), got shape {tuple(getattr(emb, 'shape', ()))}")
        emb = emb.to(torch.float32)
        z = tdnn_affine(emb.unsqueeze(0), self.weight.unsqueeze(1), self.bias, [0], gemm=self.gemm).squeeze(0)
        if not self.normalize:
            return z, None, None
        return z, row_inv_norm(emb, self.eps), row_inv_norm(self.weight, self.eps)

    def forward(self, emb, labels):
        margin, scale = _loss_args(self.kind, self.margin, self.scale, self.normalize)
        _head_args(self.sub_centers, self.top_k, self.penalty, self.label_smoothing, self.normalize)
        z, ix, iw = self._logits(emb)
        loss, pred, sub_y = _head_loss(z, labels, self.kind, margin, scale, ix, iw, self.sub_centers, self.top_k, self.penalty,
                                       self.label_smoothing)
        labels = torch.as_tensor(labels, device=loss.device)
        ok = (labels >= 0) & (labels < self.num_classes)
        if self.training and self.center_counts is not None:    # sub_y is -1 on an ignored row
            at = labels.clamp(0, self.num_classes - 1).to(torch.int64) * self.sub_centers + sub_y.clamp(min=0).to(torch.int64)
            self.center_counts.view(-1).index_add_(0, at, ok.to(torch.int64))
        valid = ok.sum().clamp(min=1)
        return loss.sum() / valid, pred                  # an ignored row's loss is 0

    def cosines(self, emb):
        """For evaluation: the (B, num_classes) cosines of a cosine head (the logits of a plain one), scaled in torch; with
        sub-centres the largest of each class's centres."""
        z, ix, iw = self._logits(emb)
        c = z if ix is None else z * ix[:, None] * iw[None, :]
        return c if self.sub_centers == 1 else c.view(c.shape[0], self.num_classes, self.sub_centers).amax(dim=2)

    def dominant(self):
        """A new head with sub_centers=1 that holds, for every class, the centre `center_counts` names most often (the lowest k among
        equal counts): the usual clean-up after sub-centre training. Every other setting is this head's."""
        K = self.sub_centers
        new = ClassifierHead(self.dim, self.num_classes, self.kind, self.margin, self.scale, self.bias is not None, self.gemm,
                             self.weight.device, self.normalize, self.eps, 1, self.top_k, self.penalty, self.label_smoothing)
        with torch.no_grad():
            if K == 1:
                new.weight.copy_(self.weight)
            else:
                best = dominant_centers(self.center_counts)
                rows = torch.arange(self.num_classes, device=self.weight.device) * K + best.to(self.weight.device)
                new.weight.copy_(self.weight.index_select(0, rows))
            if self.bias is not None:
                new.bias.copy_(self.bias)
        return new.train(self.training)


def dominant_centers(counts):
    """counts (N, K) integers -> (N,) int64: the most counted centre of every class, the lowest k among equal counts."""
    counts = torch.as_tensor(counts).to(torch.int64)
    K = counts.shape[1]
    return (counts * K + torch.arange(K - 1, -1, -1, device=counts.device)).argmax(dim=1)    # the keys of a row are distinct
