"""
ktf.optim -- the optimiser step of training on the library's own kernels (include/ktf_optim.h):
SGD (momentum, Nesterov) or Adam over one flat arena of parameters, gradients and state, with gradient clipping by global norm
and max-change limits per tensor and for the whole model. `Optimizer` is a torch.optim.Optimizer, so torch.optim.lr_scheduler
works on it unchanged; a step is one library call with no host synchronisation.
"""

import math

import torch

from . import _lib as L
from . import ops

KINDS = ("sgd", "adam")


def kaldi_lr(step, num_steps, initial, final):
    """The recipe's exponential schedule: initial * exp(step / num_steps * log(final / initial)); `initial` at step 0, `final` at
    step num_steps. For assigning to group["lr"]."""
    if not (num_steps > 0):
        raise ValueError(f"num_steps must be positive, got {num_steps}")
    if not (initial > 0 and final > 0 and math.isfinite(initial) and math.isfinite(final)):
        raise ValueError(f"initial and final must be positive and finite, got {initial}, {final}")
    return initial * math.exp(step / num_steps * math.log(final / initial))


def _number(name, x, lo=0.0, hi=None, lo_open=False):
    """x as a float in [lo, hi) (or (lo, hi) with lo_open), finite; a ValueError that names the argument otherwise."""
    try:
        f = float(x)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number, got {x!r}") from None
    ok = math.isfinite(f) and (f > lo if lo_open else f >= lo) and (hi is None or f < hi)
    if not ok:
        bounds = f"{'(' if lo_open else '['}{lo}, {'inf' if hi is None else hi})"
        raise ValueError(f"{name} must be finite and in {bounds}, got {x!r}")
    return f


class Optimizer(torch.optim.Optimizer):
    """Optimizer(params_or_groups, kind="sgd", lr=..., momentum=0, nesterov=False, weight_decay=0, decoupled=False,
    betas=(0.9, 0.999), eps=1e-8, max_change=0, max_change_global=0, clip_norm=0).

    Group options: lr, weight_decay (read at every step) and max_change (per tensor, read at construction: it is stored in the
    tensor's segment). Construction moves every parameter into a slot-aligned segment of one arena, re-points `param.data` at a view
    of it (values bit for bit) and `param.grad` at a zero view of the gradient arena. `stats` is the device tensor of
    include/ktf_optim.h rule 12: G, c, N, sigma, skipped, then sigma_s per parameter in the order of the groups."""

    def __init__(self, params, kind="sgd", lr=None, momentum=0.0, nesterov=False, weight_decay=0.0, decoupled=False, betas=(0.9, 0.999),
                 eps=1e-8, max_change=0.0, max_change_global=0.0, clip_norm=0.0):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        if lr is None:
            raise ValueError("lr is required")
        self.kind = kind
        self.momentum = _number("momentum", momentum, 0.0, 1.0)
        self.nesterov = bool(nesterov)
        if self.nesterov and (kind != "sgd" or self.momentum == 0.0):
            raise ValueError("nesterov needs kind='sgd' and a momentum above 0")
        if not (isinstance(betas, (tuple, list)) and len(betas) == 2):
            raise ValueError(f"betas must be a pair, got {betas!r}")
        self.betas = (_number("betas[0]", betas[0], 0.0, 1.0), _number("betas[1]", betas[1], 0.0, 1.0))
        self.eps = _number("eps", eps, 0.0, None, lo_open=True)
        self.decoupled = bool(decoupled)
        self.max_change_global = _number("max_change_global", max_change_global)
        self.clip_norm = _number("clip_norm", clip_norm)
        defaults = dict(lr=_number("lr", lr), weight_decay=_number("weight_decay", weight_decay), max_change=_number("max_change", max_change))
        self._built = False
        super().__init__(params, defaults)
        if len(self.param_groups) > L.OPTIM_MAX_GROUPS:
            raise ValueError(f"at most {L.OPTIM_MAX_GROUPS} parameter groups, got {len(self.param_groups)}")
        for gi, group in enumerate(self.param_groups):
            for name in ("lr", "weight_decay", "max_change"):
                _number(f"{name} of group {gi}", group[name])

        self._params = [p for group in self.param_groups for p in group["params"]]
        dev = self._params[0].device
        for i, p in enumerate(self._params):
            if not p.is_cuda or p.dtype != torch.float32 or p.device != dev:
                raise L.KtfBackendError(f"parameter {i} is {p.dtype} on {p.device}: ktf.optim takes fp32 parameters on one GPU "
                                        f"(the first is on {dev}); there is no CPU path")
        L.require_gpu()
        slot = ops.optim_slot_elems()
        rows, cursor = [], 0
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                rows.append((cursor, cursor + p.numel(), gi, group["max_change"]))
                cursor = -(-(cursor + p.numel()) // slot) * slot
        self._rows, self._total = rows, max(cursor, slot)
        with torch.no_grad():
            self._p = torch.zeros((self._total,), dtype=torch.float32, device=dev)
            self._g = torch.zeros_like(self._p)
            self._m = torch.zeros_like(self._p) if (kind == "adam" or self.momentum != 0.0) else None
            self._v = torch.zeros_like(self._p) if kind == "adam" else None
            self._gviews = []
            for p, (begin, end, _, _) in zip(self._params, rows):
                view = self._p[begin:end].view(p.shape)
                view.copy_(p.data)
                p.data = view
                p.grad = self._g[begin:end].view(p.shape)
                self._gviews.append(p.grad)
        self._segs_host, self._segs_dev = ops.optim_segments(rows, dev)
        self._workspace = ops.optim_workspace(self._total, len(rows), dev)
        self.stats = torch.zeros((5 + len(rows),), dtype=torch.float64, device=dev)
        self._step = 0
        self._built = True

    def add_param_group(self, param_group):
        if self._built:
            raise ValueError("the parameters are fixed at construction: the arenas are laid out once")
        super().add_param_group(param_group)

    def _adopt_grads(self, refuse_none):
        """Every `param.grad` back on its view of the gradient arena: a replaced one is copied in, a missing one refused or zero."""
        for i, (p, view) in enumerate(zip(self._params, self._gviews)):
            g = p.grad
            if g is view:
                continue
            if g is None:
                if refuse_none:
                    raise ValueError(f"parameter {i} has no gradient (its .grad is None): every parameter of the arena is stepped; "
                                     "leave the zero view in place for one that got none")
                view.zero_()
            else:
                with torch.no_grad():
                    view.copy_(g)
            p.grad = view

    def zero_grad(self, set_to_none=False):
        """One fill of the gradient arena."""
        if set_to_none:
            raise ValueError("set_to_none=True would take the gradients off the arena that step() reads; zero_grad() is one fill instead")
        self._adopt_grads(refuse_none=False)
        self._g.zero_()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._adopt_grads(refuse_none=True)
        groups = [(float(g["lr"]), float(g["weight_decay"])) for g in self.param_groups]
        ops.optim_step(self._p, self._g, self._m, self._v, self._segs_host, self._segs_dev, len(self._rows), groups, self.kind,
                       momentum=self.momentum, nesterov=self.nesterov, betas=self.betas, eps=self.eps, step=self._step + 1,
                       decoupled=self.decoupled, clip_norm=self.clip_norm, max_change_global=self.max_change_global, stats=self.stats,
                       workspace=self._workspace)
        self._step += 1                                    # a refused call counts no step; one the guard skips does (no host sync)
        return loss

    def state_dict(self):
        """torch's dictionary (the groups' options) plus "ktf": the step count and copies of the state arenas."""
        sd = super().state_dict()
        sd["ktf"] = dict(kind=self.kind, step=self._step, layout=[(b, e) for b, e, _, _ in self._rows],
                         m=None if self._m is None else self._m.clone(), v=None if self._v is None else self._v.clone())
        return sd

    def load_state_dict(self, state_dict):
        ktf = state_dict.get("ktf")
        if ktf is None:
            raise ValueError("not a ktf.optim state_dict (no 'ktf' entry)")
        if ktf["kind"] != self.kind or [tuple(r) for r in ktf["layout"]] != [(b, e) for b, e, _, _ in self._rows]:
            raise ValueError("the state_dict was made for another kind or another set of parameters")
        for name, mine in (("m", self._m), ("v", self._v)):
            if (ktf[name] is None) != (mine is None):
                raise ValueError(f"the state_dict and this optimiser disagree on the state arena {name!r} (momentum 0 against non-zero?)")
        # the limits that act are those of the segment table, laid down at construction: a state_dict saved with others is refused
        saved, mine = [g.get("max_change") for g in state_dict["param_groups"]], [g["max_change"] for g in self.param_groups]
        if len(saved) != len(mine) or any(s is None or float(s) != float(m) for s, m in zip(saved, mine)):
            raise ValueError(f"the state_dict was saved with max_change {saved} per group, this optimiser was built with {mine}: "
                             "construct it with the saved limits")
        super().load_state_dict({"state": state_dict["state"], "param_groups": state_dict["param_groups"]})
        with torch.no_grad():
            for name, mine in (("m", self._m), ("v", self._v)):
                if mine is not None:
                    mine.copy_(ktf[name])
        self._step = int(ktf["step"])
