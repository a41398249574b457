"""The optimizer step on the device (ABI 152): `Adam` is `torch.optim.Adam` with `step()` done by
two launches per parameter group, `vlnce_grad_sumsq` (only with `max_grad_norm`) and
`vlnce_adam_step` (csrc/optim.hip), instead of torch's `multi_tensor_apply` chains for
`clip_grad_norm_` and Adam.  `state` / `state_dict()` have torch's layout (`step`, `exp_avg`,
`exp_avg_sq` per parameter), so a checkpoint of either class loads into the other; `lr` is read
from `param_groups` at every step (`LambdaLR` works); `zero_grad()` is the inherited one.

With `max_grad_norm` the step clips by the norm over ALL groups, as
`torch.nn.utils.clip_grad_norm_(all parameters, max_grad_norm)` in front of `step()` would, and
`optimizer.grad_norm` is the device scalar `clip_grad_norm_` returns; nothing is read back.  The
one observable difference: `.grad` is read only and stays unclipped.

The kernels write the parameters through raw pointers, which torch's version counters do not see,
and every derived weight image and captured-graph key of this package is built on those counters;
so `step()` ends by bumping `_version` of each parameter that took a step (the rule for any entry
point that writes a parameter through its pointer: `torch.autograd.graph.increment_version`).
"""
import math

import torch

from . import _lib

_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay")


class Adam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *,
                 max_grad_norm=None, **kwargs):
        for name in _REFUSED:
            if kwargs.pop(name, False):
                raise ValueError(f"vlnce_amd.optim.Adam: {name}=True is not supported")
        for name in ("foreach", "fused"):
            if kwargs.pop(name, None) is not None:
                raise ValueError(f"vlnce_amd.optim.Adam: an explicit {name}= is not supported "
                                 "(the step is this package's own kernels)")
        if kwargs:
            raise ValueError(f"vlnce_amd.optim.Adam: unknown arguments {sorted(kwargs)}")
        if any(isinstance(x, torch.Tensor) for x in (lr, *betas)):
            raise ValueError("vlnce_amd.optim.Adam: a tensor lr or beta is not supported")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"vlnce_amd.optim.Adam: max_grad_norm = {max_grad_norm}")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm = None    # device scalar of the last step (with max_grad_norm)
        self._tables = {}        # group index -> [AdamTable per launch]
        self._steps = {}         # group index -> (packed step counts, their views)
        self._partials = None
        self._check_groups()

    # ---- refusals
    def _check_groups(self):
        lib = _lib.get_lib()
        device = None
        for group in self.param_groups:
            for name in _REFUSED:
                if group.get(name):
                    raise ValueError(f"vlnce_amd.optim.Adam: {name}=True is not supported")
            for name in ("foreach", "fused"):
                if group.get(name) is not None:
                    raise ValueError(f"vlnce_amd.optim.Adam: an explicit {name}= is not supported")
            if any(isinstance(x, torch.Tensor) for x in (group["lr"], *group["betas"])):
                raise ValueError("vlnce_amd.optim.Adam: a tensor lr or beta is not supported")
            for p in group["params"]:
                if p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse:
                    raise ValueError("vlnce_amd.optim.Adam: parameters must be contiguous fp32 "
                                     f"(got {p.dtype}, strides {tuple(p.stride())})")
                if lib.name == "hip" and not p.is_cuda:   # (a host simulator runs on the CPU)
                    raise ValueError("vlnce_amd.optim.Adam: parameters must live on a GPU")
                device = device or p.device
                if p.device != device:
                    raise ValueError("vlnce_amd.optim.Adam: parameters on more than one device "
                                     f"({device}, {p.device})")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_tables"):
            self._check_groups()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            # how the WRITER ran its step (torch's foreach / fused / capturable kernels) is not a
            # setting of the arithmetic: a checkpoint of such an optimizer loads
            group["foreach"] = group["fused"] = None
            group["capturable"] = False
        self._tables, self._steps = {}, {}
        self._check_groups()

    # ---- the step
    def _collect(self, index, group):
        """tensors of the group that have state after this step saw their gradients:
        (params, exp_avg, exp_avg_sq, grads or None, step_size, inv_bc2_sqrt)"""
        b1, b2 = group["betas"]
        lr = float(group["lr"])
        ps, ms, vs, gs, ss, cs = [], [], [], [], [], []
        steps, where = [], []
        device = group["params"][0].get_device() if group["params"] else -1
        for p in group["params"]:
            g = p.grad
            if g is None:
                state = self.state.get(p)
                if not state:
                    continue    # never saw a gradient: no state, as torch
            else:
                if g.is_sparse:
                    raise ValueError("vlnce_amd.optim.Adam does not support sparse gradients")
                if g.dtype != torch.float32 or g.get_device() != device:
                    raise ValueError("vlnce_amd.optim.Adam: gradients must be fp32 on the "
                                     f"parameter's device (got {g.dtype} on {g.device})")
                if not g.is_contiguous():
                    g = g.contiguous()
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                steps.append(state["step"]), where.append(len(ps))
            ps.append(p), ms.append(state["exp_avg"]), vs.append(state["exp_avg_sq"])
            gs.append(g), ss.append(0.0), cs.append(0.0)
        if steps:
            # The counts of the tensors that take a step together are 0-dim views of ONE host
            # tensor (each still its own `step` entry, torch's layout): one add and one read per
            # step instead of one of each per tensor.  Packed again when the set changes, after
            # load_state_dict() (a plain number, or a device tensor as a fused / capturable
            # optimizer writes it: one read-back, once per load), or when an entry was replaced.
            packed = self._steps.get(index)
            if packed is not None and len(packed[1]) == len(steps) \
                    and all(a is b for a, b in zip(packed[1], steps)):
                pack = packed[0]
                pack += 1
            else:
                pack = torch.tensor([float(s) for s in steps], dtype=torch.float32) + 1
                views = list(pack.unbind(0))
                for i, view in zip(where, views):
                    self.state[ps[i]]["step"] = view
                self._steps[index] = (pack, views)
            memo = {}
            for i, t in zip(where, pack.tolist()):
                if t not in memo:
                    memo[t] = (lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t))
                ss[i], cs[i] = memo[t]
        return ps, ms, vs, gs, ss, cs

    def _group_tables(self, index, lib, ps, ms, vs):
        """the group's launches: one table per adam_max_tensors() tensors, rebuilt when a pointer
        (or the set of tensors with state) changes"""
        limit = lib.adam_max_tensors()
        tables = self._tables.get(index)
        key = []
        for p, m, v in zip(ps, ms, vs):
            key += [p.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()]
        if tables is None or [w for tab in tables for w in tab.key] != key:
            tables = [lib.adam_table(ps[i:i + limit], ms[i:i + limit], vs[i:i + limit])
                      for i in range(0, len(ps), limit)]
            self._tables[index] = tables
        return tables

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.get_lib()
        limit = lib.adam_max_tensors()
        work = []
        for index, group in enumerate(self.param_groups):
            ps, ms, vs, gs, ss, cs = self._collect(index, group)
            if not ps:
                continue
            tables = self._group_tables(index, lib, ps, ms, vs)
            for k, tab in enumerate(tables):
                sl = slice(k * limit, (k + 1) * limit)
                if any(g is not None for g in gs[sl]):
                    work.append((group, tab, gs[sl], ss[sl], cs[sl]))
        if not work:
            return loss
        partials = norm = None
        if self.max_grad_norm is not None:
            device = work[0][1].ps[0].device
            if self._partials is None or self._partials.device != device:
                self._partials = torch.empty(_lib.ADAM_PARTIALS, dtype=torch.float64, device=device)
            partials = self._partials   # (re-used: the launches of two steps are stream-ordered)
            norm = torch.empty((), dtype=torch.float32, device=device)   # the caller may keep it
            for k, (_, tab, gs, _, _) in enumerate(work):
                lib.grad_sumsq(tab, gs, partials, k > 0)
        for group, tab, gs, ss, cs in work:
            b1, b2 = group["betas"]
            lib.adam_step(tab, gs, ss, cs, partials, self.max_grad_norm, b1, b2, group["eps"],
                          group["weight_decay"], norm)
        if norm is not None:
            self.grad_norm = norm
        # vlnce_adam_step wrote these parameters through their pointers: tell torch (one host call,
        # no launch), or the weight images and graphs keyed on the old versions stay in use
        torch.autograd.graph.increment_version(
            [p for _, tab, gs, _, _ in work for p, g in zip(tab.ps, gs) if g is not None])
        return loss
