"""Auxiliary losses collected as a side effect of a policy forward.

Plugin-surface mirror of vlnce_baselines/common/aux_losses.py:4-44: the nets call
`AuxLosses.register_loss(name, per-row loss, alpha)` while the registry is active
(progress monitor, cma_policy.py:296-307 / seq2seq_policy.py:166-177) and the trainer
folds them into the objective with `AuxLosses.reduce(mask)` (base_il_trainer.py:163).
The reference keeps two parallel dicts; here one ordered table of (tensor, weight) entries,
a context manager for the activation window, and explicit errors instead of bare asserts.
"""
from collections import OrderedDict
from contextlib import contextmanager
from typing import NamedTuple

import torch


class _Entry(NamedTuple):
    values: torch.Tensor  # one loss value per batch row
    weight: float


class _PairEntry(NamedTuple):
    """the loss matrix (estimate [E] - target [R, 1]) ** 2, [R, E], kept as its two vectors"""
    estimate: torch.Tensor
    target: torch.Tensor
    weight: float

    @property
    def values(self):
        estimate, target = torch.broadcast_tensors(self.estimate, self.target)
        return (estimate - target) ** 2


class PairMSEFn(torch.autograd.Function):
    """mean((estimate [E] - target [R, 1]) ** 2 over the columns mask [E] selects) as ONE launch
    that also produces the gradient wrt the estimates (vlnce_pair_mse); the [R, E] matrix, its
    masked copy and their backward twins are never built.  The targets carry no gradient."""

    @staticmethod
    def forward(ctx, estimate, target, mask):
        from . import ops

        e = ops._f32c(estimate.detach()).reshape(-1)
        t = ops._f32c(target.detach()).reshape(-1)
        m = mask.reshape(-1).contiguous()
        assert m.numel() == e.numel(), "one mask entry per estimate"
        value = torch.empty((), device=e.device, dtype=torch.float32)
        d_estimate = torch.empty_like(e)
        ops.L().pair_mse(e, t, m, e.numel(), t.numel(), value, d_estimate)
        ctx.save_for_backward(d_estimate)
        ctx.shape = estimate.shape
        return value

    @staticmethod
    def backward(ctx, g):
        (d_estimate,) = ctx.saved_tensors
        return (d_estimate * g).view(ctx.shape), None, None


class AuxLossRegistry:
    def __init__(self):
        self._table = OrderedDict()
        self._collecting = False
        self._fusing = False
        self._dp = None  # (process group | None, world size) while data parallelism is declared

    # -- data parallelism ----------------------------------------------------------------
    def set_data_parallel(self, enabled=True, group=None):
        """Upstream reduces an auxiliary loss with a GLOBAL masked mean over the batch
        (aux_losses.py:24-32).  With the batch sharded over ranks and gradients averaged, the
        mean of per-rank masked means equals it only when every rank has the same number of
        unmasked rows.  Declaring data parallelism makes reduce() return
        world * local_sum / global_count (one tiny all-reduce of the counts), whose rank-average
        -- hence the averaged gradient -- is exactly the global masked mean.  Nets that build a
        loss from per-row targets of the WHOLE batch (the progress monitor's [B] x [B,1]
        broadcast, App. B-2) gather those targets through `gather_rows`."""
        if not enabled:
            self._dp = None
            return
        import torch.distributed as dist

        self._dp = (group, dist.get_world_size(group))

    def data_parallel(self):
        return self._dp is not None

    def gather_rows(self, t):
        """[b, ...] rows of this rank -> [B_global, ...] rows of all ranks (no gradient)."""
        if self._dp is None:
            return t
        import torch.distributed as dist

        parts = [torch.empty_like(t) for _ in range(self._dp[1])]
        dist.all_gather(parts, t.detach().contiguous(), group=self._dp[0])
        return torch.cat(parts, dim=0)

    # -- activation window -------------------------------------------------------------
    def activate(self):
        self._collecting = True

    def deactivate(self):
        self._collecting = False

    def is_active(self):
        return self._collecting

    @contextmanager
    def active(self):
        """`with AuxLosses.active(): ...` -- activate, and restore the previous state after."""
        was = self._collecting
        self._collecting = True
        try:
            yield self
        finally:
            self._collecting = was

    @contextmanager
    def fused(self):
        """`with AuxLosses.fused(): ...` -- while it is open, nets register a broadcast squared
        error as its two vectors (register_pair_loss) and reduce() sends such an entry through
        one launch (PairMSEFn).  Off by default: outside it every launch is the one made before."""
        was = self._fusing
        self._fusing = True
        try:
            yield self
        finally:
            self._fusing = was

    def is_fused(self):
        return self._fusing

    # -- table ---------------------------------------------------------------------------
    def clear(self):
        self._table = OrderedDict()

    def _register(self, name, entry):
        if not self._collecting:
            raise AssertionError("AuxLosses.register_loss() outside an activation window")
        if name in self._table:
            raise AssertionError(f"auxiliary loss '{name}' registered twice in one forward")
        self._table[name] = entry

    def register_loss(self, name, loss, alpha=1.0):
        self._register(name, _Entry(loss, alpha))

    def register_pair_loss(self, name, estimate, target, alpha=1.0):
        """the loss (estimate [E] - target [R, 1]) ** 2, [R, E] -- the progress monitor's
        F.mse_loss broadcast -- without materialising it: get_loss() builds the
        matrix on demand, reduce() needs it only where it cannot take the one-launch route."""
        if estimate.dim() != 1 or target.dim() != 2 or target.size(1) != 1:
            raise AssertionError("register_pair_loss: estimate [E] against target [R, 1]")
        self._register(name, _PairEntry(estimate, target, alpha))

    def get_loss(self, name):
        return self._table[name].values

    def names(self):
        return list(self._table)

    def reduce(self, mask):
        """sum_k alpha_k * mean(loss_k[mask]) -- a Python float 0.0 when nothing was registered,
        like upstream."""
        if not self._collecting:
            raise AssertionError("AuxLosses.reduce() outside an activation window")
        if self._dp is None:
            terms = [entry.weight * (PairMSEFn.apply(entry.estimate, entry.target, mask)
                                     if self._fusing and isinstance(entry, _PairEntry)
                                     and _library_takes(entry.estimate, entry.target, mask)
                                     else entry.values.masked_select(mask).mean())
                     for entry in self._table.values()]
            return sum(terms, 0.0)
        import torch.distributed as dist

        group, world = self._dp
        terms = []
        for entry in self._table.values():
            picked = entry.values.masked_select(mask)
            count = torch.tensor([float(picked.numel())], device=picked.device)
            dist.all_reduce(count, group=group)  # selected elements over all ranks
            terms.append(entry.weight * picked.sum() * (world / count[0]))
        return sum(terms, 0.0)


def _library_takes(*tensors):
    """the kernel library takes GPU tensors only (tests install a tensor-level simulator of it,
    which takes any)"""
    from . import _lib

    if all(t.is_cuda for t in tensors):
        return True
    return _lib._LIB is not None and not isinstance(_lib._LIB, _lib.HipLib)


AuxLosses = AuxLossRegistry()
