"""The distribution arithmetic of WaypointPolicy.evaluate_actions as one HIP launch forward and one
backward (vlnce_waypoint_eval / _bwd, csrc/waypoint_dist.hip) instead of the host-paced chain of
small torch launches behind CustomFixedCategorical and TruncatedNormal, whose constructors and
log_prob each end in a host synchronisation.  Opt-in (WaypointPolicy.fused_distributions); the
reference's assertions become flag bits that policy.check_eval_flags() reads back on demand.
"""
import torch

from . import _lib, ops
from ._lib import WP_ABSENT, WP_CONTINUOUS, WP_DISCRETE, WaypointPart, WaypointPartGrad

PARTS = ("offset", "distance")   # the order of the C entry points' descriptors and entropy blocks


class WaypointEvalFn(torch.autograd.Function):
    """forward(logits [B, P+1], offset first / second, distance first / second, pano [B] int64,
    offset element [B], distance element [B], spec) -> (log_prob [B, 1], pano / offset / distance
    entropy, flags [B] int32).  The entropies are [B]; a DISCRETE part's is the reference's [B, B]
    broadcast of its [B, 1] weight over the categorical's [B] entropy (B > 1).  spec = (P, {part:
    (kind, K, lo, hi, weight)}); `second` is None for a part that is not continuous.  One launch each way, no host synchronisation, and no
    zero-fill: the backward launch writes the dense gradients."""

    @staticmethod
    def forward(ctx, logits, o_first, o_second, d_first, d_second, pano, o_elem, d_elem, spec):
        P, kinds = spec
        B = pano.numel()
        dev = logits.device
        logits = ops._f32c(logits.detach())
        pano = pano.detach().reshape(-1).to(torch.int64).contiguous()
        parts = []
        for name, first, second, elem in (("offset", o_first, o_second, o_elem),
                                          ("distance", d_first, d_second, d_elem)):
            kind, K, lo, hi, weight = kinds[name]
            if kind == WP_ABSENT:
                parts.append(WaypointPart(kind, 0, 0.0, 0.0, 0.0, None, None, None))
                continue
            elem = elem.detach().reshape(-1).to(torch.float32 if kind == WP_CONTINUOUS
                                                else torch.int64).contiguous()
            parts.append(WaypointPart(kind, K, lo, hi, weight, ops._f32c(first.detach()),
                                      ops._f32c(second.detach()) if kind == WP_CONTINUOUS else None,
                                      elem))
        sizes = [B, B] + [_lib.waypoint_entropy_floats(B, p) for p in parts]
        out = torch.empty(sum(sizes), device=dev, dtype=torch.float32)
        saved = torch.empty((_lib.waypoint_saved_planes(P, parts), B), device=dev,
                            dtype=torch.float32)
        flags = torch.empty(B, device=dev, dtype=torch.int32)
        ops.L().waypoint_eval(logits, pano, parts[0], parts[1], B, P, out, saved, flags)
        ctx.save_for_backward(pano, saved, flags)
        ctx.geometry = (B, P, [(p.kind, p.K, p.weight) for p in parts],
                        [None if p.first is None else p.first.shape for p in parts])
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(flags)
        logp, ent_pano, ent_o, ent_d = out.split(sizes)
        if B > 1:   # (weight [B, 1] * entropy [B]).squeeze(1), as the torch path shapes it
            ent_o, ent_d = (e.view(B, B) if e.numel() == B * B else e for e in (ent_o, ent_d))
        return logp.view(B, 1), ent_pano, ent_o, ent_d, flags

    @staticmethod
    def backward(ctx, g_logp, g_pano, g_offset, g_distance, _g_flags):
        pano, saved, flags = ctx.saved_tensors
        B, P, kinds, shapes = ctx.geometry
        dev = saved.device
        grads = [None if g is None else ops._f32c(g).reshape(-1)
                 for g in (g_logp, g_pano, g_offset, g_distance)]
        d_logits = torch.empty((B, P + 1), device=dev, dtype=torch.float32)
        part_grads = []
        for (kind, K, weight), shape in zip(kinds, shapes):
            part_grads.append(WaypointPartGrad(
                kind, K, weight,
                None if kind == WP_ABSENT else torch.empty(shape, device=dev, dtype=torch.float32),
                torch.empty((B, P), device=dev, dtype=torch.float32) if kind == WP_CONTINUOUS
                else None))
        ops.L().waypoint_eval_bwd(grads, pano, saved, flags, part_grads[0], part_grads[1], B, P,
                                  d_logits)
        (o, d) = part_grads
        return d_logits, o.d_first, o.d_second, d.d_first, d.d_second, None, None, None, None


def flag_errors(bits, windows):
    """the reference's assertion for the flag bits of a batch (their OR), in the order the torch path
    meets them: the panorama choice, then per component (distance first) the constructor's checks
    and log_prob's.  windows: {part: (smin, smax)}.  None when no bit is set."""
    if bits & _lib.WP_FLAG_PANO:
        return "pano index is outside [0, num_panos]"
    for part in ("distance", "offset"):
        b = bits >> _lib.WP_FLAG_SHIFT[part]
        smin, smax = windows[part]
        if b & _lib.WP_FLAG_LOC:
            return f"loc is out of range ({smin}, {smax})"
        if b & _lib.WP_FLAG_VARIANCE:
            return "scale is negative"
        if b & _lib.WP_FLAG_ELEMENT:
            return "value is out of truncation range and has an undefined log_prob."
        if b & _lib.WP_FLAG_CLASS:
            return f"{part} class index is outside the head's classes"
    return None


__all__ = ["PARTS", "WP_ABSENT", "WP_CONTINUOUS", "WP_DISCRETE", "WaypointEvalFn", "flag_errors"]
