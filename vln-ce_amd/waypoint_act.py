"""WaypointPolicy.act behind the net as ONE HIP launch (vlnce_waypoint_act, csrc/waypoint_act.hip), and
the DD-PPO trainer's pick of the observation history as one more (vlnce_waypoint_history_pick),
instead of three torch distribution objects whose constructors, log_prob and rejection sampling each
end in a host synchronisation, and a Python loop over the environments.  Opt-in
(WaypointPolicy.fused_act / the "waypoint_act" option).  The randomness of a sampled action is ONE
torch.rand on the policy's device, handed to the kernel: reproducible under torch.manual_seed.
"""
import collections

import torch

from . import _lib, ops
from ._lib import WP_ABSENT, WP_CONTINUOUS, WP_DISCRETE, WaypointActPart, WaypointPart

# what one launch leaves on the device; host_rows [B, 8] is the one buffer act() reads back:
# stop, r, theta, stored distance in metres, stored offset in radians, distance / offset variance, flags
ActResult = collections.namedtuple(
    "ActResult", "pano elements modes variances log_prob norm_logits host_rows flags")
ROW_STOP, ROW_R, ROW_THETA, ROW_DISTANCE, ROW_OFFSET, ROW_DISTANCE_VAR, ROW_OFFSET_VAR, ROW_FLAGS = range(8)


def launch(logits, o_first, o_second, d_first, d_second, spec, extras, deterministic, u=None):
    """logits [B, P+1] RAW; the heads' outputs as WaypointEvalFn takes them; spec = (P, {part: (kind, K,
    lo, hi, weight)}) of policy._eval_spec(); extras = {part: (bin_lo, bin_hi, off_metric,
    off_element)}; u [B, 3] fp32 uniforms in [0, 1) (made here when None and not deterministic).
    Returns an ActResult in the reference's shapes: [B, 1] throughout, a discrete part's variance [B]."""
    P, kinds = spec
    B = logits.shape[0]
    dev = logits.device
    logits = ops._f32c(logits.detach())
    if not deterministic and u is None:
        u = torch.rand((B, 3), device=dev, dtype=torch.float32)
    f32 = torch.empty(B * (P + 2 + _lib.WP_ACT_ROW + 6), device=dev, dtype=torch.float32)
    i64 = torch.empty(B * 5, device=dev, dtype=torch.int64)
    flags = torch.empty(B, device=dev, dtype=torch.int32)
    fs = list(f32.split([B, B * (P + 1), B * _lib.WP_ACT_ROW] + [B] * 6))
    log_prob, norm_logits, host_rows = fs[:3]
    pano, *ints = i64.split(B)
    parts, outs = [], []
    elements, modes, variances = {}, {}, {}
    for k, (name, first, second) in enumerate((("offset", o_first, o_second),
                                               ("distance", d_first, d_second))):
        kind, K, lo, hi, weight = kinds[name]
        bin_lo, bin_hi, off_metric, off_element = extras[name]
        if kind == WP_ABSENT:
            parts.append(WaypointPart(kind, 0, 0.0, 0.0, 0.0, None, None, None))
            outs.append(WaypointActPart(0.0, 0.0, off_metric, off_element, None, None, None))
            continue
        cont = kind == WP_CONTINUOUS
        element, mode = (fs[3 + 3 * k], fs[4 + 3 * k]) if cont else (ints[2 * k], ints[2 * k + 1])
        variance = fs[5 + 3 * k]
        parts.append(WaypointPart(kind, K, lo, hi, weight, ops._f32c(first.detach()),
                                  ops._f32c(second.detach()) if cont else None, None))
        outs.append(WaypointActPart(bin_lo, bin_hi, off_metric, off_element, element, mode, variance))
        elements[name], modes[name] = element.view(B, 1), mode.view(B, 1)
        # (Categorical.variance is [B]; TruncatedNormal's has the shape of loc)
        variances[name] = variance.view(B, 1) if cont else variance
    ops.L().waypoint_act(logits, parts[0], parts[1], outs[0], outs[1], deterministic, u, B, P, pano,
                         log_prob, norm_logits, host_rows, flags)
    return ActResult(pano.view(B, 1), elements, modes, variances, log_prob.view(B, 1),
                     norm_logits.view(B, P + 1), host_rows.view(B, _lib.WP_ACT_ROW), flags)


def flag_errors(bits, windows):
    """the reference's assertion for the flag bits of an act() batch (their OR), in the order the
    torch path meets them: the panorama logits, then per component (distance first) the constructor's
    checks.  windows: {part: (smin, smax)}.  None when no bit is set."""
    if bits & _lib.WP_FLAG_PANO:
        return "panorama logits are not finite"
    for part in ("distance", "offset"):
        b = bits >> _lib.WP_FLAG_SHIFT[part]
        smin, smax = windows[part]
        if b & _lib.WP_FLAG_LOC:
            return f"loc is out of range ({smin}, {smax})"
        if b & _lib.WP_FLAG_VARIANCE:
            return "scale is negative"
    return None


def history_pick(frames, pano):
    """{sensor: [B, P, ...] (fp32 or uint8; a slice of a rollout arena is fine)} and the panorama
    choice [B, 1] int64 ON THE DEVICE -> {sensor: [B, ...]}: the chosen frame, zeros for a STOP row.
    One launch for all sensors, no read-back."""
    names = list(frames)
    B, P = frames[names[0]].shape[:2]
    outs = {k: torch.empty((B,) + tuple(v.shape[2:]), device=v.device, dtype=v.dtype)
            for k, v in frames.items()}
    ops.L().waypoint_history_pick([(frames[k], outs[k]) for k in names],
                                  pano.reshape(-1).contiguous(), B, P)
    return outs


def feature_pick(features, zeros, pano):
    """{sensor: [B, P, ...] fp32 trunk outputs (a slice of a rollout arena is fine)}, {sensor: [...]
    trunk(zero frame)} and the panorama choice [B, 1] int64 ON THE DEVICE -> {sensor +
    "_history_features": [B, ...]}: the chosen slot's features, `zeros[sensor]` for a STOP row.  One
    launch for all sensors (vlnce_waypoint_feature_pick), no read-back."""
    names = list(features)
    B, P = features[names[0]].shape[:2]
    outs = {k: torch.empty((B,) + tuple(v.shape[2:]), device=v.device, dtype=torch.float32)
            for k, v in features.items()}
    ops.L().waypoint_feature_pick([(features[k], zeros[k], outs[k]) for k in names],
                                  pano.reshape(-1).contiguous(), B, P)
    return {k + "_history_features": v for k, v in outs.items()}


__all__ = ["ActResult", "WP_ABSENT", "WP_CONTINUOUS", "WP_DISCRETE", "feature_pick", "flag_errors",
           "history_pick", "launch"]
