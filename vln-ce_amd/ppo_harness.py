"""Waypoint DD-PPO inner step: one minibatch of `WDDPPO.update`
(vlnce_baselines/common/ddppo_alg.py:53-141) for callers that run without habitat
(tests, benchmarks).  `ddppo_waypoint_trainer.py` drives the same math through
habitat's DDPPO class and only needs the policy's evaluate_actions() from this package.

`sample` is the 9-tuple `RolloutStorage.recurrent_generator` yields:
(observations, recurrent_hidden_states, actions{pano,offset,distance}, prev_actions,
 value_preds, returns, masks, old_action_log_probs, advantages), rows time-major (t*N + n).
"""
from dataclasses import dataclass

import torch


@dataclass
class PPOConfig:  # RL.PPO defaults, vlnce_baselines/config/default.py:180-201
    clip_param: float = 0.2
    value_loss_coef: float = 0.5
    entropy_coef: float = 0.01
    pano_entropy_coef: float = 1.0
    offset_entropy_coef: float = 0.0
    distance_entropy_coef: float = 0.0
    offset_regularize_coef: float = 0.1146
    use_clipped_value_loss: bool = True
    max_grad_norm: float = 0.2


def normalized_advantages(returns, value_preds, normalize=False, eps=1e-5):
    """WDDPPO.get_advantages (ddppo_alg.py:31-36); inputs carry the bootstrap row."""
    adv = returns[:-1] - value_preds[:-1]
    return (adv - adv.mean()) / (adv.std() + eps) if normalize else adv


def compute_returns(rewards, value_preds, masks, next_value, gamma, tau, use_gae=True):
    """RolloutStorage.compute_returns (rollout_storage.py:127-152) on the device, one launch.
    rewards [T,N,1]; value_preds, masks [T+1,N,1] (value_preds[T] is overwritten with next_value
    under GAE, as upstream); next_value [N,1].  Returns `returns` [T+1,N,1]."""
    from . import ops

    T, N = rewards.shape[0], rewards.shape[1]
    rewards, masks = rewards.contiguous().float(), masks.contiguous().float()
    assert value_preds.is_contiguous() and value_preds.dtype == torch.float32
    returns = torch.zeros_like(value_preds)
    ops.L().ppo_returns(rewards, value_preds, masks, next_value.contiguous().float(), returns, T, N,
                        gamma, tau, use_gae)
    return returns


class PPOLossFn(torch.autograd.Function):
    """The WDDPPO minibatch loss (ddppo_alg.py:78-121) as ONE launch that also produces every
    gradient (vlnce_ppo_loss), instead of ~40 elementwise / reduction launches forward and as many
    backward, all host-paced.  forward(values, logp, ent_pano, ent_offset, ent_distance,
    value_preds, returns, old_logp, adv, radians | None, cfg) -> (loss [], stats [8] = loss,
    value_loss, action_loss, entropy_loss, mean pano / offset / distance entropy, offset_loss)."""

    @staticmethod
    def forward(ctx, values, logp, ent_p, ent_o, ent_d, value_preds, returns, old_logp, adv, radians,
                cfg):
        from . import ops

        B = values.numel()
        flat = [ops._f32c(t.detach()).reshape(-1) if t is not None else None
                for t in (values, returns, value_preds, logp, old_logp, adv, ent_p, ent_o, ent_d,
                          radians)]
        assert all(t is None or t.numel() == B for t in flat), "one value per rollout row"
        stats = torch.empty(8, device=values.device, dtype=torch.float32)
        grads = torch.empty((5, B), device=values.device, dtype=torch.float32)
        ops.L().ppo_loss(*flat, B, cfg.clip_param, cfg.value_loss_coef, cfg.entropy_coef,
                         cfg.pano_entropy_coef, cfg.offset_entropy_coef, cfg.distance_entropy_coef,
                         cfg.offset_regularize_coef, cfg.use_clipped_value_loss, stats, grads)
        ctx.save_for_backward(grads)
        ctx.shapes = tuple(t.shape for t in (values, logp, ent_p, ent_o, ent_d))
        loss = stats[0].clone()
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, g_loss, _g_stats):
        (grads,) = ctx.saved_tensors
        g = grads * g_loss
        out = [g[k].view(shape) for k, shape in enumerate(ctx.shapes)]
        return (*out, None, None, None, None, None, None)


SENSORS = ("rgb", "depth")


def _step_observation(policy, rollouts):
    """rollouts.observations at rollouts.step as the net takes them, and what to do after the forward.
    For a storage with trunk-feature arenas (ActionDictRolloutStorage(trunk_features=...)): the stored
    history features always stand in for the history frames; the stored panorama features stand in
    for the panorama frames when the row holds them under the net's current trunk_cache_key() (row 0
    after after_update); otherwise the forward runs the trunks on the panorama and `store()` writes
    their outputs into the row."""
    step = rollouts.step
    observation = {k: v[step] for k, v in rollouts.observations.items()}
    if not getattr(rollouts, "has_trunk_features", False):
        return observation, lambda: None
    net = policy.net
    key = net.trunk_cache_key()
    if rollouts.trunk_key != key:
        # nothing made under another key is used: the row's history features are made again
        if rollouts.trunk_key is not None:
            for s in SENSORS:
                observation[s + "_history_features"].copy_(net._trunk_rows(s, observation[s + "_history"]))
        rollouts.trunk_valid = [False] * len(rollouts.trunk_valid)
        rollouts.trunk_key = key
    observation["trunk_feature_key"] = key
    if rollouts.trunk_valid[step]:
        return observation, lambda: None
    arenas = {s: observation.pop(s + "_features") for s in SENSORS}

    def store():
        for s in SENSORS:
            arenas[s].copy_(net.last_trunk_features[s])
        rollouts.trunk_valid[step] = True

    return observation, store


def bootstrap_value(policy, rollouts):
    """The value of the row behind the last collected step (ddppo_waypoint_trainer.py:287-299), for
    compute_returns.  With trunk-feature arenas the row's panorama features are stored on the way, so
    that row 0 of the next rollout, where after_update carries them, needs no trunk."""
    step = rollouts.step
    observation, store = _step_observation(policy, rollouts)
    prev_actions = {k: v[step] for k, v in rollouts.prev_actions.items()}
    with torch.no_grad():
        value = policy.get_value(observation, rollouts.recurrent_hidden_states[step], prev_actions,
                                 rollouts.masks[step]).detach()
    store()
    return value


def act_for_rollout(policy, rollouts, deterministic=False):
    """The action half of `_collect_rollout_step` (ddppo_waypoint_trainer.py:160-220) over any storage
    with the arenas (vlnce_amd.ActionDictRolloutStorage, or the reference's own class): slices the
    arenas at rollouts.step, calls policy.act, picks each environment's chosen panorama frame as the
    next step's rgb / depth history (zeros for STOP) and collects the logging predictions of the
    environments that go on.  Returns (act()'s 8-tuple, {"rgb", "depth"} history, logging_predictions).

    When act() took its one-launch path (policy.fused_act / the "waypoint_act" option) the history is
    ONE launch that reads the choice on the device, and the predictions come from the host rows act()
    already read back: no second synchronisation.  Otherwise this is the reference's loop.

    Over a storage with trunk-feature arenas (see _step_observation) the history gains
    "rgb_history_features" / "depth_history_features": the chosen panorama slot's trunk output, or
    trunk(zero frame) for STOP, from ONE launch that reads the choice on the device -- with either
    act() path.  Put into the batch under those names beside `rgb_history` / `depth_history`
    (ddppo_waypoint_trainer.py:237-238), `rollouts.insert(batch, ...)` stores them at step + 1 with
    everything else."""
    from . import waypoint_act

    step = rollouts.step
    observation, store = _step_observation(policy, rollouts)
    prev_actions = {k: v[step] for k, v in rollouts.prev_actions.items()}
    with torch.no_grad():
        outputs = policy.act(observation, rollouts.recurrent_hidden_states[step], prev_actions,
                             rollouts.masks[step], deterministic=deterministic)
    _, actions, elements, _, variances, _, _, _ = outputs
    store()
    frames = {k: observation[k] for k in ("rgb", "depth")}
    feature_history = {}
    if "trunk_feature_key" in observation:
        feats = {s: rollouts.observations[s + "_features"][step] for s in SENSORS}
        zeros = {s: policy.net.trunk_zero(s, frames[s].shape[-3:], frames[s].device,
                                          observation["trunk_feature_key"]) for s in SENSORS}
        feature_history = waypoint_act.feature_pick(feats, zeros, elements["pano"])
    predictions = {k: [] for k in ("distance_pred", "offset_pred", "distance_var", "offset_var")}
    rows = getattr(policy, "last_act_rows", None)
    if rows is not None:
        history = waypoint_act.history_pick(frames, elements["pano"])
        for row in rows:
            if not row[waypoint_act.ROW_STOP]:
                predictions["distance_pred"].append(row[waypoint_act.ROW_DISTANCE])
                predictions["offset_pred"].append(row[waypoint_act.ROW_OFFSET])
                predictions["distance_var"].append(row[waypoint_act.ROW_DISTANCE_VAR])
                predictions["offset_var"].append(row[waypoint_act.ROW_OFFSET_VAR])
        history.update(feature_history)
        return outputs, history, predictions
    history = {k: torch.zeros_like(v[:, 0]) for k, v in frames.items()}
    for i, action in enumerate(actions):
        if action["action"] == "STOP":
            continue
        idx = elements["pano"][i]
        for k, v in frames.items():
            history[k][i] = v[i, idx]
        for part, to_metric in (("distance", policy.net.distance_to_continuous),
                                ("offset", policy.net.offset_to_continuous)):
            predictions[part + "_pred"].append(to_metric(elements[part][i]).item())
            var = variances[part]
            predictions[part + "_var"].append(var[i].item() if type(var) is torch.Tensor else var)
    history.update(feature_history)
    return outputs, history, predictions


def _clips_itself(optimizer):
    """vlnce_amd.optim.Adam(max_grad_norm=...) clips inside its own step (one norm launch)"""
    from .optim import Adam

    return isinstance(optimizer, Adam) and optimizer.max_grad_norm is not None


def wddppo_minibatch_update(policy, optimizer, sample, cfg=PPOConfig(), *, step_grad=True,
                            clip_grads=True, grad_hook=None):
    (obs, h0, actions, prev_actions, value_preds, returns, masks, old_logp, adv) = sample
    values, logp, entropy, _ = policy.evaluate_actions(obs, h0, prev_actions, masks, actions)
    # keep predicted headings near the pano centre (a constant: sampled offsets carry no gradient)
    radians = policy.net.offset_to_continuous(actions["offset"]) if "offset" in actions else None
    loss, stats = PPOLossFn.apply(values, logp, entropy["pano"], entropy["offset"],
                                  entropy["distance"], value_preds, returns, old_logp, adv, radians,
                                  cfg)

    if optimizer is not None:
        optimizer.zero_grad()
    loss.backward()
    if grad_hook is not None:
        grad_hook()  # data-parallel gradient all-reduce (vlnce_amd.distributed)
    if clip_grads and cfg.max_grad_norm is not None and not (step_grad and _clips_itself(optimizer)):
        torch.nn.utils.clip_grad_norm_(policy.parameters(), cfg.max_grad_norm)
    if step_grad and optimizer is not None:
        optimizer.step()
    # (value_loss, action_loss, entropy_loss, pano / offset / distance entropy) as WDDPPO.update sums
    return tuple(stats[1:7].unbind(0))


def _trunk_cache_usable(policy, rollouts):
    """None when the update can run from the storage's trunk features, else why not (an exception)"""
    if not getattr(rollouts, "has_trunk_features", False):
        return RuntimeError("trunk-feature cache: the storage has no feature arenas "
                            "(ActionDictRolloutStorage(trunk_features=...))")
    missing = [r for r in range(rollouts.step) if not rollouts.trunk_valid[r]]
    if missing or rollouts.trunk_key is None:
        return RuntimeError(f"trunk-feature cache: rows {missing} of the storage hold no trunk features "
                            "(collect with act_for_rollout / bootstrap_value)")
    try:
        now = policy.net.trunk_cache_key()
        for s in SENSORS:
            policy.net.check_trunk_cache(s, rollouts.trunk_key, now)
    except RuntimeError as e:
        return e
    return None


def wddppo_update(policy, optimizer, rollouts, cfg=PPOConfig(), *, ppo_epoch=2, num_mini_batch=4,
                  use_normalized_advantage=False, grad_hook=None, use_trunk_cache=None):
    """WDDPPO.update (ddppo_alg.py:37-149) over any storage that has `recurrent_generator` and the
    arenas (vlnce_amd.ActionDictRolloutStorage, or the reference's own class): `ppo_epoch` passes of
    `num_mini_batch` minibatches, each through wddppo_minibatch_update.  The six statistics
    accumulate on the device and are read back ONCE, at the end (the reference calls .item() six
    times per minibatch); returns their means over the ppo_epoch * num_mini_batch updates:
    (value_loss, action_loss, entropy_loss, pano / offset / distance entropy).

    use_trunk_cache: None = run the minibatches from the storage's trunk features (no frame is
    gathered, no trunk runs) when it has them for every collected row under the net's current
    trunk_cache_key(), else from the frames; True = raise instead of falling back; False = frames."""
    cached = False
    if use_trunk_cache or use_trunk_cache is None:
        why_not = _trunk_cache_usable(policy, rollouts)
        if why_not is not None and use_trunk_cache:
            raise why_not
        cached = why_not is None
    if hasattr(rollouts, "get_advantages"):
        advantages = rollouts.get_advantages(use_normalized_advantage)
    else:
        advantages = normalized_advantages(rollouts.returns, rollouts.value_preds,
                                           use_normalized_advantage)
    totals = None
    for _e in range(ppo_epoch):
        for sample in (rollouts.recurrent_generator(advantages, num_mini_batch, frames=False) if cached
                       else rollouts.recurrent_generator(advantages, num_mini_batch)):
            if cached:
                sample[0]["trunk_feature_key"] = rollouts.trunk_key
            elif getattr(rollouts, "has_trunk_features", False):   # the frame path takes no stored feature
                for k in [k for k in sample[0] if k.endswith("_features") and k != "angle_features"]:
                    del sample[0][k]
            stats = torch.stack(wddppo_minibatch_update(policy, optimizer, sample, cfg,
                                                        grad_hook=grad_hook))
            totals = stats if totals is None else totals + stats
    num_updates = ppo_epoch * num_mini_batch
    return tuple(v / num_updates for v in totals.tolist())
