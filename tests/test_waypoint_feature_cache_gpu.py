"""GPU tier: the trunk-feature cache of the Waypoint DD-PPO loop through the net, the storage and the
harness on the MI355X.  A trunk output taken once per frame -- in another batch, by other kernel
instances than the 13-frames-per-environment batch of the frame path -- must give the encoder rows,
the reference's PPO fixtures and the update the frame path gives; what the cache moves, it moves bit
for bit.  Tolerances are the ones the frame path is held to (tests/test_policy_gpu.py)."""
import os

import pytest
import torch

import cases
import rollout_cases as rc
import waypoint_features_ref as wf
from test_oracle_golden import compare
from vlnce_amd import ppo_harness
from vlnce_amd.optim import Adam
from vlnce_amd.ppo_harness import PPOConfig, wddppo_minibatch_update, wddppo_update
from vlnce_amd.rollout_storage import FRAME_KEYS, ActionDictRolloutStorage

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
torch.distributions.Distribution.set_default_validate_args(False)


def to_dev(x):
    if isinstance(x, dict):
        return {k: to_dev(v) for k, v in x.items()}
    return x.to(DEV) if isinstance(x, torch.Tensor) else x


def features_of(net, obs, envs_per_call):
    """the four feature keys from separate trunk calls: the panorama frames alone, `envs_per_call`
    environments at a time, and the history frames alone, unmasked"""
    feats = {}
    B = obs["rgb"].shape[0]
    for s in wf.SENSORS:
        for key, frames in ((s + "_features", obs[s]), (s + "_history_features", obs[s + "_history"])):
            feats[key] = torch.cat([net._trunk_rows(s, frames[i:i + envs_per_call])
                                    for i in range(0, B, envs_per_call)])
    return feats


def test_encoder_rows_from_features_equal_the_rows_from_frames():
    """_encode_frames the old way against the rows assembled from features, 1e-4 absolute after scaling
    each tensor to unit maximum (north_star); a misplaced slot or a missing mask is an error of
    order one.  Rows 0, 1 and 4 have masks == 0; row 3's history is the zero frame of a STOP."""
    name = "waypoint_ppo_update_64"
    obs, _, masks, _, _ = cases.load_case(os.path.join(wf.GOLD, name + ".npz"))
    obs, masks = to_dev(obs), masks.to(DEV)
    assert masks.reshape(-1).tolist() == [0, 0, 1, 1, 0, 1]
    for s in wf.SENSORS:
        obs[s + "_history"][3] = 0
    net = wf.build_policy(DEV, name).net
    with torch.no_grad():
        old = {s: net._encode_frames(net._sensor_encoder(s), s, obs[s], obs[s + "_history"], masks)
               for s in wf.SENSORS}
        cached = dict(obs)
        cached.update(features_of(net, obs, envs_per_call=6))
        for k in FRAME_KEYS:
            del cached[k]
        for mask in (masks, masks.float()):      # uint8 as the storage holds it, fp32 as the net does
            new = net._encode_cached(list(wf.SENSORS), cached, mask)
            for s in wf.SENSORS:
                for what, a, b in zip(("panorama", "history"), old[s], new[s]):
                    assert a.shape == b.shape, (s, what)
                    scale = float(a.abs().max())
                    err = float((a - b).abs().max()) / scale
                    print(f"{s} {what} rows: max|d| / max|x| = {err:.3e}")
                    assert err <= 1e-4, (s, what, err)
        zero = net.trunk_zero("rgb", obs["rgb"].shape[-3:], DEV)
        assert float((cached["rgb_history_features"][3] - zero).abs().max()) <= 1e-4 * float(zero.abs().max())


def cache_ppo(policy, sample):
    with wf.TrunkCounter(policy.net) as counter:
        stats = wddppo_minibatch_update(policy, None, sample, PPOConfig(**cases.PPO), step_grad=False,
                                        clip_grads=False)
    assert counter.calls == 0      # no trunk inside the update
    return [float(v) for v in stats]


def golden_through_the_cache(name, envs_per_call):
    case = cases.CASES[name]
    obs, prev, masks, extra, gold = cases.load_case(os.path.join(wf.GOLD, name + ".npz"))
    policy = wf.build_policy(DEV, name)
    obs = to_dev(obs)
    with torch.no_grad():
        feats = features_of(policy.net, obs, envs_per_call)
        for s in wf.SENSORS:
            policy.net.trunk_zero(s, obs[s].shape[-3:], DEV)
    cached = {k: v for k, v in obs.items() if k not in FRAME_KEYS}
    cached.update(feats)
    assert not set(cached) & set(FRAME_KEYS)
    del obs
    outs = cases.run_case(policy, case, cached, to_dev(prev), to_dev(masks), to_dev(extra), None, None,
                          ppo_fn=cache_ppo)
    compare(outs, gold, atol=1e-4, rtol=1e-4)


def test_reference_golden_through_the_cache():
    """the reference's own WDDPPO.update on a 3-step x 2-environment rollout, from the four feature
    keys and WITHOUT rgb / depth / rgb_history / depth_history: the compare call under which the frame
    path is held to the fixture"""
    golden_through_the_cache("waypoint_ppo_update_64", envs_per_call=2)


def test_full_size_golden_through_the_cache():
    """the same at workload size, once: 32 environments of 256 x 256 frames, the features made in four
    calls of 8 environments (96 frames each) as a rollout makes them -- collection and update then
    land on different kernel instances, which is the property the cache rests on"""
    golden_through_the_cache("waypoint_update_n32_256", envs_per_call=8)


# ---- a collected rollout
@pytest.fixture(scope="module")
def collected():
    policy = wf.build_policy(DEV)
    with wf.TrunkCounter(policy.net) as counter:
        st, panos = wf.collect(policy, DEV)
    torch.cuda.synchronize()
    return policy, st, panos, counter.calls


def test_collected_rollout_bit_for_bit(collected):
    policy, st, panos, trunk_calls = collected
    T, N, P = wf.T, wf.N, wf.P
    assert trunk_calls == 2 * (T + 1) + 2      # per row and sensor one call over the panorama; two zero frames
    assert st.trunk_valid == [True] * (T + 1) and st.trunk_key == policy.net.trunk_cache_key()
    assert int(panos[wf.STOP_AT[0]][wf.STOP_AT[1]]) == P
    assert float(st.masks[wf.DONE_AT[0]][wf.DONE_AT[1]]) == 0.0
    for s in wf.SENSORS:
        zero = policy.net.trunk_zero(s, st.observations[s].shape[-3:], DEV)
        assert float(zero.abs().sum()) > 0.0
        feats, hist = st.observations[s + "_features"], st.observations[s + "_history_features"]
        for t in range(T):
            for i in range(N):
                p = int(panos[t][i])
                assert torch.equal(hist[t + 1][i], feats[t][i, p] if p < P else zero), (s, t, i)
    # the rows a minibatch without frames yields are the arena rows of its environments
    adv = st.get_advantages(False)
    perm = torch.tensor([1, 0])
    with rc.fixed_randperm([perm]):
        batches = list(st.recurrent_generator(adv, 2, frames=False))
    for m, sample in enumerate(batches):
        env = int(perm[m])
        assert set(sample[0]) == set(st.observations) - set(FRAME_KEYS)
        for k, v in sample[0].items():
            assert torch.equal(v, st.observations[k][:T, env]), k
    # after_update: row 0 holds row T and is valid; the next step 0 runs no trunk
    st = wf.copied(st)
    last = {k: v[T].clone() for k, v in st.observations.items()}
    st.after_update()
    assert st.trunk_valid == [True] + [False] * T and st.step == 0
    for k, v in last.items():
        assert torch.equal(st.observations[k][0], v), k
    with wf.TrunkCounter(policy.net) as counter:
        _, history, _ = ppo_harness.act_for_rollout(policy, st)
    assert counter.calls == 0
    assert set(history) == {"rgb", "depth", "rgb_history_features", "depth_history_features"}


def updated(st, perms, **kw):
    policy = wf.warm_zero(wf.build_policy(DEV), st)
    cfg = PPOConfig(**cases.PPO)
    opt = Adam([p for p in policy.parameters() if p.requires_grad], lr=2.5e-4, eps=1e-5,
               max_grad_norm=cfg.max_grad_norm)
    with rc.fixed_randperm(perms), wf.TrunkCounter(policy.net) as counter:
        stats = wddppo_update(policy, opt, st, cfg, ppo_epoch=2, num_mini_batch=2, **kw)
    return policy, stats, counter.calls


def test_update_from_the_cache_equals_the_update_from_frames(collected):
    """two policies of the same state, each with its own optimizer: wddppo_update from the cache and
    from the frames under the same permutations; the six statistics and every parameter at
    rtol 1e-4 / atol 1e-5, the pair tests/test_policy_gpu.py uses for two policies that should be the
    same"""
    first, st, _, _ = collected
    perms = [torch.tensor([1, 0]), torch.tensor([0, 1])]
    a, stats_a, calls_a = updated(st, perms, use_trunk_cache=True)
    b, stats_b, calls_b = updated(st, perms, use_trunk_cache=False)
    assert calls_a == 0 and calls_b == 2 * 4      # two sensors, 2 epochs x 2 minibatches
    sa, sb = torch.tensor(stats_a, dtype=torch.float64), torch.tensor(stats_b, dtype=torch.float64)
    print(f"statistics: cache {stats_a}\n            frames {stats_b}\n            max|d| {float((sa - sb).abs().max()):.3e}")
    worst = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(a.parameters(), b.parameters()))
    print(f"parameters: max|d| {worst:.3e}")
    assert torch.allclose(sa, sb, rtol=1e-4, atol=1e-5)
    moved = 0
    for (n, p), q, r in zip(a.named_parameters(), b.parameters(), first.parameters()):
        assert torch.allclose(p, q, rtol=1e-4, atol=1e-5), n
        moved += int(not torch.equal(p, r))
    assert moved > 0


def test_refusals_on_the_device(collected):
    _, st, _, _ = collected
    cfg = PPOConfig(**cases.PPO)
    kw = dict(ppo_epoch=1, num_mini_batch=2, use_trunk_cache=True)
    policy = wf.build_policy(DEV)
    policy.net.rgb_encoder.train()
    with pytest.raises(RuntimeError, match="BatchNorm of rgb_encoder is in training mode"):
        wddppo_update(policy, None, st, cfg, **kw)
    policy = wf.build_policy(DEV)
    with torch.no_grad():      # an in-place change of a trunk weight between collection and update
        policy.net.depth_encoder.visual_encoder.backbone.conv1[0].weight.mul_(1.5)
    with pytest.raises(RuntimeError, match="depth_encoder.*parameter versions"):
        wddppo_update(policy, None, st, cfg, **kw)
    obs = {k: v[0] for k, v in st.observations.items()}
    obs["trunk_feature_key"] = st.trunk_key
    with pytest.raises(RuntimeError, match="depth_encoder.*another key"), torch.no_grad():
        policy.get_value(obs, st.recurrent_hidden_states[0], {k: v[0] for k, v in st.prev_actions.items()},
                         st.masks[0])
    # a storage without feature arenas
    policy = wf.build_policy(DEV)
    plain, _ = wf.collect(policy, DEV, trunk_features=False)
    assert not plain.has_trunk_features and isinstance(plain, ActionDictRolloutStorage)
    with pytest.raises(RuntimeError, match="no feature arenas"):
        wddppo_update(policy, None, plain, cfg, **kw)
