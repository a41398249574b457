"""Shared by the trunk-feature cache tests (host and GPU tier).  `feature_pick_ref` and
`feature_rows_ref` ARE the written contract of vlnce_waypoint_feature_pick / vlnce_waypoint_feature_rows
(include/vlnce_hip.h, ABI 155) in plain torch; `FeatureSim` runs the package's host code on them
without a GPU; `collect` is the small rollout both tiers drive through ppo_harness."""
import copy
import os
import types

import torch

import cases
import vlnce_amd
from oracle import thirdparty as tp
from test_rollout_storage_host import RolloutSim
from test_waypoint_act_host import WaypointActSim
from vlnce_amd import ppo_harness
from vlnce_amd.rollout_storage import ActionDictRolloutStorage

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SENSORS = ("rgb", "depth")


def feature_pick_ref(src, zero, pano):
    """src [B, P, ...], zero [...], pano int64 [B] -> [B, ...]: the chosen slot, `zero` outside 0..P-1"""
    B, P = src.shape[:2]
    out = torch.empty((B,) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)
    for b, p in enumerate(pano.reshape(-1).tolist()):
        out[b] = src[b, p] if 0 <= p < P else zero
    return out


def feature_rows_ref(pano, hist, zero, masks):
    """pano [B, P, ...], hist [B, ...], zero [...], masks [B] -> [B, P + 1, ...]: the panorama rows, then
    the history row where masks[b] != 0 and `zero` where it is 0"""
    B, P = pano.shape[:2]
    out = torch.empty((B, P + 1) + tuple(pano.shape[2:]), dtype=pano.dtype, device=pano.device)
    out[:, :P] = pano
    for b, m in enumerate(masks.reshape(-1).tolist()):
        out[b, P] = hist[b] if m != 0 else zero
    return out


class FeatureSim(WaypointActSim, RolloutSim):
    """the tensor-level simulator with the two entry points of ABI 155 beside the rollout storage's
    and act()'s"""

    def __init__(self):
        RolloutSim.__init__(self)
        self.option = 0

    def waypoint_feature_pick(self, fields, pano, B, P):
        self.calls.append("waypoint_feature_pick")
        assert pano.dtype == torch.int64 and pano.numel() == B
        for src, zero, dst in fields:
            assert src.dtype == zero.dtype == dst.dtype == torch.float32 and src.shape[:2] == (B, P)
            dst.copy_(feature_pick_ref(src, zero, pano).view_as(dst))

    def waypoint_feature_rows(self, fields, masks, B, P):
        self.calls.append("waypoint_feature_rows")
        assert masks.dtype in (torch.uint8, torch.float32) and masks.numel() == B
        for pano, hist, zero, out in fields:
            assert pano.dtype == hist.dtype == zero.dtype == out.dtype == torch.float32
            assert pano.shape[:2] == (B, P) and out.shape[:2] == (B, P + 1)
            out.copy_(feature_rows_ref(pano, hist, zero, masks))

    def names(self):
        return [c if isinstance(c, str) else c[0] for c in self.calls]


def build_policy(device, name="waypoint_ppo_update_64"):
    """the case's policy as the trainer holds it during an update (agent.train(), encoders in eval
    mode).  Every call builds the same policy again -- same seeded state, same parameter versions and
    so the same trunk_cache_key(): the tests' "copies" of a policy (the net's graphed tail holds on
    to the net it was made for, so copy.deepcopy is not a way to get one)."""
    policy, _ = cases.build_policy(vlnce_amd, cases.CASES[name], vlnce_amd.make_config,
                                   vlnce_amd.make_spaces, tp.synth_state_dict)
    return policy.to(device)


def warm_zero(policy, st):
    """the zero frames' features of a freshly built policy, as the collecting policy has them"""
    for s in SENSORS:
        policy.net.trunk_zero(s, st.observations[s].shape[-3:], st.observations[s].device)
    return policy


def copied(st):
    """a storage of its own with the same contents"""
    st._build_tables()      # (drops the cached row views and the library handle: neither is to be copied)
    st = copy.deepcopy(st)
    st._build_tables()
    return st


class TrunkCounter:
    """counts the trunk calls of a net (both encoders' trunk_features) while active"""

    def __init__(self, net):
        self.encoders = [net.rgb_encoder, net.depth_encoder]
        self.calls = 0

    def __enter__(self):
        for enc in self.encoders:
            inner = type(enc).trunk_features

            def counted(observations, enc=enc, inner=inner):
                self.calls += 1
                return inner(enc, observations)

            enc.trunk_features = counted
        return self

    def __exit__(self, *exc):
        for enc in self.encoders:
            del enc.trunk_features


T, N, HW, P = 3, 2, 64, 12
STOP_AT = (1, 0)   # (step, environment) whose action is forced to STOP
DONE_AT = (2, 1)   # the mask inserted behind step 1 ends environment 1's episode: masks[2][1] == 0


def simulator_frames(device, seed=3):
    """seeded frames standing in for the simulator: what it would return for steps 0..T"""
    g = torch.Generator().manual_seed(seed)
    tok = torch.zeros(N, 200, dtype=torch.long)
    for i, L in enumerate((9, 14)):
        tok[i, :L] = torch.randint(1, cases.VOCAB, (L,), generator=g)
    steps = []
    for _ in range(T + 1):
        steps.append({
            "rgb": torch.randint(0, 256, (N, P, HW, HW, 3), generator=g).float().to(device),
            "depth": torch.rand(N, P, HW, HW, 1, generator=g).to(device),
            "angle_features": torch.randn(N, P, 4, generator=g).to(device),
            "instruction": tok.to(device),
        })
    return steps


def _stops_row(net, row):
    """net.forward with the STOP logit of `row` raised (and every other row's lowered) by 60"""
    from vlnce_amd.utils import CustomFixedCategorical

    def forward(*args, **kwargs):
        out = list(type(net).forward(net, *args, **kwargs))
        raw = torch.is_tensor(out[0])
        logits = (out[0] if raw else out[0].logits).clone()
        logits[:, -1] -= 60.0
        logits[row, -1] += 120.0
        out[0] = logits if raw else CustomFixedCategorical(logits=logits)
        return tuple(out)

    return forward


def collect(policy, device, trunk_features=True, fused_act=True, seed=0):
    """T steps of act_for_rollout + insert as ddppo_waypoint_trainer.py:160-220 drives them, then
    bootstrap_value + compute_returns.  Returns (storage, [pano choice of every step])."""
    net = policy.net
    frames = simulator_frames(device)
    shapes = {k: tuple(v.shape[1:]) for k, v in frames[0].items()}
    for k in SENSORS:   # the trainer adds the history sensors to the space
        shapes[k + "_history"] = shapes[k][1:]
    space = types.SimpleNamespace(spaces={k: types.SimpleNamespace(shape=s) for k, s in shapes.items()})
    st = ActionDictRolloutStorage(
        T, N, space, net._hidden_size, num_recurrent_layers=net.num_recurrent_layers, device=device,
        trunk_features=net.trunk_feature_shapes() if trunk_features else None)
    for k, v in frames[0].items():
        st.observations[k][0].copy_(v)
    policy.fused_act = fused_act
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(17)
    panos = []
    for t in range(T):
        if t == STOP_AT[0]:
            net.forward = _stops_row(net, STOP_AT[1])
        try:
            outputs, history, _ = ppo_harness.act_for_rollout(policy, st)
        finally:
            net.__dict__.pop("forward", None)
        values, actions, elements, _, _, log_prob, hidden, _ = outputs
        if t == STOP_AT[0]:
            assert [a["action"] == "STOP" for a in actions] == [i == STOP_AT[1] for i in range(N)]
        panos.append(elements["pano"].reshape(-1).clone())
        batch = dict(frames[t + 1])
        for k, v in history.items():   # (ddppo_waypoint_trainer.py:237-238, and the feature history beside it)
            batch[k + "_history" if k in SENSORS else k] = v
        masks = torch.ones(N, 1, device=device)
        if t + 1 == DONE_AT[0]:
            masks[DONE_AT[1]] = 0.0
        rewards = (torch.randn(N, 1, generator=g) * 0.5).to(device)
        st.insert(batch, hidden, elements, log_prob, values, rewards, masks)
    next_value = ppo_harness.bootstrap_value(policy, st)
    st.compute_returns(next_value, True, 0.99, 0.95)
    return st, panos
