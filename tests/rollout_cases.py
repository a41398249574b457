"""Shared by the rollout storage tests (host and GPU tier): tests/golden/rollout_storage.npz -- the
reference's own ActionDictRolloutStorage driven on the CPU by tests/golden/make_goldens_rollout.py --
replayed through vlnce_amd.ActionDictRolloutStorage and compared bit for bit."""
import contextlib
import functools
import os
import types

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden", "rollout_storage.npz")
NUM_STEPS, N, L, H = 3, 4, 2, 8
SENSORS = {"rgb": (2, 5, 7, 3), "depth": (2, 4, 4, 1), "angle_features": (12, 4), "instruction": (11,)}
ACTION_KEYS = ("pano", "offset", "distance")


def space(sensors=None):
    sensors = SENSORS if sensors is None else sensors
    return types.SimpleNamespace(spaces={k: types.SimpleNamespace(shape=s) for k, s in sensors.items()})


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLD)
    return {k: (torch.from_numpy(z[k]) if z[k].ndim else float(z[k])) for k in z.files}


def sub(z, prefix):
    """the entries below `prefix/`, nested one level per '/'"""
    out = {}
    for k, v in z.items():
        if k.startswith(prefix + "/"):
            node, parts = out, k[len(prefix) + 1:].split("/")
            for p in parts[:-1]:
                node = node.setdefault(p, {})
            node[parts[-1]] = v
    return out


@contextlib.contextmanager
def fixed_randperm(perms):
    """torch.randperm hands out the stored permutations, in order: the cut of the minibatches does
    not depend on the torch build"""
    real, left = torch.randperm, list(perms)

    def stored(n, *a, **kw):
        p = left.pop(0)
        assert p.numel() == n
        return p.clone()

    torch.randperm = stored
    try:
        yield
    finally:
        torch.randperm = real
    assert not left, "a generator pass drew no permutation"


def same(got, want, what):
    assert got.dtype == want.dtype, f"{what}: {got.dtype} for {want.dtype}"
    assert tuple(got.shape) == tuple(want.shape), f"{what}: {tuple(got.shape)} for {tuple(want.shape)}"
    assert torch.equal(got.cpu(), want), f"{what}: values differ"


def check_sample(sample, want, what):
    obs, hidden, actions, prev_actions, value_preds, returns, masks, logp, adv = sample
    assert set(obs) == set(want["obs"]) and set(actions) == set(ACTION_KEYS) == set(prev_actions)
    for k in obs:
        same(obs[k], want["obs"][k], f"{what} obs[{k}]")
    for k in ACTION_KEYS:
        same(actions[k], want["actions"][k], f"{what} actions[{k}]")
        same(prev_actions[k], want["prev_actions"][k], f"{what} prev_actions[{k}]")
    for got, name in ((hidden, "hidden"), (value_preds, "value_preds"), (returns, "returns"),
                      (masks, "masks"), (logp, "logp"), (adv, "adv")):
        same(got, want[name], f"{what} {name}")


def insert_step(st, inputs, device):
    dev = lambda t: t.to(device)   # noqa: E731
    st.insert({k: dev(v) for k, v in inputs["obs"].items()}, dev(inputs["hidden"]),
              {k: dev(v) for k, v in inputs["action"].items()}, dev(inputs["logp"]),
              dev(inputs["value"]), dev(inputs["reward"]), dev(inputs["mask"]))


def replay(name, device, make_storage):
    """the golden script through `make_storage(num_steps, num_envs, space, H, **kw)`, every yielded
    tensor and every arena held to the reference's bits"""
    z = golden()
    g = sub(z, name)
    discrete = name == "disc"
    st = make_storage(NUM_STEPS, N, space(), H, num_recurrent_layers=L, continuous_offset=not discrete,
                      continuous_distance=not discrete)
    for k, v in g["obs0"].items():
        st.observations[k][0].copy_(v.to(device))

    def run_pass(tag, next_value, num_mini_batch):
        st.compute_returns(next_value.to(device), True, z["gamma"], z["tau"])
        st.check_returns()
        adv = st.get_advantages(False)
        same(adv, g[tag]["advantages"][:st.step], f"{name}/{tag} advantages")
        with fixed_randperm([g[tag]["perm"]]):
            batches = list(st.recurrent_generator(adv, num_mini_batch))
        assert len(batches) == num_mini_batch
        for m, sample in enumerate(batches):
            check_sample(sample, g[tag][f"mb{m}"], f"{name}/{tag}/mb{m}")

    for i in range(5):
        if i == 3:
            assert st.step == 3
            run_pass("pass0", g["next_value0"], 2)
            st.after_update()
            assert st.step == 0
        insert_step(st, g[f"insert{i}"], device)
    assert st.step == 2 and isinstance(st.step, int)
    run_pass("pass1", g["next_value1"], 4)
    final = g["final"]
    for k in final["observations"]:
        same(st.observations[k], final["observations"][k], f"{name} observations[{k}]")
    for k in ACTION_KEYS:
        same(st.actions[k], final["actions"][k], f"{name} actions[{k}]")
        same(st.prev_actions[k], final["prev_actions"][k], f"{name} prev_actions[{k}]")
    for attr in ("recurrent_hidden_states", "rewards", "value_preds", "returns", "action_log_probs",
                 "masks"):
        same(getattr(st, attr), final[attr], f"{name} {attr}")
    return st


def collect_with_policy(policy, obs, masks, h0, N, T, device, make_storage):
    """a storage filled the way ddppo_waypoint_trainer.py fills it (:162-173, 289-298, 394-395), from
    policy.act on a case's time-major inputs (row t * N + n): returns it after compute_returns"""
    sensors = {k: tuple(v.shape[1:]) for k, v in obs.items()}
    L, Hs = h0.size(1), h0.size(2)
    st = make_storage(T, N, space(sensors), Hs, num_recurrent_layers=L, device=device)
    rows = lambda t: slice((t % T) * N, (t % T + 1) * N)   # noqa: E731
    for k, v in obs.items():
        st.observations[k][0].copy_(v[rows(0)])
    st.recurrent_hidden_states[0].copy_(h0)
    st.masks[0].copy_(masks[rows(0)])
    g = torch.Generator().manual_seed(17)
    for t in range(T):
        step_obs = {k: v[st.step] for k, v in st.observations.items()}
        with torch.no_grad():
            values, _, elements, _, _, log_prob, hidden, _ = policy.act(
                step_obs, st.recurrent_hidden_states[st.step],
                {k: v[st.step] for k, v in st.prev_actions.items()}, st.masks[st.step])
        rewards = (torch.randn(N, 1, generator=g) * 0.5).to(device)
        st.insert({k: v[rows(t + 1)] for k, v in obs.items()}, hidden, elements, log_prob, values,
                  rewards, masks[rows(t + 1)].float())
    with torch.no_grad():
        next_value = policy.get_value({k: v[st.step] for k, v in st.observations.items()},
                                      st.recurrent_hidden_states[st.step],
                                      {k: v[st.step] for k, v in st.prev_actions.items()},
                                      st.masks[st.step])
    st.compute_returns(next_value, True, 0.99, 0.95)
    return st


def torch_minibatches(st, advantages, num_mini_batch, perm):
    """recurrent_generator restated with plain torch indexing on the storage's own arenas"""
    T, n = st.step, st.rewards.size(1) // num_mini_batch
    for start in range(0, n * num_mini_batch, n):
        envs = perm[start:start + n].to(st.returns.device)

        def cut(arena):
            x = arena[:T][:, envs]
            return x.reshape(T * n, *x.shape[2:])

        yield ({k: cut(v) for k, v in st.observations.items()}, st.recurrent_hidden_states[0][envs].clone(),
               {k: cut(st.actions[k]) for k in st.actions},
               {k: cut(st.prev_actions[k]) for k in st.actions}, cut(st.value_preds), cut(st.returns),
               cut(st.masks), cut(st.action_log_probs), cut(advantages))
