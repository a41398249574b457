"""Golden vectors for the DD-PPO rollout storage: __init__, insert, after_update,
compute_returns, recurrent_generator and _flatten_helper of ActionDictRolloutStorage are extracted
from vlnce_baselines/common/rollout_storage.py with `ast` and hung on a plain class (none of them
needs the habitat base class), then driven on the CPU the way ddppo_waypoint_trainer.py drives them:
row 0 of the observations, three inserts, compute_returns (GAE), a generator pass with two
minibatches, after_update, two more inserts (a partial rollout: step < num_steps), compute_returns,
a generator pass with four minibatches.  Stored: every input, the permutation each pass drew, every
yielded tensor, every arena at the end -- for both action components continuous ("cont") and both
discrete ("disc").  CPU container only.   python tests/golden/make_goldens_rollout.py"""
import ast
import os
import sys
import types
import typing
from collections import defaultdict

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.oracle import shims  # noqa: E402

NUM_STEPS, N, L, H = 3, 4, 2, 8
SENSORS = {"rgb": (2, 5, 7, 3), "depth": (2, 4, 4, 1), "angle_features": (12, 4), "instruction": (11,)}
GAMMA, TAU = 0.99, 0.95
WANTED = ("__init__", "insert", "after_update", "compute_returns", "recurrent_generator",
          "_flatten_helper")
YIELDED = ("obs", "hidden", "actions", "prev_actions", "value_preds", "returns", "masks", "logp", "adv")


def reference_class():
    path = os.path.join(shims.REFERENCE_ROOT, "vlnce_baselines/common/rollout_storage.py")
    fns = [n for n in ast.walk(ast.parse(open(path).read()))
           if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(f.name for f in fns) == sorted(WANTED)
    cls = ast.ClassDef(name="ReferenceStorage", bases=[], keywords=[], body=fns, decorator_list=[],
                       **({"type_params": []} if sys.version_info >= (3, 12) else {}))
    scope = {"torch": torch, "Tensor": torch.Tensor, "defaultdict": defaultdict, "Space": object,
             "Observations": dict, "Dict": typing.Dict, "Iterator": typing.Iterator,
             "Tuple": typing.Tuple, "DefaultDict": typing.DefaultDict}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[cls], type_ignores=[])), path, "exec"),
         scope)
    return scope["ReferenceStorage"]


def step_inputs(g, discrete, first_mask):
    obs = {k: torch.randn(N, *shape, generator=g) for k, shape in SENSORS.items()}
    obs["instruction"] = torch.randint(0, 2504, (N, 11), generator=g).float()
    action = {"pano": torch.randint(0, 12, (N, 1), generator=g)}
    if discrete:
        action["offset"] = torch.randint(0, 7, (N, 1), generator=g)
        action["distance"] = torch.randint(0, 6, (N, 1), generator=g)
    else:
        action["offset"] = torch.rand(N, 1, generator=g) * 0.5 - 0.25
        action["distance"] = torch.rand(N, 1, generator=g) * 2.5 + 0.25
    masks = (torch.rand(N, 1, generator=g) > 0.3).float()
    if first_mask is not None:
        masks[0, 0] = first_mask
    if discrete:
        masks = masks.to(torch.uint8)   # (the trainer hands floats; the arena is uint8 either way)
    return dict(obs=obs, hidden=torch.randn(N, L, H, generator=g), action=action,
                logp=-torch.rand(N, 1, generator=g), value=torch.randn(N, 1, generator=g),
                reward=torch.randn(N, 1, generator=g) * 0.5, mask=masks)


def put(blob, prefix, value):
    if isinstance(value, dict):
        for k, v in value.items():
            put(blob, f"{prefix}/{k}", v)
    else:
        blob[prefix] = value.numpy().copy()


def run_pass(storage, blob, tag, num_mini_batch):
    advantages = storage.returns[:-1] - storage.value_preds[:-1]   # WDDPPO.get_advantages, not normalised
    put(blob, f"{tag}/advantages", advantages)
    drawn, real = [], torch.randperm

    def recording(n):
        drawn.append(real(n))
        return drawn[-1].clone()

    torch.randperm = recording
    try:
        batches = list(storage.recurrent_generator(advantages, num_mini_batch))
    finally:
        torch.randperm = real
    assert len(drawn) == 1 and len(batches) == num_mini_batch
    put(blob, f"{tag}/perm", drawn[0])
    for m, sample in enumerate(batches):
        for name, value in zip(YIELDED, sample):
            put(blob, f"{tag}/mb{m}/{name}", dict(value) if isinstance(value, dict) else value)


def variant(ref_cls, name, discrete, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    space = types.SimpleNamespace(spaces={k: types.SimpleNamespace(shape=s) for k, s in SENSORS.items()})
    st = ref_cls(NUM_STEPS, N, space, H, num_recurrent_layers=L, continuous_offset=not discrete,
                 continuous_distance=not discrete)
    blob = {}
    first = step_inputs(g, discrete, None)["obs"]
    put(blob, f"{name}/obs0", first)
    for k in first:
        st.observations[k][0].copy_(first[k])
    # one mask of each value in the first rollout whatever the draw
    for i, first_mask in zip(range(5), (0.0, 1.0, None, None, None)):
        if i == 3:
            nv = torch.randn(N, 1, generator=g)
            put(blob, f"{name}/next_value0", nv)
            st.compute_returns(nv, True, GAMMA, TAU)
            run_pass(st, blob, f"{name}/pass0", 2)
            st.after_update()
        inputs = step_inputs(g, discrete, first_mask)
        put(blob, f"{name}/insert{i}", inputs)
        st.insert(inputs["obs"], inputs["hidden"], inputs["action"], inputs["logp"], inputs["value"],
                  inputs["reward"], inputs["mask"])
    assert st.step == 2 < NUM_STEPS
    nv = torch.randn(N, 1, generator=g)
    put(blob, f"{name}/next_value1", nv)
    st.compute_returns(nv, True, GAMMA, TAU)
    run_pass(st, blob, f"{name}/pass1", 4)
    put(blob, f"{name}/final", dict(
        observations=st.observations, recurrent_hidden_states=st.recurrent_hidden_states,
        rewards=st.rewards, value_preds=st.value_preds, returns=st.returns,
        action_log_probs=st.action_log_probs, actions=st.actions, prev_actions=st.prev_actions,
        masks=st.masks))
    return blob


def main():
    ref_cls = reference_class()
    blob = dict(gamma=np.float64(GAMMA), tau=np.float64(TAU))
    blob.update(variant(ref_cls, "cont", False, 31))
    blob.update(variant(ref_cls, "disc", True, 32))
    out = os.path.join(HERE, "rollout_storage.npz")
    np.savez_compressed(out, **blob)
    print(len(blob), "arrays,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
