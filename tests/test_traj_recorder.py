"""DAgger rollout collection, CPU tier: data_path.TrajectoryRecorder / dagger_step through the
numpy simulator of csrc/traj.hip (tests/hostsim_traj.py) against a restatement of the reference's
own bookkeeping (dagger_trainer.py:339-386, :414-442).  Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

import hostsim_traj
from vlnce_amd import _lib, data_path

EXPERT = "shortest_path_sensor"


def same_bits(a, b):
    """dtype, shape and bits; NaN is compared with isnan, not by payload"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


# ------------------------------------------------------------------ numpy itself
def test_numpy_narrows_as_the_kernel_tests_assume():
    """the GPU tier takes astype(np.float16) as its reference; this pins what that is: round to
    nearest even, subnormals kept, overflow to infinity, int64 by way of float32"""
    def i64(v):
        return float(np.array([v], dtype=np.int64).astype(np.float32).astype(np.float16)[0])

    def f32(v):
        return float(np.array([v], dtype=np.float32).astype(np.float16)[0])

    assert i64(2049) == 2048.0 and i64(2051) == 2052.0 and i64(2503) == 2504.0
    with np.errstate(over="ignore"):
        assert f32(65520.0) == float("inf")
    assert f32(65519.996) == 65504.0
    assert f32(2.0 ** -25) == 0.0
    assert f32(1.0001 * 2.0 ** -25) == 2.0 ** -24
    assert f32(1.0 + 2.0 ** -11) == 1.0
    assert f32(1.0 + 3 * 2.0 ** -11) == 1.0 + 2.0 ** -9
    # the float32 inputs above are what they claim to be
    assert float(np.float32(65519.996)) < 65520.0 and float(np.float32(1.0001 * 2.0 ** -25)) > 2.0 ** -25


# ------------------------------------------------------------------ binding: the [n, C, P] form
def test_collapse_rows_finds_the_strided_form():
    n = 3
    nhwc = torch.zeros(n, 2, 2, 8).permute(0, 3, 1, 2)             # the trunks' output view
    assert _lib.collapse_rows(nhwc)[1:] == (32, 8, 1, 4, 8)
    assert _lib.collapse_rows(torch.zeros(n, 4, 2, 2))[1:] == (16, 16, 1, 1, 0)
    assert _lib.collapse_rows(torch.zeros(n, 1))[1:] == (1, 1, 0, 1, 0)
    assert _lib.collapse_rows(torch.zeros(n))[1:] == (1, 1, 0, 1, 0)
    wide = torch.zeros(n, 40)
    assert _lib.collapse_rows(wide[:, 3:19].unflatten(1, (4, 2, 2)))[1:] == (40, 16, 1, 1, 0)
    assert _lib.collapse_rows(wide[:, ::2])[1:] == (40, 20, 2, 1, 0)
    three = torch.zeros(n, 4, 6, 10)[:, :, :3, :5]                  # three groups: no such form
    t, rs, C, cs, P, ps = _lib.collapse_rows(three)
    assert t.is_contiguous() and (rs, C, cs, P, ps) == (60, 60, 1, 1, 0)
    assert _lib.collapse_rows(torch.zeros(1, 4, 2, 2))[1] == 0       # a single row has no stride


# ------------------------------------------------------------------ scripted loop
SPECIAL_F32 = [65520.0, 65519.996, 2.0 ** -25, 1.0001 * 2.0 ** -25, 1.0 + 2.0 ** -11,
               1.0 + 3 * 2.0 ** -11, -0.0, float("inf"), -70000.0, 6.1e-5, 5.9e-8]
TOKENS = [2049, 2051, 2503]
NUM_ENVS, STEPS = 5, 23
# (step, active position): expert action -1 on an episode's last step (the episode is dropped) and
# in the middle of one (the row stays, the simulator gets action 0)
SKIP_LAST, SKIP_MIDDLE = (4, 2), (7, 0)
PAUSE_AT, PAUSED = 11, [1, 3]


def _script():
    """per step: (observations of the active environments, expert actions [n, 1] float, policy
    actions [n, 1], dones) -- all seeded"""
    g = torch.Generator().manual_seed(11)
    rng = np.random.RandomState(5)
    n, steps = NUM_ENVS, []
    for step in range(STEPS):
        if step == PAUSE_AT:
            n -= len(PAUSED)
        rgb_out = (torch.randn(n, 2, 2, 8, generator=g) * 40).permute(0, 3, 1, 2)   # NHWC view
        depth_out = torch.randn(n, 4, 2, 2, generator=g)
        k = step % len(SPECIAL_F32)
        rgb_out[0, 1, 0, 1] = SPECIAL_F32[k]
        depth_out[n - 1, 2, 1, 0] = SPECIAL_F32[(k + 3) % len(SPECIAL_F32)]
        tokens = torch.randint(0, 2504, (n, 10), generator=g)
        tokens[:, 3] = TOKENS[step % 3]
        tokens[0, 7] = TOKENS[(step + 1) % 3]
        obs = {"rgb": torch.rand(n, 3, 3, 3, generator=g),
               "instruction": tokens,
               EXPERT: torch.randint(0, 4, (n, 1), generator=g).float(),
               "progress": torch.rand(n, 1, generator=g)}
        dones = [bool(rng.rand() < 0.25) for _ in range(n)]
        for (s, i), last in ((SKIP_LAST, True), (SKIP_MIDDLE, False)):
            if step == s:
                obs[EXPERT][i] = -1.0
                dones[i] = last
        if step == SKIP_MIDDLE[0] + 2:
            dones[SKIP_MIDDLE[1]] = True      # ... and that episode does end, two steps on
        steps.append((obs, rgb_out, depth_out, torch.randint(0, 4, (n, 1), generator=g), dones))
    return steps


def _restatement(fp16, beta):
    """the reference's bookkeeping in its own shape: per environment a list of (row dict, prev,
    expert); at an episode's end stack, cast to float as batch_obs does, narrow with astype"""
    torch.manual_seed(3)
    episodes = [[] for _ in range(NUM_ENVS)]
    prev_actions = torch.zeros(NUM_ENVS, 1, dtype=torch.long)
    skips, dones = [False] * NUM_ENVS, [False] * NUM_ENVS
    written, stepped = [], []

    def write(ep):
        traj = {}
        for key in ep[0][0]:
            if key == EXPERT:
                continue
            v = torch.stack([row[0][key] for row in ep]).to(dtype=torch.float).numpy()
            with np.errstate(over="ignore"):
                traj[key] = v.astype(np.float16) if fp16 else v
        return [traj, np.array([row[1] for row in ep], dtype=np.int64),
                np.array([row[2] for row in ep], dtype=np.int64)]

    for step, (obs, rgb_out, depth_out, actions, new_dones) in enumerate(_script() + [(None,) * 5]):
        for i in range(len(episodes)):
            if dones[i] and not skips[i]:
                written.append(write(episodes[i]))
            if dones[i]:
                episodes[i] = []
        if step == STEPS:
            break
        if step == PAUSE_AT:
            for i in reversed(PAUSED):
                episodes.pop(i)
            keep = [i for i in range(prev_actions.size(0)) if i not in PAUSED]
            prev_actions = prev_actions[keep]
        actions = torch.where(torch.rand_like(actions, dtype=torch.float) < beta,
                              obs[EXPERT].long(), actions)
        for i in range(len(episodes)):
            row = {k: v[i] for k, v in obs.items()}
            row["rgb_features"] = rgb_out[i]
            del row["rgb"]
            row["depth_features"] = depth_out[i]
            episodes[i].append((row, prev_actions[i].item(), obs[EXPERT][i].item()))
        skips = obs[EXPERT].long() == -1
        actions = torch.where(skips, torch.zeros_like(actions), actions)
        skips = skips.squeeze(-1).tolist()
        prev_actions.copy_(actions)
        stepped.append([a[0].item() for a in actions])
        dones = new_dones
    leftovers = [write(ep) if ep else None for ep in episodes]
    return written, leftovers, stepped


def _recorded(fp16, beta):
    torch.manual_seed(3)
    rec = data_path.TrajectoryRecorder(NUM_ENVS, "cpu", fp16, capacity=2, exclude=(EXPERT,))
    rgb_hook, depth_hook = rec.feature_hook("rgb_features"), rec.feature_hook("depth_features")
    prev_actions = torch.zeros(NUM_ENVS, 1, dtype=torch.long)
    skips, dones = [False] * NUM_ENVS, [False] * NUM_ENVS
    written, stepped = [], []
    for step, (obs, rgb_out, depth_out, actions, new_dones) in enumerate(_script() + [(None,) * 5]):
        n = len(dones)
        written += rec.pop([i for i in range(n) if dones[i] and not skips[i]])
        rec.discard([i for i in range(n) if dones[i] and skips[i]])
        if step == STEPS:
            break
        if step == PAUSE_AT:
            rec.pause(PAUSED)
            keep = [i for i in range(n) if i not in PAUSED]
            prev_actions = prev_actions[keep].contiguous()
        rgb_hook(None, None, rgb_out)       # what act() would trigger
        depth_hook(None, None, depth_out)
        rec.append(obs, prev_actions, obs[EXPERT])
        before = prev_actions
        new_actions, ints, skips = data_path.dagger_step(actions, obs[EXPERT], beta, prev_actions)
        assert prev_actions is before and torch.equal(new_actions, prev_actions)
        stepped.append(ints)
        dones = new_dones
    lengths = rec.lengths()
    leftovers = [ep if lengths[i] else None
                 for i, ep in enumerate(rec.pop(range(len(lengths))))]
    return written, leftovers, stepped, rec


def _assert_same_episode(got, want):
    assert isinstance(got, list) and len(got) == 3
    assert list(got[0]) == list(want[0])                      # keys, in order
    for key in want[0]:
        assert same_bits(got[0][key], want[0][key]), key
        assert got[0][key].flags.owndata
    for k in (1, 2):
        assert got[k].dtype == np.int64 and same_bits(got[k], want[k])


@pytest.mark.parametrize("fp16", [True, False])
def test_scripted_collection_loop_matches_the_restatement(monkeypatch, fp16):
    monkeypatch.setattr(_lib, "_LIB", hostsim_traj.HostSimTraj())
    beta = 0.5
    want, want_left, want_stepped = _restatement(fp16, beta)
    got, got_left, got_stepped, rec = _recorded(fp16, beta)
    assert rec.capacity >= 8                                   # 2 -> 4 -> 8: grown at least twice
    assert got_stepped == want_stepped                         # same RNG stream, same skip rule
    assert len(want) >= 6 and len(got) == len(want)
    # the script did what it says: an expert -1 inside a written episode, none at an end
    assert any((ep[2][:-1] == -1).any() for ep in want) and all(ep[2][-1] != -1 for ep in want)
    for g, w in zip(got, want):
        _assert_same_episode(g, w)
        dt = np.float16 if fp16 else np.float32
        assert all(v.dtype == dt for v in g[0].values())
        assert list(g[0]) == ["instruction", "progress", "rgb_features", "depth_features"]
        assert g[0]["rgb_features"].shape[1:] == (8, 2, 2) and g[0]["instruction"].shape[1:] == (10,)
    for g, w in zip(got_left, want_left):
        assert (g is None) == (w is None)
        if w is not None:
            _assert_same_episode(g, w)
    # what the read half makes of them
    a = data_path.collate_trajectories(got, "cpu", inflection_coef=3.2)
    b = data_path.collate_trajectories(want, "cpu", inflection_coef=3.2)
    assert list(a[0]) == list(b[0])
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    for x, y in zip(a[1:], b[1:]):
        assert x.dtype == y.dtype and torch.equal(x, y)


def test_popped_arrays_own_their_memory_and_lengths_reset(monkeypatch):
    monkeypatch.setattr(_lib, "_LIB", hostsim_traj.HostSimTraj())
    rec = data_path.TrajectoryRecorder(2, "cpu", True, capacity=4)
    for step in range(3):
        rec.append({"x": torch.full((2, 3), float(step))}, torch.zeros(2, 1, dtype=torch.long),
                   torch.ones(2, 1, dtype=torch.long))
    (first,) = rec.pop([1])
    assert rec.lengths() == [3, 0]
    rec.append({"x": torch.full((2, 3), 9.0)}, torch.zeros(2, 1, dtype=torch.long),
               torch.ones(2, 1, dtype=torch.long))
    assert first[0]["x"][:, 0].tolist() == [0.0, 1.0, 2.0]     # not a view of the arena
    rec.discard([0])
    assert rec.lengths() == [0, 1]
    with pytest.raises(RuntimeError, match="sensors"):
        rec.append({"y": torch.zeros(2, 3)}, torch.zeros(2, 1, dtype=torch.long),
                   torch.ones(2, 1, dtype=torch.long))
    hook = rec.feature_hook("late_features")
    del hook
    with pytest.raises(RuntimeError, match="has not fired"):
        rec.append({"x": torch.zeros(2, 3)}, torch.zeros(2, 1, dtype=torch.long),
                   torch.ones(2, 1, dtype=torch.long))


# ------------------------------------------------------------------ dagger_step
@pytest.mark.parametrize("expert_dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("n", [1, 7])
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
def test_dagger_step_matches_the_torch_where_restatement(monkeypatch, beta, n, expert_dtype):
    monkeypatch.setattr(_lib, "_LIB", hostsim_traj.HostSimTraj())
    g = torch.Generator().manual_seed(n)
    actions = torch.randint(0, 4, (n, 1), generator=g)
    expert = torch.randint(0, 4, (n, 1), generator=g)
    expert[::3] = -1
    expert = expert.to(expert_dtype)
    # dagger_trainer.py:414-444
    torch.manual_seed(17)
    want = torch.where(torch.rand_like(actions, dtype=torch.float) < beta, expert.long(), actions)
    skips = expert.long() == -1
    want = torch.where(skips, torch.zeros_like(want), want)
    prev = torch.full((n, 1), 3, dtype=torch.long)
    storage = prev.data_ptr()
    torch.manual_seed(17)
    got, ints, skipped = data_path.dagger_step(actions, expert, beta, prev)
    assert got.shape == actions.shape and got.dtype == torch.int64 and torch.equal(got, want)
    assert prev.data_ptr() == storage and torch.equal(prev, want)
    assert ints == [a[0].item() for a in want] and all(type(v) is int for v in ints)
    assert skipped == skips.squeeze(-1).tolist() and all(type(v) is bool for v in skipped)
