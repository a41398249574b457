"""DAgger rollout collection on the device (csrc/traj.hip): vlnce_traj_append and
vlnce_dagger_mix_actions against numpy / torch, and data_path.TrajectoryRecorder behind the real
CMA policy against the reference-shaped `o.cpu()` hooks.  Every comparison is bit for bit (NaN by
isnan): the kernels convert the values numpy's astype converts (pinned on the CPU tier by
tests/test_traj_recorder.py::test_numpy_narrows_as_the_kernel_tests_assume)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

import vlnce_amd  # noqa: E402
from oracle import policy_cpu as oc  # noqa: E402
from oracle import thirdparty as tp  # noqa: E402
from vlnce_amd import data_path, ops  # noqa: E402

DEV = "cuda:0"
SENTINEL = 0x5A
SPECIAL_F32 = [65520.0, 65519.996, 2.0 ** -25, 1.0001 * 2.0 ** -25, 1.0 + 2.0 ** -11,
               1.0 + 3 * 2.0 ** -11, -0.0, float("inf"), float("-inf"), float("nan"), -65520.0,
               6.1e-5, 5.9e-8, -2.0 ** -25, 3.0e38]
SPECIAL_I64 = [2049, 2051, 2503, 65520, 65519, 2 ** 24 + 1, -1, -2049, 2 ** 40, -(2 ** 40), 0]
_NP = {torch.float16: np.float16, torch.float32: np.float32, torch.int64: np.int64}
# source kind -> storage dtypes; "f32i" = float32 holding finite values (the cast to int64
# truncates them; what it makes of NaN or infinity is nobody's contract)
PAIRS = [("f32", torch.float16), ("f32", torch.float32), ("f32i", torch.int64),
         ("i64", torch.float16), ("i64", torch.float32), ("i64", torch.int64),
         ("u8", torch.float16), ("u8", torch.float32), ("u8", torch.int64)]


def same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def _values(n, D, seed):
    """logical rows [n, D] per source kind, random with the rounding cases in front"""
    rng = np.random.RandomState(seed)
    f32 = (rng.randn(n, D) * rng.choice([1e-6, 1.0, 300.0, 4e4], size=(n, D))).astype(np.float32)
    k = min(f32.size, len(SPECIAL_F32))
    f32.reshape(-1)[:k] = np.array(SPECIAL_F32[:k], dtype=np.float32)
    if n > 1:   # ... and at a row's end, where a write past D would land
        f32[-1, -min(D, 4):] = np.array(SPECIAL_F32[:min(D, 4)], dtype=np.float32)
    i64 = rng.randint(-3000, 3000, size=(n, D)).astype(np.int64)
    k = min(i64.size, len(SPECIAL_I64))
    i64.reshape(-1)[:k] = SPECIAL_I64[:k]
    return {"f32": f32, "f32i": (rng.rand(n, D) * 2000 - 1000).astype(np.float32), "i64": i64,
            "u8": rng.randint(0, 256, size=(n, D)).astype(np.uint8)}


def _expected(rows, dst_dtype):
    with np.errstate(over="ignore", invalid="ignore"):
        if dst_dtype == torch.float16:
            rows = rows.astype(np.float32)   # batch_obs casts to float, astype then narrows
        return rows.astype(_NP[dst_dtype])


def _layout(rows, C, P, layout):
    """the logical [n, C, P] rows as a device tensor laid out one of four ways"""
    n = rows.shape[0]
    t = torch.from_numpy(rows).view(n, C, P)
    if layout == "nhwc":            # what the trunks hand the hook: memory [n, P, C]
        return t.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1)
    if layout == "contiguous":
        return t.contiguous().to(DEV)
    lead = 3 if layout == "slice" else 4   # misaligned start | aligned start, row stride > D
    wide = torch.zeros((n, C * P + 9), dtype=t.dtype)
    wide[:, lead:lead + C * P] = t.reshape(n, -1)
    return wide.to(DEV)[:, lead:lead + C * P].unflatten(1, (C, P))


@pytest.mark.parametrize("n", [1, 5, 130])
@pytest.mark.parametrize("C,P", [(2048, 16), (128, 16), (40, 4), (7, 1), (1, 1), (200, 1)])
def test_traj_append_every_path_dtype_and_layout(C, P, n):
    lib = ops.L()
    D = C * P
    vals = _values(n, D, seed=C * 31 + P + n)
    want = [_expected(vals[kind], dt) for kind, dt in PAIRS]      # once, shared by the layouts
    num_envs, capacity = n + 3, 3
    rng = np.random.RandomState(n)
    slots = [int(s) for s in rng.permutation(num_envs)[:n]]        # not the identity, with gaps
    steps = [(2 * r + 1) % capacity for r in range(n)]
    assert n == 1 or (slots != sorted(slots) and len(set(steps)) > 1)
    si, ti = torch.tensor(slots, device=DEV), torch.tensor(steps, device=DEV)
    for layout in ("nhwc", "contiguous", "slice", "slice_aligned"):
        sources = [_layout(vals[kind], C, P, layout) for kind, _ in PAIRS]
        arenas = [torch.full((num_envs, capacity, D * torch.empty((), dtype=dt).element_size()),
                             SENTINEL, dtype=torch.uint8, device=DEV).view(dt) for _, dt in PAIRS]
        assert all(a.shape == (num_envs, capacity, D) for a in arenas)
        lib.traj_append(sources, arenas, slots, steps)            # 9 sensors: two launches per 128 rows
        torch.cuda.synchronize()
        for (kind, dt), arena, w in zip(PAIRS, arenas, want):
            got = arena[si, ti].cpu().numpy()
            assert same_bits(got, w), (layout, kind, dt)
            # every cell no row addresses still holds the fill: nothing was written outside a
            # row, no vector store went past D
            raw = arena.view(torch.uint8)
            raw[si, ti] = SENTINEL
            assert bool((raw == SENTINEL).all()), (layout, kind, dt)


def test_traj_append_refuses_what_it_cannot_address():
    lib = ops.L()
    src = torch.zeros(2, 8, device=DEV)
    arena = torch.zeros(4, 3, 8, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match="outside the arena"):
        lib.traj_append([src], [arena], [0, 1], [0, 3])            # step == capacity
    with pytest.raises(RuntimeError, match="slot outside"):
        lib.traj_append([src], [arena], [0, 4], [0, 0])
    with pytest.raises(RuntimeError, match="not a recorded pair"):
        lib.traj_append([src.half()], [arena], [0, 1], [0, 0])
    with pytest.raises(RuntimeError, match="arena"):
        lib.traj_append([src], [arena[:, :, :4]], [0, 1], [0, 0])


def test_traj_append_entry_point_refuses_more_than_it_takes_per_call():
    """the binding splits larger requests; the C entry point itself must refuse them"""
    import ctypes

    from vlnce_amd._lib import TrajSensor

    lib = ops.L()
    ints = (ctypes.c_int * 129)()
    for n_sensors, n_rows, what in ((9, 1, "9 sensors"), (1, 129, "129 rows"), (0, 1, "0 sensors"),
                                    (1, 0, "0 rows")):
        rc = lib.dll.vlnce_traj_append((TrajSensor * 9)(), n_sensors, ints, ints, n_rows, 4, None)
        assert rc != 0 and what in lib.dll.vlnce_last_error().decode(), (n_sensors, n_rows)


def test_traj_append_offsets_beyond_32_bits():
    """a 64-environment fp16 arena of 1024 steps of rgb + depth features is 4.6 GB: rows at its two
    ends in one call"""
    free, _ = torch.cuda.mem_get_info()
    if free < 8 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the 4.6 GB arena wants 8")
    lib = ops.L()
    num_envs, capacity, D = 64, 1024, 2048 * 16 + 128 * 16
    arena = torch.empty((num_envs, capacity, D), dtype=torch.float16, device=DEV)
    assert arena.numel() * 2 > 2 ** 32
    beside = [(0, 1), (1, 0), (63, 1022), (62, 1023), (32, 0), (31, 1023)]
    for s, t in beside + [(0, 0), (63, 1023)]:
        arena[s, t].view(torch.uint8).fill_(SENTINEL)
    rows = np.random.RandomState(0).randn(2, D).astype(np.float32)
    lib.traj_append([torch.from_numpy(rows).to(DEV)], [arena], [0, 63], [0, 1023])
    torch.cuda.synchronize()
    want = rows.astype(np.float16)
    assert same_bits(arena[0, 0].cpu().numpy(), want[0])
    assert same_bits(arena[63, 1023].cpu().numpy(), want[1])
    for s, t in beside:
        assert bool((arena[s, t].view(torch.uint8) == SENTINEL).all()), (s, t)


# ------------------------------------------------------------------ behind the real policy
def hook_builder(tgt_tensor):
    # verbatim shape of the reference's closure (dagger_trainer.py:296-300)
    def hook(m, i, o):
        tgt_tensor.set_(o.cpu())

    return hook


def _batch(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    obs = {"rgb": torch.randint(0, 256, (n, hw, hw, 3), generator=g).float(),
           "depth": torch.rand(n, hw, hw, 1, generator=g),
           "instruction": torch.zeros(n, 200, dtype=torch.long)}
    obs["instruction"][:, :11] = torch.randint(1, 2504, (n, 11), generator=g)
    return obs


@pytest.mark.parametrize("n", [2, 64])   # the hook test's geometry, and a collection run's width
@pytest.mark.parametrize("mode", ["plain", "encode_ahead", "act_graph"])
def test_recorder_stores_what_the_reference_hooks_capture(mode, n, monkeypatch):
    hw = 256
    if mode == "act_graph":
        monkeypatch.setenv("VLNCE_ACT_GRAPH", "1")
    torch.manual_seed(0)
    policy = vlnce_amd.build_model(vlnce_amd.make_config("CMAPolicy"), *vlnce_amd.make_spaces(hw, hw))
    ref = oc.build_model(tp.make_config("CMAPolicy"), *tp.make_spaces(hw, hw))
    policy.load_state_dict(tp.synth_state_dict(ref))
    policy.to(DEV)
    recs = {fp16: data_path.TrajectoryRecorder(n, DEV, fp16, capacity=2) for fp16 in (True, False)}
    rgb_f, dep_f = torch.zeros((1,)), torch.zeros((1,))
    cnn, venc = policy.net.rgb_encoder.cnn, policy.net.depth_encoder.visual_encoder
    hooks = [cnn.register_forward_hook(hook_builder(rgb_f)),
             venc.register_forward_hook(hook_builder(dep_f))]
    for rec in recs.values():
        hooks.append(cnn.register_forward_hook(rec.feature_hook("rgb_features")))
        hooks.append(venc.register_forward_hook(rec.feature_hook("depth_features")))
    states = torch.zeros(n, policy.net.num_recurrent_layers, 512, device=DEV)
    prev = torch.zeros(n, 1, dtype=torch.long, device=DEV)
    masks = torch.ones(n, 1, dtype=torch.uint8, device=DEV)
    captured, tokens, popped = [], [], {True: [], False: []}
    with torch.no_grad():
        for step in range(4):
            obs = _batch(n, hw, 100 + step)
            dobs = {k: v.to(DEV) for k, v in obs.items()}
            acting = policy.encode_ahead(dobs) if mode == "encode_ahead" else dobs
            policy.act(acting, states, prev, masks, deterministic=True)
            assert tuple(rgb_f.shape) == (n, 2048, 4, 4) and tuple(dep_f.shape) == (n, 128, 4, 4)
            captured.append((rgb_f.clone().numpy(), dep_f.clone().numpy()))
            tokens.append(obs["instruction"].numpy())
            oracle = torch.full((n, 1), step, dtype=torch.long, device=DEV)
            for rec in recs.values():
                rec.append(dobs, prev + step, oracle)
            if step == 1:
                for fp16, rec in recs.items():
                    popped[fp16] += rec.pop([1])
    for fp16, rec in recs.items():
        popped[fp16] += rec.pop(range(n))
    for h in hooks:
        h.remove()
    # episodes: environment 1 steps 0-1, then every environment in turn: steps 0-3, environment 1
    # steps 2-3
    episodes = [(1, [0, 1])] + [(i, [2, 3] if i == 1 else [0, 1, 2, 3]) for i in range(n)]
    for fp16 in (True, False):
        dt = np.float16 if fp16 else np.float32
        assert len(popped[fp16]) == n + 1
        for (env, steps), (ep_obs, ep_prev, ep_oracle) in zip(episodes, popped[fp16]):
            assert list(ep_obs) == ["instruction", "rgb_features", "depth_features"]
            for key, idx in (("rgb_features", 0), ("depth_features", 1)):
                want = np.stack([captured[s][idx][env] for s in steps]).astype(dt)
                assert same_bits(ep_obs[key], want), (mode, n, fp16, key, env)
            want = np.stack([tokens[s][env] for s in steps]).astype(np.float32).astype(dt)
            assert same_bits(ep_obs["instruction"], want)
            assert ep_prev.dtype == np.int64 and ep_prev.tolist() == steps
            assert ep_oracle.dtype == np.int64 and ep_oracle.tolist() == steps


# ------------------------------------------------------------------ dagger_step
@pytest.mark.parametrize("expert_dtype", [torch.float32, torch.int64])
@pytest.mark.parametrize("n", [1, 64, 130])
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
def test_dagger_step_on_the_device(beta, n, expert_dtype):
    g = torch.Generator().manual_seed(n)
    actions = torch.randint(0, 4, (n, 1), generator=g).to(DEV)
    expert = torch.randint(0, 4, (n, 1), generator=g)
    expert[::3] = -1
    expert = expert.to(expert_dtype).to(DEV)
    # dagger_trainer.py:414-444
    torch.manual_seed(17)
    want = torch.where(torch.rand_like(actions, dtype=torch.float) < beta, expert.long(), actions)
    skips = expert.long() == -1
    want = torch.where(skips, torch.zeros_like(want), want)
    prev = torch.full((n, 1), 3, dtype=torch.long, device=DEV)
    storage = prev.data_ptr()
    torch.manual_seed(17)
    got, ints, skipped = data_path.dagger_step(actions, expert, beta, prev)
    assert got.is_cuda and got.shape == actions.shape and torch.equal(got, want)
    assert prev.data_ptr() == storage and torch.equal(prev, want)      # updated in place
    assert ints == want.view(-1).tolist() and skipped == skips.view(-1).tolist()
