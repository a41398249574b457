"""CPU tier of the trunk-feature cache of the Waypoint DD-PPO loop (ABI 155): the contract of
vlnce_waypoint_feature_pick / vlnce_waypoint_feature_rows restated in plain torch
(tests/waypoint_features_ref.py) on hand-built cases, the refusals of the real entry points (they are
made before anything is launched, so the library answers without a GPU), the agreement of header,
binding and exported symbols, and the host logic -- the net's cached path, the storage's validity
flags, act_for_rollout / bootstrap_value / wddppo_update -- through the tensor-level simulator.  The
kernels are held to the same restatement, bit for bit, by tests/test_waypoint_features_gpu.py."""
import os
import re

import pytest
import torch

import __graft_entry__ as ge
import cases
import rollout_cases as rc
import waypoint_features_ref as wf
from test_oracle_golden import compare
from vlnce_amd import _lib, ppo_harness
from vlnce_amd._lib import WpFeaturePickField, WpFeatureRowsField
from vlnce_amd.ppo_harness import PPOConfig, wddppo_minibatch_update, wddppo_update
from vlnce_amd.rollout_storage import FRAME_KEYS, ActionDictRolloutStorage

torch.distributions.Distribution.set_default_validate_args(False)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "vlnce_hip.h")


# ---- the restatement on hand-built cases
def test_feature_pick_restatement():
    src = torch.arange(2 * 3 * 2, dtype=torch.float32).view(2, 3, 2)       # [B=2, P=3, F=2]
    zero = torch.tensor([-1.0, -2.0])
    got = wf.feature_pick_ref(src, zero, torch.tensor([2, 0]))
    assert got.tolist() == [[4.0, 5.0], [6.0, 7.0]]
    got = wf.feature_pick_ref(src, zero, torch.tensor([3, -1]))            # STOP (P) and a negative
    assert got.tolist() == [[-1.0, -2.0], [-1.0, -2.0]]
    got = wf.feature_pick_ref(src, zero, torch.tensor([[1], [6]]))         # [B, 1] as act() hands it
    assert got.tolist() == [[2.0, 3.0], [-1.0, -2.0]]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32])
def test_feature_rows_restatement(dtype):
    pano = torch.arange(2 * 2 * 3, dtype=torch.float32).view(2, 2, 3)      # [B=2, P=2, F=3]
    hist = torch.tensor([[100.0, 101.0, 102.0], [200.0, 201.0, 202.0]])
    zero = torch.tensor([-1.0, -2.0, -3.0])
    got = wf.feature_rows_ref(pano, hist, zero, torch.tensor([[1], [0]]).to(dtype))
    assert got.shape == (2, 3, 3)
    assert got[0].tolist() == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0], [100.0, 101.0, 102.0]]
    assert got[1].tolist() == [[6.0, 7.0, 8.0], [9.0, 10.0, 11.0], [-1.0, -2.0, -3.0]]


# ---- header, binding, symbols
def test_header_binding_and_version_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(vlnce_[a-z0-9_]+)\s*\(", text))
    for name in ("vlnce_waypoint_feature_pick", "vlnce_waypoint_feature_rows"):
        assert name in declared and name in _lib.exported_symbols()
    assert _lib.HipLib.ABI == 155
    assert "#define VLNCE_WP_FEATURE_MAX_FIELDS 8" in text and _lib.WP_FEATURE_MAX_FIELDS == 8
    # the structs of the binding follow the header's member order
    for struct, cls in (("vlnce_wp_feature_pick_field", WpFeaturePickField),
                        ("vlnce_wp_feature_rows_field", WpFeatureRowsField)):
        body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", text).group(1)
        members = re.findall(r"(\w+);", body)
        assert members == [n for n, _ in cls._fields_], struct


@pytest.fixture(scope="module")
def dll():
    if not os.path.exists(ge.HIPCC) and not os.path.exists(ge.OUT):
        pytest.skip("no hipcc and no prebuilt library")
    ge.build()
    lib = _lib.HipLib()      # loads without a GPU; checks the ABI
    assert lib.dll.vlnce_version() == 155
    return lib.dll


def test_library_exports_both_entry_points(dll):
    for name in ("vlnce_waypoint_feature_pick", "vlnce_waypoint_feature_rows"):
        assert hasattr(dll, name), name


A = 0x10000   # a non-null, 16-byte aligned address; a refused call reads nothing behind it


def pick_field(**kw):
    f = dict(src=A, zero=A, dst=A, F=8, src_row_stride=96)
    f.update(kw)
    return WpFeaturePickField(**f)


def rows_field(**kw):
    f = dict(pano=A, hist=A, zero=A, out=A, F=8, pano_row_stride=96, hist_row_stride=8)
    f.update(kw)
    return WpFeatureRowsField(**f)


PICK_REFUSALS = [
    ("null-pano", dict(pano=None), "bad argument"),
    ("B-0", dict(B=0), "bad argument"),
    ("P-0", dict(P=0), "bad argument"),
    ("no-fields", dict(n=0), "0 fields"),
    ("nine-fields", dict(n=9), "9 fields"),
    ("null-src", dict(field=dict(src=None)), "null pointer"),
    ("null-zero", dict(field=dict(zero=None)), "null pointer"),
    ("null-dst", dict(field=dict(dst=None)), "null pointer"),
    ("F-0", dict(field=dict(F=0)), "F = 0"),
    ("F-negative", dict(field=dict(F=-4)), "F = -4"),
    ("short-stride", dict(field=dict(src_row_stride=95)), "row stride 95"),
    ("misaligned", dict(field=dict(dst=A + 2)), "misaligned"),
]


@pytest.mark.parametrize("what,kw,message", PICK_REFUSALS, ids=[r[0] for r in PICK_REFUSALS])
def test_feature_pick_refuses_before_it_launches(dll, what, kw, message):
    n = kw.get("n", 1)
    arr = (WpFeaturePickField * max(n, 1))(*[pick_field(**kw.get("field", {})) for _ in range(max(n, 1))])
    rc_ = dll.vlnce_waypoint_feature_pick(arr, n, kw.get("pano", A), kw.get("B", 2), kw.get("P", 12), None)
    assert rc_ == 1, what           # (2 would be a launch that failed)
    text = dll.vlnce_last_error().decode()
    assert "waypoint_feature_pick" in text and message in text, text


def test_feature_pick_refuses_a_null_table(dll):
    assert dll.vlnce_waypoint_feature_pick(None, 1, A, 2, 12, None) == 1
    assert "waypoint_feature_pick" in dll.vlnce_last_error().decode()


ROWS_REFUSALS = [
    ("null-masks", dict(masks=None), "bad argument"),
    ("B-0", dict(B=0), "bad argument"),
    ("P-negative", dict(P=-1), "bad argument"),
    ("mask-dtype", dict(mask_dtype=2), "masks of dtype 2"),
    ("misaligned-f32-masks", dict(masks=A + 1, mask_dtype=0), "misaligned masks"),
    ("no-fields", dict(n=0), "0 fields"),
    ("nine-fields", dict(n=9), "9 fields"),
    ("null-pano", dict(field=dict(pano=None)), "null pointer"),
    ("null-hist", dict(field=dict(hist=None)), "null pointer"),
    ("null-zero", dict(field=dict(zero=None)), "null pointer"),
    ("null-out", dict(field=dict(out=None)), "null pointer"),
    ("F-0", dict(field=dict(F=0)), "F = 0"),
    ("short-pano-stride", dict(field=dict(pano_row_stride=95)), "row strides 95 / 8"),
    ("short-hist-stride", dict(field=dict(hist_row_stride=7)), "row strides 96 / 7"),
    ("misaligned", dict(field=dict(hist=A + 3)), "misaligned pointer"),
]


@pytest.mark.parametrize("what,kw,message", ROWS_REFUSALS, ids=[r[0] for r in ROWS_REFUSALS])
def test_feature_rows_refuses_before_it_launches(dll, what, kw, message):
    n = kw.get("n", 1)
    arr = (WpFeatureRowsField * max(n, 1))(*[rows_field(**kw.get("field", {})) for _ in range(max(n, 1))])
    rc_ = dll.vlnce_waypoint_feature_rows(arr, n, kw.get("masks", A), kw.get("mask_dtype", 3),
                                          kw.get("B", 2), kw.get("P", 12), None)
    assert rc_ == 1, what
    text = dll.vlnce_last_error().decode()
    assert "waypoint_feature_rows" in text and message in text, text


def test_feature_rows_refuses_a_null_table(dll):
    assert dll.vlnce_waypoint_feature_rows(None, 1, A, 3, 2, 12, None) == 1
    assert "waypoint_feature_rows" in dll.vlnce_last_error().decode()


# ---- the storage's arenas and flags (no policy)
SHAPES = {"rgb": (2, 2, 5), "depth": (1, 1, 6)}


def small_storage(sim, steps=0, **kw):
    sensors = dict(rc.SENSORS, rgb_history=rc.SENSORS["rgb"][1:], depth_history=rc.SENSORS["depth"][1:])
    st = ActionDictRolloutStorage(rc.NUM_STEPS, rc.N, rc.space(sensors), rc.H, num_recurrent_layers=rc.L,
                                  **kw)
    g = torch.Generator().manual_seed(5)
    for i in range(steps):
        obs = {k: torch.randn(rc.N, *s, generator=g) for k, s in sensors.items()}
        if st.has_trunk_features:
            for s, shape in SHAPES.items():
                obs[s + "_history_features"] = torch.randn(rc.N, *shape, generator=g)
        action = {k: torch.rand(rc.N, 1, generator=g) for k in rc.ACTION_KEYS}
        action["pano"] = torch.randint(0, 12, (rc.N, 1), generator=g)
        st.insert(obs, torch.randn(rc.N, rc.L, rc.H, generator=g), action, -torch.rand(rc.N, 1, generator=g),
                  torch.randn(rc.N, 1, generator=g), torch.randn(rc.N, 1, generator=g),
                  torch.ones(rc.N, 1))
    return st


@pytest.fixture
def sim(monkeypatch):
    s = wf.FeatureSim()
    monkeypatch.setattr(_lib, "_LIB", s)
    return s


def test_storage_without_the_argument_is_unchanged(sim):
    st = small_storage(sim, steps=2)
    assert not st.has_trunk_features and not any("features" in k and k != "angle_features"
                                                 for k in st.observations)
    with pytest.raises(AssertionError, match="frames=False"):
        next(st.recurrent_generator(st.get_advantages(), 2, frames=False))
    rc.replay("cont", "cpu", ActionDictRolloutStorage)   # the reference's bits, as before


def test_arenas_flags_and_the_frameless_generator(sim):
    st = small_storage(sim, trunk_features=SHAPES)
    T, n, P = rc.NUM_STEPS, rc.N, 2
    assert st.observations["rgb_features"].shape == (T + 1, n, P, 2, 2, 5)
    assert st.observations["depth_features"].shape == (T + 1, n, P, 1, 1, 6)
    assert st.observations["rgb_history_features"].shape == (T + 1, n, 2, 2, 5)
    assert st.observations["depth_history_features"].shape == (T + 1, n, 1, 1, 6)
    assert st.trunk_valid == [False] * (T + 1) and st.trunk_key is None
    g = torch.Generator().manual_seed(1)
    filled = small_storage(sim, steps=3, trunk_features=SHAPES)
    for k in ("rgb_features", "depth_features"):
        filled.observations[k].copy_(torch.randn(filled.observations[k].shape, generator=g))
    filled.trunk_valid = [True, False, True, True]
    filled.trunk_key = "k"
    # insert clears the row it writes
    two = small_storage(sim, steps=0, trunk_features=SHAPES)
    two.trunk_valid = [True] * (T + 1)
    rc.insert_step(two, dict(obs={}, hidden=torch.zeros(n, rc.L, rc.H),
                             action={k: torch.zeros(n, 1) for k in rc.ACTION_KEYS}, logp=torch.zeros(n, 1),
                             value=torch.zeros(n, 1), reward=torch.zeros(n, 1), mask=torch.ones(n, 1)), "cpu")
    assert two.trunk_valid == [True, False, True, True]
    # rows [0, step) decide
    assert not filled.trunk_rows_valid("k")
    filled.trunk_valid[1] = True
    assert filled.trunk_rows_valid("k") and not filled.trunk_rows_valid("other")
    # the generator without frames: the feature arenas' rows, no frame key, one gather
    adv = filled.get_advantages()
    perm = torch.tensor([2, 0, 3, 1])
    sim.calls.clear()
    with rc.fixed_randperm([perm]):
        batches = list(filled.recurrent_generator(adv, 2, frames=False))
    assert sim.names() == ["rollout_gather"] * 2
    with rc.fixed_randperm([perm]):
        full = list(filled.recurrent_generator(adv, 2))
    for m, (sample, whole) in enumerate(zip(batches, full)):
        envs = perm[2 * m:2 * m + 2]
        assert set(sample[0]) == set(filled.observations) - set(FRAME_KEYS)
        for k, v in sample[0].items():
            want = filled.observations[k][:3][:, envs]
            assert torch.equal(v, want.reshape(6, *want.shape[2:])), k
            assert torch.equal(v, whole[0][k]), k
        for a, b in zip(sample[1:], whole[1:]):
            if isinstance(a, dict):
                assert all(torch.equal(a[k], b[k]) for k in a)
            else:
                assert torch.equal(a, b)
    # after_update carries the flag with the row
    filled.trunk_valid = [True, True, True, False]
    last = {k: v[3].clone() for k, v in filled.observations.items()}
    filled.after_update()
    assert filled.trunk_valid == [False, False, False, False] and filled.step == 0
    for k, v in last.items():
        assert torch.equal(filled.observations[k][0], v), k
    filled.step = 2
    filled.trunk_valid = [False, True, True, False]
    filled.after_update()
    assert filled.trunk_valid == [True, False, False, False]


# ---- the net and the loop on the simulator (64-pixel sensors, 2 environments)
@pytest.fixture(scope="module")
def collected():
    """(policy, storage, panorama choices, trunk calls during collection) of waypoint_features_ref.collect"""
    sim = wf.FeatureSim()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "_LIB", sim)
        policy = wf.build_policy("cpu")
        with wf.TrunkCounter(policy.net) as counter:
            st, panos = wf.collect(policy, "cpu")
        return policy, st, panos, counter.calls, list(sim.names())


def test_golden_through_the_cache_on_the_simulator(sim):
    """the reference's own WDDPPO.update fixture with the four feature keys and without a frame"""
    name = "waypoint_ppo_update_64"
    case = cases.CASES[name]
    obs, prev, masks, extra, gold = cases.load_case(os.path.join(wf.GOLD, name + ".npz"))
    policy = wf.build_policy("cpu", name)
    net = policy.net
    feats = {}
    for s in wf.SENSORS:
        feats[s + "_features"] = net._trunk_rows(s, obs[s])
        feats[s + "_history_features"] = net._trunk_rows(s, obs[s + "_history"])
    cached = {k: v for k, v in obs.items() if k not in FRAME_KEYS}
    cached.update(feats)

    def ppo(pol, sample):
        with wf.TrunkCounter(pol.net) as counter:
            stats = wddppo_minibatch_update(pol, None, sample, PPOConfig(**cases.PPO), step_grad=False,
                                            clip_grads=False)
        assert counter.calls == 0
        return [float(v) for v in stats]

    for s in wf.SENSORS:               # the zero frame's features are made once, outside the update
        net.trunk_zero(s, obs[s].shape[-3:], "cpu")
    outs = cases.run_case(policy, case, cached, prev, masks, extra, None, None, ppo_fn=ppo)
    compare(outs, gold, atol=1e-4, rtol=1e-4)
    assert sim.names().count("waypoint_feature_rows") == 1


def test_collection_stores_what_the_update_needs(collected):
    policy, st, panos, trunk_calls, names = collected
    T, N, P = wf.T, wf.N, wf.P
    # per step one trunk call per sensor over the panorama; the bootstrap row's too; the two zero frames
    assert trunk_calls == 2 * (T + 1) + 2
    assert names.count("waypoint_feature_pick") == T and names.count("waypoint_feature_rows") == T + 1
    assert st.trunk_valid == [True] * (T + 1) and st.trunk_key == policy.net.trunk_cache_key()
    assert int(panos[wf.STOP_AT[0]][wf.STOP_AT[1]]) == P
    for s in wf.SENSORS:
        zero = policy.net.trunk_zero(s, st.observations[s].shape[-3:], "cpu")
        feats, hist = st.observations[s + "_features"], st.observations[s + "_history_features"]
        for t in range(T):
            for i in range(N):
                p = int(panos[t][i])
                want = feats[t][i, p] if p < P else zero
                assert torch.equal(hist[t + 1][i], want), (s, t, i)
        assert float(zero.abs().sum()) > 0.0
    assert float(st.masks[wf.DONE_AT[0]][wf.DONE_AT[1]]) == 0.0


def test_row_zero_after_after_update_needs_no_trunk(collected, sim):
    policy, st, _, _, _ = collected
    st = wf.copied(st)
    row_T = {k: v[wf.T].clone() for k, v in st.observations.items()}
    st.after_update()
    assert st.trunk_valid == [True] + [False] * wf.T
    for k, v in row_T.items():
        assert torch.equal(st.observations[k][0], v), k
    with wf.TrunkCounter(policy.net) as counter:
        _, history, _ = ppo_harness.act_for_rollout(policy, st)
    assert counter.calls == 0
    assert set(history) == {"rgb", "depth", "rgb_history_features", "depth_history_features"}


def updated(st, perms, **kw):
    policy = wf.warm_zero(wf.build_policy("cpu"), st)
    cfg = PPOConfig(**cases.PPO)
    opt = torch.optim.Adam([p for p in policy.parameters() if p.requires_grad], lr=2.5e-4, eps=1e-5)
    with rc.fixed_randperm(perms), wf.TrunkCounter(policy.net) as counter:
        stats = wddppo_update(policy, opt, st, cfg, ppo_epoch=2, num_mini_batch=2, **kw)
    return policy, stats, counter.calls


def test_update_from_the_cache_equals_the_update_from_frames(collected, sim):
    policy, st, _, _, _ = collected
    perms = [torch.tensor([1, 0]), torch.tensor([0, 1])]
    a, stats_a, calls_a = updated(st, perms, use_trunk_cache=True)
    b, stats_b, calls_b = updated(st, perms, use_trunk_cache=False)
    assert calls_a == 0 and calls_b == 2 * 4      # two sensors, 2 epochs x 2 minibatches
    assert torch.allclose(torch.tensor(stats_a), torch.tensor(stats_b), rtol=1e-4, atol=1e-5)
    moved = 0
    for (n, p), q, r in zip(a.named_parameters(), b.parameters(), policy.parameters()):
        assert torch.allclose(p, q, rtol=1e-4, atol=1e-5), n
        moved += int(not torch.equal(p, r))
    assert moved > 0
    _, stats_c, calls_c = updated(st, perms)      # None: the cache, when it can
    assert calls_c == 0 and stats_c == stats_a


def spoil_version(policy, sim):
    policy.net.rgb_encoder.cnn[0].weight.data.mul_(1.0)   # (.data: no version bump)
    with torch.no_grad():
        policy.net.depth_encoder.visual_encoder.backbone.conv1[0].weight.mul_(1.0)
    return "depth_encoder.*parameter versions"


def spoil_plane_format(policy, sim):
    sim.plane_format = lambda options=None: 1
    return "rgb_encoder.*plane format"


def spoil_bn_mode(policy, sim):
    policy.net.rgb_encoder.train()
    return "BatchNorm of rgb_encoder is in training mode"


def spoil_gn_mode(policy, sim):
    policy.net.depth_encoder.train()
    return "depth_encoder.*norm layers in eval mode"


def spoil_requires_grad(policy, sim):
    next(iter(policy.net.depth_encoder.visual_encoder.parameters())).requires_grad_(True)
    return "depth_encoder requires grad"


@pytest.mark.parametrize("spoil", [spoil_version, spoil_plane_format, spoil_bn_mode, spoil_gn_mode,
                                   spoil_requires_grad], ids=lambda f: f.__name__)
def test_a_changed_key_raises_or_falls_back(collected, sim, spoil):
    _, st, _, _, _ = collected
    policy = wf.build_policy("cpu")
    message = spoil(policy, sim)
    cfg = PPOConfig(**cases.PPO)
    with pytest.raises(RuntimeError, match=message):
        wddppo_update(policy, None, st, cfg, ppo_epoch=1, num_mini_batch=2, use_trunk_cache=True)
    if spoil in (spoil_bn_mode, spoil_requires_grad):
        return   # (the frame path of these configurations is another test's subject)
    with wf.TrunkCounter(policy.net) as counter:
        stats = wddppo_update(policy, None, st, cfg, ppo_epoch=1, num_mini_batch=2)
    assert counter.calls == 2 * 2 and all(v == v for v in stats)      # fell back to the frames


def test_the_net_refuses_stale_features_itself(collected, sim):
    _, st, _, _, _ = collected
    policy = wf.build_policy("cpu")
    obs = {k: v[0] for k, v in st.observations.items()}
    obs["trunk_feature_key"] = st.trunk_key
    args = (st.recurrent_hidden_states[0], {k: v[0] for k, v in st.prev_actions.items()}, st.masks[0])
    with torch.no_grad():
        policy.get_value(dict(obs), args[0], dict(args[1]), args[2])
        with torch.no_grad():
            policy.net.rgb_encoder.cnn[0].weight.add_(0.0)
        with pytest.raises(RuntimeError, match="rgb_encoder.*another key"):
            policy.get_value(dict(obs), args[0], dict(args[1]), args[2])


def test_missing_rows_and_missing_arenas(collected, sim):
    policy, st, _, _, _ = collected
    cfg = PPOConfig(**cases.PPO)
    holed = wf.copied(st)
    holed.trunk_valid[1] = False
    with pytest.raises(RuntimeError, match=r"rows \[1\]"):
        wddppo_update(policy, None, holed, cfg, ppo_epoch=1, num_mini_batch=2,
                      use_trunk_cache=True)
    plain = small_storage(sim, steps=1)
    with pytest.raises(RuntimeError, match="no feature arenas"):
        wddppo_update(policy, None, plain, cfg, ppo_epoch=1, num_mini_batch=2, use_trunk_cache=True)


@pytest.mark.parametrize("fused", [True, False], ids=["fused-act", "default-act"])
def test_feature_history_with_either_act_path(sim, fused):
    """act_for_rollout hands out the feature history whichever path act() takes: the pick reads the
    choice on the device either way"""
    policy = wf.build_policy("cpu")
    with wf.TrunkCounter(policy.net):
        st, panos = wf.collect(policy, "cpu", fused_act=fused)
    assert ("waypoint_act" in sim.names()) == fused
    assert sim.names().count("waypoint_feature_pick") == wf.T
    feats, hist = st.observations["depth_features"], st.observations["depth_history_features"]
    zero = policy.net.trunk_zero("depth", st.observations["depth"].shape[-3:], "cpu")
    for t in range(wf.T):
        for i in range(wf.N):
            p = int(panos[t][i])
            assert torch.equal(hist[t + 1][i], feats[t][i, p] if p < wf.P else zero), (t, i)
