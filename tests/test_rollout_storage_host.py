"""CPU tier: the host side of the device rollout storage (vlnce_amd.ActionDictRolloutStorage,
ppo_harness.wddppo_update) run through a tensor-level simulator of vlnce_rollout_copy /
vlnce_rollout_gather / vlnce_ppo_advantages.  `RolloutSim` below IS their written contract, in plain
torch.  The kernels are held to the same contract, bit for bit against torch indexing, by
tests/test_rollout_storage_gpu.py."""
import copy

import pytest
import torch
import torch.nn as nn

import hostsim
import rollout_cases as rc
import vlnce_amd
from vlnce_amd import _lib
from vlnce_amd.ppo_harness import PPOConfig, wddppo_minibatch_update, wddppo_update
from vlnce_amd.rollout_storage import ActionDictRolloutStorage

SUPPORTED = {(torch.float32, torch.float32), (torch.int64, torch.int64), (torch.uint8, torch.uint8),
             (torch.bool, torch.uint8), (torch.int64, torch.float32), (torch.uint8, torch.float32),
             (torch.bool, torch.float32), (torch.float32, torch.int64), (torch.float32, torch.uint8)}


class RolloutSim(hostsim.HostSim):
    def __init__(self, refuse=()):
        self.calls = []
        self.copies = []    # the fields of every rollout_copy
        self.refuse = set(refuse)

    def rollout_copy_supported(self, src_dtype, dst_dtype):
        """contract of vlnce_rollout_copy_supported: exactly these pairs (a bool source is u8)"""
        return (src_dtype, dst_dtype) in SUPPORTED - self.refuse

    def rollout_copy(self, fields, n_rows):
        """contract of vlnce_rollout_copy: row r of every field, E contiguous elements from src + r *
        src_row_stride to dst + r * dst_row_stride, converted as Tensor.copy_ converts"""
        assert 1 <= len(fields) <= _lib.ROLLOUT_MAX_FIELDS and n_rows > 0
        self.calls.append(("rollout_copy", len(fields)))
        self.copies.append(list(fields))
        for f in fields:
            assert self.rollout_copy_supported(f.src.dtype, f.dst.dtype)
            assert f.E > 0 and f.src_row_stride >= 0 and f.dst_row_stride >= f.E
            src = torch.as_strided(f.src, (n_rows, f.E), (f.src_row_stride, 1))
            torch.as_strided(f.dst, (n_rows, f.E), (f.dst_row_stride, 1)).copy_(src)

    def rollout_gather(self, fields, envs, T):
        """contract of vlnce_rollout_gather: out[t, column + j] = arena[t, envs[j]] for t < T (t < 1
        where once), no conversion"""
        assert 1 <= len(fields) <= _lib.ROLLOUT_MAX_FIELDS and 1 <= len(envs) <= _lib.ROLLOUT_MAX_ENVS
        assert T > 0
        self.calls.append(("rollout_gather", len(fields), len(envs)))
        for f in fields:
            Tf = 1 if f.once else T
            assert f.arena.dtype == f.out.dtype and all(0 <= e < f.N for e in envs)
            arena = f.arena.reshape(-1, f.N, f.E)[:Tf]
            out = f.out.view(Tf, f.out_N, f.E)
            out[:, f.column:f.column + len(envs)] = arena[:, list(envs)]

    def ppo_advantages(self, returns, value_preds, adv, T, N, normalize, eps):
        """contract of vlnce_ppo_advantages: the fp32 difference; normalised with its mean and unbiased
        standard deviation in fp64, rounded once"""
        self.calls.append(("ppo_advantages", T, N))
        d = returns.reshape(-1)[:T * N] - value_preds.reshape(-1)[:T * N]
        if normalize:
            dd = d.double()
            d = ((dd - dd.mean()) / (dd.std() + float(torch.tensor(eps, dtype=torch.float32)))).float()
        adv.view(-1).copy_(d)

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture
def sim(monkeypatch):
    s = RolloutSim()
    monkeypatch.setattr(_lib, "_LIB", s)
    return s


def make_inputs(n, sensors=None, seed=0, discrete=False):
    g = torch.Generator().manual_seed(seed)
    sensors = rc.SENSORS if sensors is None else sensors
    action = {"pano": torch.randint(0, 12, (n, 1), generator=g)}
    for k in ("offset", "distance"):
        action[k] = torch.randint(0, 6, (n, 1), generator=g) if discrete else torch.rand(n, 1, generator=g)
    return dict(obs={k: torch.randn(n, *s, generator=g) for k, s in sensors.items()},
                hidden=torch.randn(n, rc.L, rc.H, generator=g), action=action,
                logp=-torch.rand(n, 1, generator=g), value=torch.randn(n, 1, generator=g),
                reward=torch.randn(n, 1, generator=g), mask=(torch.rand(n, 1, generator=g) > 0.3).float())


def filled(n, num_steps=3, steps=None, sensors=None, seed=0, **kw):
    st = ActionDictRolloutStorage(num_steps, n, rc.space(sensors), rc.H, num_recurrent_layers=rc.L, **kw)
    for i in range(num_steps if steps is None else steps):
        rc.insert_step(st, make_inputs(n, sensors, seed + i), "cpu")
    return st


def reference_insert(st, s, inputs):
    """rollout_storage.py:95-110 on the arenas of `st`, at step s"""
    for k, v in inputs["obs"].items():
        st.observations[k][s + 1].copy_(v)
    st.recurrent_hidden_states[s + 1].copy_(inputs["hidden"])
    for k, v in inputs["action"].items():
        st.actions[k][s].copy_(v)
        st.prev_actions[k][s + 1].copy_(v)
    st.action_log_probs[s].copy_(inputs["logp"])
    st.value_preds[s].copy_(inputs["value"])
    st.rewards[s].copy_(inputs["reward"])
    st.masks[s + 1].copy_(inputs["mask"])


def arenas(st):
    out = dict(st.observations)
    out.update({f"actions/{k}": v for k, v in st.actions.items()})
    out.update({f"prev_actions/{k}": v for k, v in st.prev_actions.items()})
    for a in ("recurrent_hidden_states", "rewards", "value_preds", "returns", "action_log_probs", "masks"):
        out[a] = getattr(st, a)
    return out


def assert_same_arenas(a, b):
    a, b = arenas(a), arenas(b)
    assert a.keys() == b.keys()
    for k in a:
        rc.same(a[k], b[k], k)


# ------------------------------------------------------------------ the reference's own results
@pytest.mark.parametrize("name", ["cont", "disc"])
def test_golden_variant_bit_for_bit(sim, name):
    st = rc.replay(name, "cpu", ActionDictRolloutStorage)
    assert st.prev_actions["pano"].dtype == torch.int64 and st.masks.dtype == torch.uint8
    for k in ("offset", "distance"):
        assert st.prev_actions[k].dtype == (torch.int64 if name == "disc" else torch.float32)
        assert st.actions[k].dtype == torch.float32


def test_exported_with_the_reference_signature_and_arenas():
    assert vlnce_amd.ActionDictRolloutStorage is ActionDictRolloutStorage
    st = ActionDictRolloutStorage(3, 4, rc.space(), 8, 2, False, True)
    assert st.num_steps == 3 and st.step == 0 and isinstance(st.step, int)
    assert st.observations["rgb"].shape == (4, 4, 2, 5, 7, 3)
    assert st.recurrent_hidden_states.shape == (4, 4, 2, 8)
    assert st.rewards.shape == st.action_log_probs.shape == st.actions["pano"].shape == (3, 4, 1)
    assert st.value_preds.shape == st.returns.shape == st.masks.shape == (4, 4, 1)
    assert st.prev_actions["offset"].dtype == torch.int64
    assert st.prev_actions["distance"].dtype == torch.float32
    assert all(v.dtype == torch.float32 for v in st.observations.values())


# ------------------------------------------------------------------ launches
def test_one_launch_each(sim):
    st = filled(4)
    assert sim.names() == ["rollout_copy"] * 3
    assert sim.calls[0] == ("rollout_copy", len(rc.SENSORS) + 1 + 6 + 4)
    sim.calls.clear()
    st.compute_returns(torch.zeros(4, 1), True, 0.99, 0.95)
    adv = st.get_advantages(True)
    assert sim.calls == [("ppo_advantages", 3, 4)] and adv.shape == (3, 4, 1)
    sim.calls.clear()
    assert len(list(st.recurrent_generator(adv, 2))) == 2
    assert sim.calls == [("rollout_gather", len(rc.SENSORS) + 1 + 6 + 5, 2)] * 2
    sim.calls.clear()
    st.after_update()
    assert sim.calls == [("rollout_copy", len(rc.SENSORS) + 2 + 3)] and st.step == 0
    st.after_update()   # step == 0: nothing to move
    assert len(sim.calls) == 1


def test_after_update_carries_the_last_row(sim):
    st = filled(4)
    before = {k: v.clone() for k, v in arenas(st).items()}
    st.after_update()
    for k, v in arenas(st).items():
        carried = k in rc.SENSORS or k.startswith("prev_actions") or k in ("recurrent_hidden_states",
                                                                            "masks")
        want = before[k].clone()
        if carried:
            want[0] = before[k][3]
        assert torch.equal(v, want), k


def test_unsupported_pair_goes_through_copy_(monkeypatch):
    s = RolloutSim(refuse={(torch.float32, torch.uint8)})
    monkeypatch.setattr(_lib, "_LIB", s)
    st, ref = filled(4, steps=0), filled(4, steps=0)
    inputs = make_inputs(4)
    inputs["obs"]["depth"] = inputs["obs"]["depth"].half()   # no kernel pair either
    rc.insert_step(st, inputs, "cpu")
    reference_insert(ref, 0, inputs)
    assert s.calls == [("rollout_copy", len(rc.SENSORS) + 1 + 6 + 4 - 2)]
    assert_same_arenas(st, ref)


def test_row_strided_source_is_read_in_place(sim):
    st, ref = filled(4, steps=0), filled(4, steps=0)
    inputs = make_inputs(4)
    wide = torch.randn(4, 3, *rc.SENSORS["rgb"])
    inputs["obs"]["rgb"] = wide[:, 1]                       # rows contiguous inside, row stride 3 E
    rc.insert_step(st, inputs, "cpu")
    reference_insert(ref, 0, inputs)
    f = sim.copies[0][0]
    assert f.src.data_ptr() == inputs["obs"]["rgb"].data_ptr() and f.E == 2 * 5 * 7 * 3
    assert f.src_row_stride == 3 * f.E and f.dst_row_stride == f.E
    assert_same_arenas(st, ref)


def test_source_not_contiguous_inside_is_made_contiguous(sim):
    st, ref = filled(4, steps=0), filled(4, steps=0)
    inputs = make_inputs(4)
    inputs["obs"]["angle_features"] = torch.randn(4, 4, 12).transpose(1, 2)   # [4, 12, 4], inner stride 12
    assert not inputs["obs"]["angle_features"].is_contiguous()
    rc.insert_step(st, inputs, "cpu")
    reference_insert(ref, 0, inputs)
    f = sim.copies[0][list(rc.SENSORS).index("angle_features")]
    assert f.src.is_contiguous() and f.src_row_stride == 48
    assert_same_arenas(st, ref)


def test_broadcast_and_host_sources_behave_as_copy_(sim):
    st, ref = filled(4, steps=0), filled(4, steps=0)
    inputs = make_inputs(4)
    inputs["reward"] = torch.tensor([[0.25]])               # broadcast over the environments
    rc.insert_step(st, inputs, "cpu")
    reference_insert(ref, 0, inputs)
    assert_same_arenas(st, ref)


def test_more_than_32_fields_split(sim):
    sensors = {f"s{i:02d}": (3,) for i in range(30)}
    st, ref = filled(3, steps=0, sensors=sensors), filled(3, steps=0, sensors=sensors)
    for s in range(3):
        inputs = make_inputs(3, sensors, seed=s)
        rc.insert_step(st, inputs, "cpu")
        reference_insert(ref, s, inputs)
    assert sim.calls == [("rollout_copy", 32), ("rollout_copy", 30 + 1 + 6 + 4 - 32)] * 3
    assert_same_arenas(st, ref)
    sim.calls.clear()
    adv = torch.randn(3, 3, 1)
    perm = torch.tensor([2, 0, 1])
    with rc.fixed_randperm([perm]):
        got = list(st.recurrent_generator(adv, 3))
    assert sim.calls == [("rollout_gather", 32, 1), ("rollout_gather", 30 + 1 + 6 + 5 - 32, 1)] * 3
    for sample, want in zip(got, rc.torch_minibatches(st, adv, 3, perm)):
        assert_same_sample(sample, want)
    sim.calls.clear()
    st.after_update()
    assert sim.calls == [("rollout_copy", 32), ("rollout_copy", 30 + 2 + 3 - 32)]


def assert_same_sample(got, want):
    for g, w in zip(got, want):
        if isinstance(w, dict):
            assert g.keys() == w.keys()
            for k in w:
                rc.same(g[k], w[k], k)
        else:
            rc.same(g, w, "sample")


def test_more_than_64_environments_split(sim):
    n = 70
    st = filled(n, num_steps=2, sensors={"depth": (3, 2)})
    adv = torch.randn(2, n, 1)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    sim.calls.clear()
    with rc.fixed_randperm([perm]):
        got = list(st.recurrent_generator(adv, 1))
    assert sim.calls == [("rollout_gather", 1 + 1 + 6 + 5, 64), ("rollout_gather", 1 + 1 + 6 + 5, 6)]
    (want,) = rc.torch_minibatches(st, adv, 1, perm)
    assert_same_sample(got[0], want)
    assert got[0][1].shape == (n, rc.L, rc.H) and got[0][0]["depth"].shape == (2 * n, 3, 2)


# ------------------------------------------------------------------ the generator's draw
def test_same_seed_same_draw_as_the_reference(sim):
    st = filled(8, sensors={"depth": (2,)})
    st.masks.zero_()
    st.value_preds[:, :, 0] = torch.arange(8.0)   # every environment carries its own index
    torch.manual_seed(123)
    want = torch.randperm(8)
    torch.manual_seed(123)
    got = torch.cat([sample[4][:2, 0] for sample in st.recurrent_generator(torch.zeros(3, 8, 1), 4)])
    assert got.long().tolist() == want.tolist()
    # exactly one draw, from torch's global generator: the next draw is the reference's next draw
    torch.manual_seed(123)
    list(st.recurrent_generator(torch.zeros(3, 8, 1), 4))
    after = torch.rand(3)
    torch.manual_seed(123)
    torch.randperm(8)
    assert torch.equal(after, torch.rand(3))


def test_indivisible_count_yields_the_full_batches_then_index_error(sim):
    st = filled(5, sensors={"depth": (2,)})
    gen = st.recurrent_generator(torch.zeros(3, 5, 1), 2)
    assert next(gen)[4].shape == (3 * 2, 1)
    assert next(gen)[4].shape == (3 * 2, 1)
    with pytest.raises(IndexError):
        next(gen)


def test_fewer_processes_than_minibatches_assertion(sim):
    st = filled(2, sensors={"depth": (2,)})
    with pytest.raises(AssertionError) as e:
        next(st.recurrent_generator(torch.zeros(3, 2, 1), 4))
    assert str(e.value) == ("Trainer requires the number of processes (2) to be greater than or equal "
                            "to the number of trainer mini batches (4).")


# ------------------------------------------------------------------ returns, advantages, .to()
def test_check_returns_raises_the_reference_message(sim):
    st = filled(4, sensors={"depth": (2,)})
    st.compute_returns(torch.zeros(4, 1), True, 0.99, 0.95)
    st.check_returns()
    st.rewards[1, 2, 0] = float("nan")
    st.compute_returns(torch.zeros(4, 1), True, 0.99, 0.95)   # itself: no check, no synchronisation
    with pytest.raises(AssertionError,
                       match=r"(?s)Return is NaN\.\nreward:\t.*\ngae:\t.*\ndelta:\t.*\nvalue_preds: "):
        st.check_returns()


@pytest.mark.parametrize("use_gae", [True, False])
def test_compute_returns_over_a_partial_rollout(sim, use_gae):
    st = filled(4, num_steps=5, steps=3, sensors={"depth": (2,)})
    ref = copy.deepcopy(st)
    nv = torch.randn(4, 1)
    st.compute_returns(nv, use_gae, 0.99, 0.95)
    if use_gae:
        ref.value_preds[3] = nv
        gae = 0
        for s in reversed(range(3)):
            delta = ref.rewards[s] + 0.99 * ref.value_preds[s + 1] * ref.masks[s + 1] - ref.value_preds[s]
            gae = delta + 0.99 * 0.95 * ref.masks[s + 1] * gae
            ref.returns[s] = gae + ref.value_preds[s]
    else:
        ref.returns[3] = nv
        for s in reversed(range(3)):
            ref.returns[s] = ref.returns[s + 1] * 0.99 * ref.masks[s + 1] + ref.rewards[s]
    assert_same_arenas(st, ref)
    assert torch.equal(st.returns[4], torch.zeros(4, 1))


def test_get_advantages_shapes_and_values(sim):
    st = filled(4, num_steps=5, steps=3, sensors={"depth": (2,)})
    st.returns.copy_(torch.randn(6, 4, 1))
    plain = st.get_advantages(False)
    assert plain.shape == (3, 4, 1) and torch.equal(plain, st.returns[:3] - st.value_preds[:3])
    d = plain.double()
    want = ((d - d.mean()) / (d.std() + 1e-5)).float()
    assert torch.allclose(st.get_advantages(True), want, rtol=2 ** -22, atol=0)


def test_to_rebuilds_the_tables(sim):
    st = filled(4, steps=1)
    old = list(arenas(st).values())
    assert st.to(torch.float64) is None   # (as the reference; every arena is replaced by a new tensor)
    st.to("cpu")
    new = list(arenas(st).values())
    assert all(v.dtype == torch.float64 for v in new) and torch.equal(new[0], old[0].double())
    tabled = st._carried + [a for a, _ in st._batched]
    assert len(tabled) == len(rc.SENSORS) + 5 + len(rc.SENSORS) + 1 + 6 + 4
    for a in tabled:
        assert any(a is b for b in new) and not any(a is b for b in old)


# ------------------------------------------------------------------ WDDPPO.update
class ToyPolicy(nn.Module):
    """evaluate_actions of the right shapes over two small linears"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.body = nn.Linear(rc.SENSORS["instruction"][0] + rc.H, 5)
        self.net = self

    def offset_to_continuous(self, offset):
        return offset * 0.5

    def evaluate_actions(self, obs, h0, prev_actions, masks, actions):
        rows = obs["instruction"].size(0)
        h = h0[:, 0].repeat(rows // h0.size(0), 1) * masks.float()
        out = self.body(torch.cat([obs["instruction"], h], 1))
        logp = -(out[:, 1:2] - actions["distance"]).pow(2)
        entropy = {"pano": out[:, 2].abs(), "offset": out[:, 3].abs(), "distance": out[:, 4].abs()}
        return out[:, 0:1], logp, entropy, None


def test_wddppo_update_runs_every_minibatch_and_reads_back_once(sim):
    st = filled(4)
    st.compute_returns(torch.randn(4, 1), True, 0.99, 0.95)
    policy = ToyPolicy()
    base = copy.deepcopy(policy)
    opt = torch.optim.SGD(policy.parameters(), lr=0.05)
    base_opt = torch.optim.SGD(base.parameters(), lr=0.05)
    perms = [torch.randperm(4, generator=torch.Generator().manual_seed(s)) for s in (1, 2, 3)]
    reads = []
    real_tolist, real_item = torch.Tensor.tolist, torch.Tensor.item
    sim.calls.clear()
    with pytest.MonkeyPatch.context() as mp, rc.fixed_randperm(perms):
        mp.setattr(torch.Tensor, "tolist", lambda t: reads.append(("tolist", t.numel())) or real_tolist(t))
        mp.setattr(torch.Tensor, "item", lambda t: reads.append(("item", t.numel())) or real_item(t))
        got = wddppo_update(policy, opt, st, PPOConfig(), ppo_epoch=3, num_mini_batch=2,
                            use_normalized_advantage=True)
    assert reads == [("tolist", 6)]
    assert sim.names().count("rollout_gather") == 6 and sim.names().count("ppo_advantages") == 1
    assert len(got) == 6 and all(isinstance(v, float) for v in got)
    # the same minibatches, cut by torch indexing, through the minibatch update
    adv = st.get_advantages(True)
    total = torch.zeros(6)
    for perm in perms:
        for sample in rc.torch_minibatches(st, adv, 2, perm):
            total = total + torch.stack(wddppo_minibatch_update(base, base_opt, sample, PPOConfig()))
    assert got == tuple(v / 6 for v in total.tolist())
    for p, q in zip(policy.parameters(), base.parameters()):
        assert torch.equal(p, q)


def test_wddppo_update_takes_a_storage_without_get_advantages(sim):
    st = filled(4)
    st.compute_returns(torch.randn(4, 1), True, 0.99, 0.95)

    class Plain:   # the reference's surface: the arenas and recurrent_generator
        returns, value_preds = st.returns, st.value_preds
        recurrent_generator = staticmethod(st.recurrent_generator)

    policy = ToyPolicy()
    sim.calls.clear()
    got = wddppo_update(policy, torch.optim.SGD(policy.parameters(), lr=0.05), Plain, ppo_epoch=1,
                        num_mini_batch=4)
    assert "ppo_advantages" not in sim.names() and sim.names().count("rollout_gather") == 4
    assert len(got) == 6
