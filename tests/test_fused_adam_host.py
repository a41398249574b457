"""CPU tier: the host side of the two-launch optimizer step (vlnce_amd.optim.Adam) run through a
tensor-level simulator of vlnce_grad_sumsq / vlnce_adam_step.  `AdamSim` below IS their written
contract: clip_grad_norm_'s coefficient and torch's Adam as plain fp32 torch.  The kernels are held
to the same formulas, against fp64, by tests/test_fused_adam_gpu.py."""
import copy
import os

import pytest
import torch
import torch.nn as nn

import cases
import hostsim
import vlnce_amd
from oracle import thirdparty as tp
from vlnce_amd import _lib
from vlnce_amd.il_harness import update_agent
from vlnce_amd.optim import Adam
from vlnce_amd.ppo_harness import PPOConfig, wddppo_minibatch_update

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FLOOR = 2.0 ** -23


class AdamSim(hostsim.HostSim):
    def adam_max_tensors(self):
        return 128

    def adam_chunk(self):
        return 4096

    def adam_supported(self, n_tensors, n_chunks):
        return 1 <= n_tensors <= self.adam_max_tensors() and 0 <= n_chunks < 2 ** 31

    def adam_table(self, ps, ms, vs):
        assert 1 <= len(ps) <= self.adam_max_tensors()
        return _lib.AdamTable(ps, ms, vs, self.adam_chunk())

    def grad_sumsq(self, tab, grads, partials, accumulate):
        """contract of vlnce_grad_sumsq: partials [512] fp64 (+)= sums of squares of the gradients
        present, whose total is the squared norm (how they are dealt to the 512 is the kernel's)"""
        assert len(grads) == tab.n_tensors and partials.dtype == torch.float64
        assert partials.numel() >= _lib.ADAM_PARTIALS
        if not accumulate:
            partials.zero_()
        for g in grads:
            if g is not None:
                partials[0] += g.double().pow(2).sum()

    def adam_step(self, tab, grads, step_size, inv_bc2_sqrt, partials, max_norm, beta1, beta2, eps,
                  weight_decay, norm_out):
        """contract of vlnce_adam_step, in fp32: coef = min(1, max_norm / (norm + 1e-6)) with the
        norm over every launch's gradients; then torch's Adam on each tensor whose gradient is
        present, step_size = lr / (1 - beta1^t), inv_bc2_sqrt = 1 / sqrt(1 - beta2^t) per tensor.
        The gradients are left as they are, and so is every tensor's `_version`."""
        assert len(grads) == len(step_size) == len(inv_bc2_sqrt) == tab.n_tensors
        coef = None
        if partials is not None:
            norm = partials.sum().sqrt().float()
            coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
            if norm_out is not None:
                norm_out.copy_(norm)
        for p, m, v, g, s, c in zip(tab.ps, tab.ms, tab.vs, grads, step_size, inv_bc2_sqrt):
            if g is None:
                continue
            p, g = p.detach(), g.detach()
            if coef is not None:
                g = g * coef
            if weight_decay != 0:
                g = g + weight_decay * p
            m += (g - m) * (1 - beta1)
            v.mul_(beta2).add_((1 - beta2) * g * g)
            # written through the storage, as the kernel writes through the pointer: torch's
            # version counter of the parameter does not move (Adam.step() has to move it)
            p.numpy()[...] = (p - s * m / (v.sqrt() * c + eps)).numpy()


class Recording(AdamSim):
    def __init__(self):
        self.calls = []
        self.step_sizes = []

    def grad_sumsq(self, tab, grads, partials, accumulate):
        self.calls.append(("grad_sumsq", tab.n_tensors, bool(accumulate)))
        return super().grad_sumsq(tab, grads, partials, accumulate)

    def adam_step(self, tab, grads, step_size, *a):
        self.calls.append(("adam_step", tab.n_tensors))
        self.step_sizes.append(list(step_size))
        return super().adam_step(tab, grads, step_size, *a)

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture
def sim(monkeypatch):
    s = Recording()
    monkeypatch.setattr(_lib, "_LIB", s)
    return s


def small_net(seed=0, dtype=torch.float32):
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Linear(7, 6), nn.Tanh(), nn.Linear(6, 3))
    return net.to(dtype)


def batches(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(9, 7, generator=g), torch.randn(9, 3, generator=g) * 3) for _ in range(n)]


def train(net, opt, data, clip=None, before=None):
    dtype = next(net.parameters()).dtype
    for k, (x, y) in enumerate(data):
        opt.zero_grad()
        ((net(x.to(dtype)) - y.to(dtype)) ** 2).mean().backward()
        if before is not None:
            before(k, net)
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(net.parameters(), clip)
        opt.step()


def rel_err(x, x64):
    return ((x.double() - x64).abs().max() / x64.abs().max()).item()


def state_tensors(net, opt):
    out = {}
    for n, p in net.named_parameters():
        out[n] = p.detach()
        if p in opt.state:
            out[n + ".exp_avg"] = opt.state[p]["exp_avg"]
            out[n + ".exp_avg_sq"] = opt.state[p]["exp_avg_sq"]
    return out


@pytest.mark.parametrize("eps", [1e-8, 1e-5])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("clip", [None, 0.5])
def test_ten_steps_follow_torch_adam(sim, clip, weight_decay, eps):
    """bound per tensor: 2 x the error of torch's own fp32 CPU Adam + 2^-23, both measured against
    torch's Adam (+ clip_grad_norm_) in fp64 on the same inputs"""
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=eps, weight_decay=weight_decay)
    data = batches(10)
    ours, ref32, ref64 = small_net(), small_net(), small_net(dtype=torch.float64)
    o_ours = Adam(ours.parameters(), max_grad_norm=clip, **kw)
    o32 = torch.optim.Adam(ref32.parameters(), **kw)
    o64 = torch.optim.Adam(ref64.parameters(), **kw)
    train(ours, o_ours, data)
    train(ref32, o32, data, clip=clip)
    norms = []
    train(ref64, o64, data, before=lambda k, net: norms.append(
        torch.nn.utils.clip_grad_norm_(net.parameters(), clip if clip is not None else 1e30)))
    mine, t32, t64 = (state_tensors(n, o) for n, o in ((ours, o_ours), (ref32, o32), (ref64, o64)))
    assert mine.keys() == t64.keys()
    for name in t64:
        err, yard = rel_err(mine[name], t64[name]), rel_err(t32[name], t64[name])
        print(f"{name}: err {err:.3e} yardstick {yard:.3e}")
        assert err <= 2 * yard + FLOOR, (name, err, yard)
    if clip is not None:
        assert any(n > 1.01 * clip for n in norms) and sim.names().count("grad_sumsq") == 10
        assert abs(o_ours.grad_norm.item() - norms[-1].item()) <= 1e-5 * norms[-1].item()
        assert norms[-1] > 1.01 * clip   # .grad stays unclipped: its norm is still the returned one
        total = torch.cat([p.grad.reshape(-1) for p in ours.parameters()]).norm()
        assert total.item() == pytest.approx(norms[-1].item(), rel=1e-4)
    else:
        assert "grad_sumsq" not in sim.names() and o_ours.grad_norm is None
    for p in ours.parameters():
        assert o_ours.state[p]["step"].item() == 10 and o_ours.state[p]["step"].device.type == "cpu"


def _same_layout(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for name in a["state"][k]:
            assert a["state"][k][name].shape == b["state"][k][name].shape, (k, name)
            assert a["state"][k][name].dtype == b["state"][k][name].dtype, (k, name)


@pytest.mark.parametrize("direction", ["ours_to_torch", "torch_to_ours"])
def test_checkpoint_round_trip(sim, direction):
    kw = dict(lr=3e-3, eps=1e-5, weight_decay=0.01)
    data = batches(7)
    make = {"ours": lambda ps: Adam(ps, **kw), "torch": lambda ps: torch.optim.Adam(ps, **kw)}
    first, second = direction.split("_to_")
    net_a = small_net()
    opt_a = make[first](net_a.parameters())
    train(net_a, opt_a, data[:3])
    sd = copy.deepcopy(opt_a.state_dict())
    net_b = copy.deepcopy(net_a)
    opt_b = make[second](net_b.parameters())
    train(small_net(seed=5), make[second](small_net(seed=5).parameters()), data[:1])
    opt_b.load_state_dict(sd)
    _same_layout(opt_a.state_dict(), opt_b.state_dict())
    for p in net_b.parameters():
        assert opt_b.state[p]["step"].item() == 3
    train(net_a, opt_a, data[3:])
    train(net_b, opt_b, data[3:])
    _same_layout(opt_a.state_dict(), opt_b.state_dict())
    for (n, x), y in zip(state_tensors(net_a, opt_a).items(), state_tensors(net_b, opt_b).values()):
        assert torch.allclose(x, y, rtol=2e-6, atol=1e-9), (n, (x - y).abs().max())
    for p in net_b.parameters():
        assert opt_b.state[p]["step"].item() == 7


def test_a_step_stored_as_a_plain_number_or_float64_tensor_loads(sim):
    """checkpoints of older torch versions keep `step` as an int; both continue from it"""
    net = small_net()
    opt = Adam(net.parameters(), lr=1e-3)
    train(net, opt, batches(2))
    sd = copy.deepcopy(opt.state_dict())
    for k, s in sd["state"].items():
        s["step"] = int(s["step"].item()) if k % 2 else s["step"].double()
    opt2 = Adam(copy.deepcopy(net).parameters(), lr=1e-3)
    opt2.load_state_dict(sd)
    sim.step_sizes.clear()
    for p in opt2.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    opt2.step()
    assert sim.step_sizes[-1] == [1e-3 / (1 - 0.9 ** 3)] * 4
    assert all(isinstance(s["step"], torch.Tensor) and s["step"].item() == 3
               for s in opt2.state.values())


def test_a_checkpoint_of_a_foreach_optimizer_loads(sim):
    """foreach / fused / capturable say how the writer ran its step, not what it computed"""
    net = small_net()
    writer = torch.optim.Adam(net.parameters(), lr=1e-3, foreach=True)
    train(net, writer, batches(2))
    sd = copy.deepcopy(writer.state_dict())
    sd["param_groups"][0]["capturable"] = True
    opt = Adam(net.parameters(), lr=1e-3)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["foreach"] is None and opt.param_groups[0]["fused"] is None
    assert opt.param_groups[0]["capturable"] is False
    train(net, opt, batches(1))
    assert all(s["step"].item() == 3 for s in opt.state.values())
    sd["param_groups"][0]["amsgrad"] = True   # that one changes the arithmetic
    with pytest.raises(ValueError):
        Adam(net.parameters(), lr=1e-3).load_state_dict(sd)


def test_step_counts_survive_torch_save_and_a_replaced_entry(sim):
    """the counts are separate 0-dim `step` entries for everyone else, whatever storage they share"""
    import io

    net = small_net()
    opt = Adam(net.parameters(), lr=1e-3)
    train(net, opt, batches(3))
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf)
    ref = torch.optim.Adam(copy.deepcopy(net).parameters(), lr=1e-3)
    ref.load_state_dict(sd)
    for s in ref.state.values():
        assert s["step"].shape == () and s["step"].dtype == torch.float32 and s["step"].item() == 3
    ps = list(ref.state)
    ps[0].grad = torch.ones_like(ps[0])
    ref.step()   # torch increments one of them in place: the others keep their count
    assert [s["step"].item() for s in ref.state.values()] == [4, 3, 3, 3]
    # an entry the user replaces is read, not a stale copy of it
    first = next(iter(net.parameters()))
    opt.state[first]["step"] = torch.tensor(10.0)
    sim.step_sizes.clear()
    train(net, opt, batches(1))
    assert opt.state[first]["step"].item() == 11
    assert sorted(set(sim.step_sizes[-1])) == pytest.approx(
        sorted([1e-3 / (1 - 0.9 ** 4), 1e-3 / (1 - 0.9 ** 11)]), rel=1e-12)
    opt.state[first]["step"].fill_(20.0)   # ... and so is one changed in place
    train(net, opt, batches(1))
    assert opt.state[first]["step"].item() == 21


def test_lambda_lr_sets_the_rate_of_every_step(sim):
    net = small_net()
    opt = Adam(net.parameters(), lr=2e-3)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0 / (1 + e))
    data = batches(5)
    for k, (x, y) in enumerate(data):
        opt.zero_grad()
        ((net(x) - y) ** 2).mean().backward()
        opt.step()
        sched.step()
        want = 2e-3 / (1 + k) / (1 - 0.9 ** (k + 1))
        assert sim.step_sizes[-1] == pytest.approx([want] * 4, rel=1e-15)
        assert sched.get_last_lr() == [pytest.approx(2e-3 / (2 + k))]


def test_missing_gradients_keep_a_step_count_per_parameter(sim):
    """grad is None on every second step for one parameter, always for another"""
    def before(k, net):
        net[0].bias.grad = None
        if k % 2:
            net[2].weight.grad = None

    kw = dict(lr=1e-2, eps=1e-8)
    data = batches(6)
    ours, ref = small_net(), small_net()
    o_ours, o_ref = Adam(ours.parameters(), max_grad_norm=0.5, **kw), torch.optim.Adam(ref.parameters(), **kw)
    train(ours, o_ours, data, before=before)
    train(ref, o_ref, data, before=before, clip=0.5)
    assert ours[0].bias not in o_ours.state and ref[0].bias not in o_ref.state
    assert o_ours.state[ours[2].weight]["step"].item() == 3 == o_ref.state[ref[2].weight]["step"].item()
    assert o_ours.state[ours[0].weight]["step"].item() == 6
    _same_layout(o_ours.state_dict(), o_ref.state_dict())
    assert torch.equal(ours[0].bias, ref[0].bias)
    for (n, x), y in zip(state_tensors(ours, o_ours).items(), state_tensors(ref, o_ref).values()):
        assert torch.allclose(x, y, rtol=2e-6, atol=1e-9), (n, (x - y).abs().max())
    # the skipped tensor's bias corrections are its own
    last = sim.step_sizes[-1]
    assert 0.0 in last and 1e-2 / (1 - 0.9 ** 6) in last


def _flat_params(n, groups=1):
    torch.manual_seed(3)
    ps = [nn.Parameter(torch.randn(5)) for _ in range(n)]
    for p in ps:
        p.grad = torch.randn(5)
    return ps


def test_call_counts_without_clipping(sim):
    M = sim.adam_max_tensors()
    ps, qs = _flat_params(M), _flat_params(3)
    opt = Adam([dict(params=ps), dict(params=qs, lr=1e-2)])
    opt.step()
    assert sim.calls == [("adam_step", M), ("adam_step", 3)]


def test_call_counts_with_clipping_and_a_split_list(sim):
    M = sim.adam_max_tensors()
    ps = _flat_params(M + 1)
    ref = [nn.Parameter(p.detach().clone()) for p in ps]
    for p, q in zip(ps, ref):
        q.grad = p.grad.clone()
    opt = Adam(ps, lr=1e-2, max_grad_norm=0.3)
    opt.step()
    assert sim.calls == [("grad_sumsq", M, False), ("grad_sumsq", 1, True), ("adam_step", M),
                         ("adam_step", 1)]
    norm = torch.nn.utils.clip_grad_norm_(ref, 0.3)
    torch.optim.Adam(ref, lr=1e-2).step()
    assert opt.grad_norm.item() == pytest.approx(norm.item(), rel=1e-6)   # spans both launches
    for p, q in zip(ps, ref):
        assert torch.allclose(p, q, rtol=2e-6, atol=1e-9)
    opt.step()   # the tables are kept: same launches again
    assert len(sim.calls) == 8 and sim.calls[4:] == sim.calls[:4]


def test_a_moved_parameter_rebuilds_the_table(sim, monkeypatch):
    built = []
    inner = AdamSim.adam_table
    monkeypatch.setattr(AdamSim, "adam_table", lambda self, *a: built.append(1) or inner(self, *a))
    ps = _flat_params(3)
    opt = Adam(ps)
    opt.step(), opt.step()
    assert len(built) == 1
    ps[1].data = ps[1].data.clone()
    opt.step()
    assert len(built) == 2


def test_closure_is_honoured(sim):
    net = small_net()
    opt = Adam(net.parameters())
    x, y = batches(1)[0]

    def closure():
        opt.zero_grad()
        loss = ((net(x) - y) ** 2).mean()
        loss.backward()
        return loss

    loss = opt.step(closure)
    assert loss.requires_grad and sim.names() == ["adam_step"]


def test_a_non_contiguous_gradient_is_made_contiguous(sim):
    p, q = nn.Parameter(torch.randn(4, 6)), nn.Parameter(torch.randn(4, 6))
    q.data.copy_(p.data)
    g = torch.randn(6, 4).t()
    p.grad, q.grad = g, g.contiguous()
    assert not p.grad.is_contiguous()
    Adam([p]).step(), torch.optim.Adam([q]).step()
    assert torch.allclose(p, q, rtol=2e-6, atol=1e-9)


@pytest.mark.parametrize("kw", [dict(amsgrad=True), dict(maximize=True), dict(capturable=True),
                                dict(differentiable=True), dict(foreach=True), dict(foreach=False),
                                dict(fused=True), dict(fused=False)])
def test_refused_settings(sim, kw):
    with pytest.raises(ValueError):
        Adam(small_net().parameters(), **kw)


def test_refused_parameters_and_gradients(sim, monkeypatch):
    with pytest.raises(ValueError):
        Adam([nn.Parameter(torch.randn(4).double())])
    with pytest.raises(ValueError):
        Adam([nn.Parameter(torch.randn(4).half())])
    with pytest.raises(ValueError):
        Adam([nn.Parameter(torch.randn(4, 6).t())])
    with pytest.raises(ValueError):   # a later group is held to the same rules
        Adam(small_net().parameters()).add_param_group(dict(params=[nn.Parameter(torch.randn(3, 2).t())]))
    with pytest.raises(ValueError):
        Adam(small_net().parameters()).add_param_group(dict(params=[nn.Parameter(torch.randn(3))],
                                                             amsgrad=True))
    emb = nn.Embedding(6, 3, sparse=True)
    opt = Adam(emb.parameters())
    emb(torch.tensor([1, 2])).sum().backward()
    with pytest.raises(ValueError):
        opt.step()
    # with the HIP library a parameter on the CPU is refused at construction
    monkeypatch.setattr(sim, "name", "hip", raising=False)
    with pytest.raises(ValueError):
        Adam(small_net().parameters())


# ---- the harnesses
def _policy(name):
    case = cases.CASES[name]
    obs, prev, masks, extra, _ = cases.load_case(os.path.join(GOLD, name + ".npz"))
    policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                   tp.synth_state_dict)
    return policy, obs, prev, masks, extra


def _trainable(policy):
    return [p for p in policy.parameters() if p.requires_grad]


@pytest.fixture
def clip_calls(monkeypatch):
    calls = []
    inner = torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda *a, **k: calls.append(1) or inner(*a, **k))
    return calls


def test_update_agent_default_optimizer_never_calls_the_new_entry_points(sim):
    policy, obs, prev, masks, extra = _policy("cma_update_64")
    hs = policy.net.model_config.STATE_ENCODER.hidden_size
    opt = torch.optim.Adam(_trainable(policy), lr=2.5e-4)
    update_agent(policy, opt, obs, prev, masks, extra["targets"], extra["weights"], hs)
    assert sim.calls == []


def test_update_agent_with_this_optimizer_steps_through_it(sim):
    policy, obs, prev, masks, extra = _policy("cma_update_64")
    ref = _policy("cma_update_64")[0]
    hs = policy.net.model_config.STATE_ENCODER.hidden_size
    args = (obs, prev, masks, extra["targets"], extra["weights"], hs)
    opt = Adam(_trainable(policy), lr=2.5e-4)
    update_agent(policy, opt, *args)
    update_agent(ref, torch.optim.Adam(_trainable(ref), lr=2.5e-4), *args)
    n = len(opt.state)
    assert n > 10 and sim.names() == ["adam_step"] * -(-n // sim.adam_max_tensors())
    for (name, p), q in zip(policy.named_parameters(), ref.parameters()):
        assert torch.allclose(p, q, rtol=1e-4, atol=1e-4), name
        assert p.grad is None or not p.grad.any()   # update_agent's own zero_grad()


def _sample(policy, obs, prev, masks, extra):
    L = policy.net.num_recurrent_layers
    return cases.ppo_sample(obs, {k: v.clone() for k, v in prev.items()}, masks, extra,
                            extra["h0"][:, :L].contiguous())


def test_wddppo_default_optimizer_clips_with_torch(sim, clip_calls):
    policy, obs, prev, masks, extra = _policy("waypoint_ppo_update_64")
    opt = torch.optim.Adam(_trainable(policy), lr=2.5e-4, eps=1e-5)
    wddppo_minibatch_update(policy, opt, _sample(policy, obs, prev, masks, extra), PPOConfig(**cases.PPO))
    assert sim.calls == [] and clip_calls == [1]


def test_wddppo_with_this_optimizer_does_not_call_clip_grad_norm(sim, clip_calls):
    policy, obs, prev, masks, extra = _policy("waypoint_ppo_update_64")
    ref = _policy("waypoint_ppo_update_64")[0]
    cfg = PPOConfig(**cases.PPO)
    opt = Adam(_trainable(policy), lr=2.5e-4, eps=1e-5, max_grad_norm=cfg.max_grad_norm)
    wddppo_minibatch_update(policy, opt, _sample(policy, obs, prev, masks, extra), cfg)
    assert clip_calls == [] and sim.names().count("grad_sumsq") >= 1
    assert sim.names() == sorted(sim.names(), reverse=True)   # the norm set first, then the steps
    ropt = torch.optim.Adam(_trainable(ref), lr=2.5e-4, eps=1e-5)
    wddppo_minibatch_update(ref, ropt, _sample(ref, obs, prev, masks, extra), cfg)
    assert clip_calls == [1]
    for (name, p), q in zip(policy.named_parameters(), ref.parameters()):
        assert torch.allclose(p, q, rtol=1e-4, atol=1e-4), name
    # an optimizer of this class WITHOUT max_grad_norm leaves the clip to the harness
    opt2 = Adam(_trainable(ref), lr=2.5e-4, eps=1e-5)
    wddppo_minibatch_update(ref, opt2, _sample(ref, obs, prev, masks, extra), cfg)
    assert clip_calls == [1, 1]
