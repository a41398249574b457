"""CPU tier: the host side of the one-launch imitation-learning objective (ILLossFn, il_loss,
AuxLosses.fused / register_pair_loss, update_agent(fused_loss=True)) run through a tensor-level
simulator of the two new entry points.  `ILSim` below IS their written contract: the reference
trainer's formulas (base_il_trainer.py:159-172, aux_losses.py:24-32 over the broadcast of
cma_policy.py:296-307) as plain fp32 torch with torch's own autograd.  The kernels are held to the
same formulas, in fp64, by tests/test_il_loss_gpu.py."""
import os

import pytest
import torch
import torch.nn.functional as F

import cases
import hostsim
import vlnce_amd
from oracle import thirdparty as tp
from test_oracle_golden import compare
from vlnce_amd import _lib
from vlnce_amd.aux_losses import AuxLossRegistry
from vlnce_amd.il_harness import ILLossFn, il_loss, update_agent

GOLD = os.path.join(os.path.dirname(__file__), "golden")
torch.distributions.Distribution.set_default_validate_args(False)


class ILSim(hostsim.HostSim):
    def il_loss_supported(self, T, N, A):
        return T >= 1 and 1 <= N <= 1024 and 1 <= A <= 16

    def il_loss(self, logits, targets, weights, aux, inv_scalar, T, N, A, stats, dlogits):
        """contract of vlnce_il_loss: stats [3] = {(action + aux) * inv_scalar, action, aux or 0},
        dlogits [T*N, A] = d stats[0] / d logits"""
        assert self.il_loss_supported(T, N, A)
        with torch.enable_grad():   # (called from inside an autograd.Function's forward)
            z = logits.detach().clone().view(T, N, A).requires_grad_(True)
            w = weights.view(T, N)
            ce = F.cross_entropy(z.permute(0, 2, 1), targets.view(T, N), reduction="none")
            action = ((w * ce).sum(0) / w.sum(0)).mean()
            x = aux.reshape(()) if aux is not None else torch.zeros(())
            loss = (action + x) * inv_scalar
            (g,) = torch.autograd.grad(loss, z)
        stats.copy_(torch.stack([loss, action, x]).detach())
        dlogits.copy_(g.reshape(T * N, A))

    def pair_mse(self, estimate, target, mask, E, R, value, d_estimate):
        """contract of vlnce_pair_mse: the masked mean of the [R, E] matrix (e_j - t_i)^2, the
        [E] mask selecting columns, and its gradient wrt the estimates"""
        with torch.enable_grad():
            e = estimate.detach().clone().view(E).requires_grad_(True)
            v = ((e - target.view(R, 1)) ** 2).masked_select(mask.view(E).bool()).mean()
            (g,) = torch.autograd.grad(v, e)
        value.copy_(v.detach())
        d_estimate.copy_(g)


class Recording(ILSim):
    def __init__(self):
        self.calls = []

    def il_loss(self, *a):
        self.calls.append("il_loss")
        return super().il_loss(*a)

    def pair_mse(self, *a):
        self.calls.append("pair_mse")
        return super().pair_mse(*a)


def fused_update(policy, obs, prev, masks, targets, weights):
    hs = policy.net.model_config.STATE_ENCODER.hidden_size
    return update_agent(policy, None, obs, prev, masks, targets, weights, hs, step_grad=False,
                        fused_loss=True)


def default_update(policy, obs, prev, masks, targets, weights):
    hs = policy.net.model_config.STATE_ENCODER.hidden_size
    return update_agent(policy, None, obs, prev, masks, targets, weights, hs, step_grad=False)


def run(name, update_fn, case=None):
    case = case or cases.CASES[name]
    obs, prev, masks, extra, gold = cases.load_case(os.path.join(GOLD, name + ".npz"))
    policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                   tp.synth_state_dict)
    outs = cases.run_case(policy, case, obs, prev, masks, extra, update_fn, vlnce_amd.AuxLosses)
    return outs, gold


@pytest.mark.parametrize("name", ["cma_update_64", "seq2seq_update_64"])
def test_fused_update_matches_reference_golden(monkeypatch, name):
    """both progress-monitor goldens of the real reference classes, through fused_loss=True"""
    sim = Recording()
    monkeypatch.setattr(_lib, "_LIB", sim)
    outs, gold = run(name, fused_update)
    compare(outs, gold, atol=1e-4, rtol=1e-4)
    assert sorted(sim.calls) == ["il_loss", "pair_mse"]   # exactly one launch of each
    assert all(isinstance(v, float) for v in outs["loss"].tolist())
    assert not vlnce_amd.AuxLosses.is_fused()


@pytest.mark.parametrize("name", ["cma_update_64", "seq2seq_update_64"])
def test_default_update_never_calls_the_new_entry_points(monkeypatch, name):
    sim = Recording()
    monkeypatch.setattr(_lib, "_LIB", sim)
    outs, gold = run(name, default_update)
    compare(outs, gold, atol=1e-4, rtol=1e-4)
    assert sim.calls == []


def test_monitor_off_makes_one_il_loss_and_no_pair_mse(monkeypatch):
    sim = Recording()
    monkeypatch.setattr(_lib, "_LIB", sim)
    case = dict(cases.CASES["cma_update_64"], overrides={})
    policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                   tp.synth_state_dict)
    obs, prev, masks, extra = cases.build_inputs(case)
    vlnce_amd.AuxLosses.activate()
    try:
        fused = fused_update(policy, obs, prev, masks, extra["targets"], extra["weights"])
        grads = {n: p.grad.clone() for n, p in policy.named_parameters() if p.grad is not None}
        assert sim.calls == ["il_loss"]
        policy.zero_grad(set_to_none=True)
        plain = default_update(policy, obs, prev, masks, extra["targets"], extra["weights"])
    finally:
        vlnce_amd.AuxLosses.deactivate()
    assert sim.calls == ["il_loss"]
    assert fused[2] == 0.0 and isinstance(fused[2], float) and plain[2] == 0.0
    assert fused == pytest.approx(plain, rel=1e-5, abs=1e-6)
    for n, p in policy.named_parameters():
        if p.grad is not None:
            assert torch.allclose(grads[n], p.grad, rtol=1e-4, atol=1e-6), n


def test_registry_inactive_returns_float_zero_aux(monkeypatch):
    """without an activation window (bench.py, smoke()) nothing is registered or reduced"""
    sim = Recording()
    monkeypatch.setattr(_lib, "_LIB", sim)
    case = cases.CASES["cma_update_64"]
    policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                   tp.synth_state_dict)
    obs, prev, masks, extra = cases.build_inputs(case)
    assert not vlnce_amd.AuxLosses.is_active()
    out = fused_update(policy, obs, prev, masks, extra["targets"], extra["weights"])
    assert sim.calls == ["il_loss"] and out[2] == 0.0 and out[0] == pytest.approx(out[1])


def pair_inputs(E, R, seed=0):
    g = torch.Generator().manual_seed(seed)
    estimate = torch.tanh(torch.randn(E, generator=g)).requires_grad_(True)
    target = torch.rand(R, 1, generator=g)
    mask = torch.rand(E, generator=g) < 0.6
    mask[0] = True
    return estimate, target, mask


def test_get_loss_on_a_pair_entry_is_the_broadcast_matrix():
    reg = AuxLossRegistry()
    estimate, target, _ = pair_inputs(5, 7)
    with reg.active():
        reg.register_pair_loss("pm", estimate, target, 0.5)
        got = reg.get_loss("pm")
        assert reg.names() == ["pm"]
        with pytest.raises(AssertionError, match="twice"):
            reg.register_pair_loss("pm", estimate, target, 0.5)
    e, t = torch.broadcast_tensors(estimate, target)
    assert got.shape == (7, 5) and torch.equal(got, (e - t) ** 2)
    with pytest.raises(AssertionError, match="outside an activation window"):
        AuxLossRegistry().register_pair_loss("pm", estimate, target)


@pytest.mark.parametrize("E,R", [(6, 6), (5, 9)])
def test_reduce_routes_pair_entries_only_inside_fused(monkeypatch, E, R):
    sim = Recording()
    monkeypatch.setattr(_lib, "_LIB", sim)
    estimate, target, mask = pair_inputs(E, R)
    want = 0.5 * ((estimate - target) ** 2).masked_select(mask).mean()
    (gwant,) = torch.autograd.grad(want * 3, estimate)
    reg = AuxLossRegistry()
    with reg.active():
        reg.register_pair_loss("pm", estimate, target, 0.5)
        plain = reg.reduce(mask)             # not fused: today's arithmetic on the matrix
        assert sim.calls == []
        with reg.fused():
            fused = reg.reduce(mask)
        assert sim.calls == ["pair_mse"] and not reg.is_fused()
    assert torch.equal(plain, want)
    (gplain,) = torch.autograd.grad(plain * 3, estimate)
    (gfused,) = torch.autograd.grad(fused * 3, estimate)
    assert torch.equal(gplain, gwant)
    assert torch.allclose(fused, want, rtol=1e-6, atol=0)
    assert torch.allclose(gfused, gwant, rtol=1e-5, atol=1e-8)


def test_reduce_takes_the_existing_path_under_data_parallelism(monkeypatch):
    import torch.distributed as dist

    sim = Recording()
    monkeypatch.setattr(_lib, "_LIB", sim)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    monkeypatch.setattr(dist, "all_reduce", lambda t, group=None: None)   # one rank: the sum is t
    estimate, target, mask = pair_inputs(6, 6)
    reg = AuxLossRegistry()
    reg.set_data_parallel(True)
    assert reg.data_parallel()
    with reg.active(), reg.fused():
        reg.register_pair_loss("pm", estimate, target, 0.5)
        got = reg.reduce(mask)
    assert sim.calls == []
    want = 0.5 * ((estimate - target) ** 2).masked_select(mask).mean()
    assert torch.allclose(got, want, rtol=1e-6, atol=0)
    (g,) = torch.autograd.grad(got, estimate)
    (gw,) = torch.autograd.grad(want, estimate)
    assert torch.allclose(g, gw, rtol=1e-5, atol=1e-8)


def test_il_loss_function_gradients_and_stats(monkeypatch):
    """ILLossFn: dlogits * g for the logits, g * inv_scalar for a tensor aux, stats detached"""
    monkeypatch.setattr(_lib, "_LIB", ILSim())
    g = torch.Generator().manual_seed(4)
    T, N, A = 5, 3, 6
    logits = torch.randn(T, N, A, generator=g, requires_grad=True)
    targets = torch.randint(0, A, (T, N), generator=g)
    weights = torch.ones(T, N)
    weights[0] = 3.2
    weights[3:, 1] = 0.0
    aux = torch.tensor(0.37, requires_grad=True)
    loss, stats = il_loss(logits, targets, weights, aux, loss_accumulation_scalar=4)
    assert not stats.requires_grad and loss.shape == () and stats.shape == (3,)
    (loss * 3).backward()
    z = logits.detach().clone().requires_grad_(True)
    ce = F.cross_entropy(z.permute(0, 2, 1), targets, reduction="none")
    action = ((weights * ce).sum(0) / weights.sum(0)).mean()
    ref = (action + 0.37) / 4
    (ref * 3).backward()
    assert torch.allclose(loss, ref, rtol=1e-6) and torch.allclose(stats[1], action, rtol=1e-6)
    assert float(stats[2]) == pytest.approx(0.37)
    assert torch.allclose(logits.grad, z.grad, rtol=1e-5, atol=1e-8)
    assert float(aux.grad) == pytest.approx(0.75)
    # a Python number for aux: no gradient slot, the same loss
    loss2, stats2 = il_loss(logits.detach(), targets, weights, 0.37, loss_accumulation_scalar=4)
    assert torch.allclose(loss2, ref, rtol=1e-6) and float(stats2[2]) == pytest.approx(0.37)
    loss3, stats3 = ILLossFn.apply(logits.detach(), targets, weights, None, 1.0)
    assert float(stats3[2]) == 0.0 and torch.allclose(loss3, action, rtol=1e-6)


def test_unsupported_shape_takes_the_torch_path(monkeypatch):
    sim = Recording()
    sim.il_loss_supported = lambda T, N, A: False
    monkeypatch.setattr(_lib, "_LIB", sim)
    outs, gold = run("cma_update_64", fused_update)
    compare(outs, gold, atol=1e-4, rtol=1e-4)
    assert sim.calls == ["pair_mse"]
