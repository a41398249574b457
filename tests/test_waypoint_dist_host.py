"""CPU tier: the host side of the one-launch WaypointPolicy.evaluate_actions (WaypointEvalFn,
policy.fused_distributions, the "waypoint_dist" option, check_eval_flags) run through a tensor-level
simulator of the two new entry points.  `WaypointSim` below IS their written contract: the
arithmetic of waypoint_policy.py:258-347 through this package's own CustomFixedCategorical and
TruncatedNormal (utils.py) as plain fp32 torch with torch's autograd, plus the flag bits that stand
in for the reference's assertions.  The kernels are held to the same formulas, in fp64, by
tests/test_waypoint_dist_gpu.py."""
import math
import os

import pytest
import torch

import cases
import hostsim
import vlnce_amd
from oracle import thirdparty as tp
from test_oracle_golden import compare
from vlnce_amd import _lib
from vlnce_amd._lib import (WP_ABSENT, WP_CONTINUOUS, WP_DISCRETE, WP_FLAG_CLASS, WP_FLAG_ELEMENT,
                            WP_FLAG_LOC, WP_FLAG_PANO, WP_FLAG_SHIFT, WP_FLAG_VARIANCE)
from vlnce_amd.ppo_harness import PPOConfig, wddppo_minibatch_update
from vlnce_amd.utils import CustomFixedCategorical, TruncatedNormal, batched_index_select

GOLD = os.path.join(os.path.dirname(__file__), "golden")
torch.distributions.Distribution.set_default_validate_args(False)
WAYPOINT_GOLDENS = ["waypoint_64", "waypoint_discrete_64", "waypoint_hpn_c_64", "waypoint_hpn_64",
                    "waypoint_ppo_update_64"]


def _planes(value, leaf):
    """d sum(value) / d leaf [B, n] as n planes [n, B] (the rows are independent)"""
    (g,) = torch.autograd.grad(value.sum(), leaf, retain_graph=True)
    return g.reshape(g.shape[0], -1).t()


class WaypointSim(hostsim.HostSim):
    def waypoint_eval_supported(self, B, P, K_offset, K_distance):
        return B >= 1 and 1 <= P <= 63 and 0 <= K_offset <= 32 and 0 <= K_distance <= 32

    def waypoint_eval(self, logits, pano, offset, distance, B, P, out, saved, flags):
        """contract of vlnce_waypoint_eval (include/vlnce_hip.h): out = {log_prob [B], pano entropy
        [B], offset block, distance block}, a block being gate * weight * H [B] or, for a discrete
        part, the reference's broadcast E[i][j] = gate_i weight H_j [B, B]; saved [S, B] = the partial
        derivatives of log_prob and of the entropies (gate * weight folded in, except a discrete
        part's entropy planes); flags [B].  A flagged row is NaN in every output; its inputs are
        replaced by harmless ones before the distribution classes (which assert on them) see them."""
        assert self.waypoint_eval_supported(B, P, offset.K, distance.K)
        c = pano.view(B)
        bad = (c < 0) | (c > P)
        fl = bad.to(torch.int32) * WP_FLAG_PANO
        c = torch.where(bad, torch.zeros_like(c), c)
        heading = (c % P).view(B, 1)
        gate = (c != P).float().view(B, 1)
        with torch.enable_grad():   # (called from inside an autograd.Function's forward)
            z = logits.detach().clone().view(B, P + 1).requires_grad_(True)
            head = CustomFixedCategorical(logits=z)
            total, h_pano = head.log_prob(c.view(B, 1)), head.entropy()
            planes = {"pano": [_planes(total, z), _planes(h_pano, z)]}
            total = total.detach().clone()
            ents = {}
            for name, part in (("distance", distance), ("offset", offset)):   # the reference's order
                planes[name] = []
                ents[name] = torch.zeros(B)
                bits = torch.zeros(B, 1, dtype=torch.int32)
                if part.kind == WP_ABSENT:
                    continue
                w = gate * part.weight
                if part.kind == WP_CONTINUOUS:
                    lo, hi = part.lo, part.hi
                    loc = part.first.view(B, P).gather(1, heading)
                    var = part.second.view(B, P).gather(1, heading)
                    v = part.element.view(B, 1)
                    bits = (~((loc >= lo) & (loc <= hi))).int() * WP_FLAG_LOC \
                        | (~(var.sqrt() >= 0.0)).int() * WP_FLAG_VARIANCE \
                        | (~((v >= lo) & (v <= hi))).int() * WP_FLAG_ELEMENT
                    ok = bits == 0
                    mid = 0.5 * (lo + hi)
                    loc = torch.where(ok, loc, torch.full_like(loc, mid)).detach().requires_grad_(True)
                    var = torch.where(ok, var, torch.ones_like(var)).detach().requires_grad_(True)
                    v = torch.where(ok, v, torch.full_like(v, mid))
                    d = TruncatedNormal(loc=loc, scale=var.sqrt(), smin=lo, smax=hi)
                    lp, ent = w * d.log_prob(v), w * d.entropy()
                    planes[name] = [_planes(lp, loc), _planes(lp, var), _planes(ent, loc),
                                    _planes(ent, var)]
                else:
                    K = part.K
                    k = part.element.view(B)
                    badk = (k < 0) | (k >= K)
                    bits = badk.int().view(B, 1) * WP_FLAG_CLASS
                    k = torch.where(badk, torch.zeros_like(k), k)
                    rows = batched_index_select(part.first.view(B, P, K), dim=1, index=heading)
                    rows = rows.detach().clone().requires_grad_(True)
                    d = CustomFixedCategorical(logits=rows)
                    lp, ent = w * d.log_prob(k.view(B, 1)), d.entropy()
                    planes[name] = [_planes(lp, rows), _planes(ent, rows)]
                    ent = w * ent           # [B, 1] * [B]: the reference's broadcast
                    ent[bad] = math.nan     # (no gate for a choice outside [0, P])
                fl = fl | (bits.view(B) << WP_FLAG_SHIFT[name])
                total = total + lp.detach()
                ents[name] = ent.detach().reshape(B, -1)    # [B, 1] or [B, B]
        res = [total.view(B, 1), h_pano.detach().view(B, 1), ents["offset"], ents["distance"]]
        for r in res[:2] + [e for e in res[2:] if e.shape[1] == 1]:
            r[fl != 0] = math.nan
        for e in res[2:]:
            if e.shape[1] == B and e.numel() == B * B:
                e[:, fl != 0] = math.nan    # column j belongs to row j's categorical
        out.copy_(torch.cat([r.reshape(-1) for r in res]))
        saved.view(-1, B).copy_(torch.cat(planes["pano"] + planes["offset"] + planes["distance"]))
        flags.copy_(fl)

    def waypoint_eval_bwd(self, grads, pano, saved, flags, offset, distance, B, P, d_logits):
        """contract of vlnce_waypoint_eval_bwd: dense gradients (zero outside the chosen heading),
        NaN throughout a flagged row"""
        sv = saved.view(-1, B)
        bad = flags != 0
        c = pano.view(B)
        valid = (c >= 0) & (c <= P)
        h = torch.where(valid, c, torch.zeros_like(c)) % P
        g = []
        for x, part in zip(grads, (None, None, offset, distance)):
            if x is None:
                g.append(torch.zeros(B))
            elif part is not None and part.kind == WP_DISCRETE:   # column sums over the rows' gates
                w = (valid & (c != P)).float() * part.weight
                g.append((x.view(B, B)[valid] * w[valid, None]).sum(0))
            else:
                g.append(x.view(B))
        rows = torch.arange(B)
        dl = sv[:P + 1].t() * g[0][:, None] + sv[P + 1:2 * P + 2].t() * g[1][:, None]
        dl[bad] = math.nan
        d_logits.copy_(dl)
        s = 2 * (P + 1)
        for part, ge in ((offset, g[2]), (distance, g[3])):
            if part.kind == WP_CONTINUOUS:
                for dst, lp_plane, ent_plane in ((part.d_first, s, s + 2), (part.d_second, s + 1, s + 3)):
                    dense = torch.zeros(B, P)
                    dense[rows, h] = sv[lp_plane] * g[0] + sv[ent_plane] * ge
                    dense[bad] = math.nan
                    dst.copy_(dense.view_as(dst))
                s += 4
            elif part.kind == WP_DISCRETE:
                K = part.K
                dense = torch.zeros(B, P, K)
                dense[rows, h] = sv[s:s + K].t() * g[0][:, None] + sv[s + K:s + 2 * K].t() * ge[:, None]
                dense[bad] = math.nan
                part.d_first.copy_(dense.view_as(part.d_first))
                s += 2 * K


class Recording(WaypointSim):
    def __init__(self):
        self.calls = []

    def waypoint_eval(self, *a):
        self.calls.append("waypoint_eval")
        return super().waypoint_eval(*a)

    def waypoint_eval_bwd(self, *a):
        self.calls.append("waypoint_eval_bwd")
        return super().waypoint_eval_bwd(*a)


def ppo(policy, sample):
    stats = wddppo_minibatch_update(policy, None, sample, PPOConfig(**cases.PPO), step_grad=False,
                                    clip_grads=False)
    return [float(v) for v in stats]


def run(name, fused):
    case = cases.CASES[name]
    obs, prev, masks, extra, gold = cases.load_case(os.path.join(GOLD, name + ".npz"))
    policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                   tp.synth_state_dict)
    policy.fused_distributions = fused
    outs = cases.run_case(policy, case, obs, prev, masks, extra, None, vlnce_amd.AuxLosses, ppo_fn=ppo)
    return policy, outs, gold


@pytest.mark.parametrize("name", WAYPOINT_GOLDENS)
def test_fused_distributions_match_reference_golden(monkeypatch, name):
    """all five Waypoint goldens of the real reference classes through fused_distributions=True:
    exactly one forward launch per evaluate_actions, one backward launch per backward()"""
    sim = Recording()
    monkeypatch.setattr(_lib, "_LIB", sim)
    policy, outs, gold = run(name, True)
    compare(outs, gold, atol=1e-4, rtol=1e-4)
    update = cases.CASES[name]["call"] == "ppo_update"
    assert sim.calls == (["waypoint_eval", "waypoint_eval_bwd"] if update else ["waypoint_eval"])
    B = cases.CASES[name]["N"] * cases.CASES[name]["T"]
    assert policy.eval_flags.shape == (B,) and policy.eval_flags.dtype == torch.int32
    assert not policy.eval_flags.requires_grad
    policy.check_eval_flags()   # clean input: silent


@pytest.mark.parametrize("name", WAYPOINT_GOLDENS)
def test_default_path_never_calls_the_new_entry_points(monkeypatch, name):
    sim = Recording()
    monkeypatch.setattr(_lib, "_LIB", sim)
    policy, outs, gold = run(name, False)
    compare(outs, gold, atol=1e-4, rtol=1e-4)
    assert sim.calls == [] and policy.eval_flags is None
    assert vlnce_amd.WaypointPolicy.fused_distributions is False


def test_result_shapes_and_dtypes_are_those_of_the_torch_path(monkeypatch):
    monkeypatch.setattr(_lib, "_LIB", WaypointSim())
    got = {}
    for fused in (False, True):
        _, outs, _ = run("waypoint_discrete_64", fused)
        got[fused] = outs
    for k, v in got[False].items():
        if isinstance(v, torch.Tensor):
            assert got[True][k].shape == v.shape and got[True][k].dtype == v.dtype, k
    # a discrete part's entropy is the reference's [B, 1] * [B] broadcast
    assert got[True]["ev_logp"].shape == (2, 1) and got[True]["ent_offset"].shape == (2, 2)
    _, cont, _ = run("waypoint_64", True)
    assert cont["ent_offset"].shape == (2,) and cont["ent_pano"].shape == (2,)
    assert list(got[True]) == list(got[False])


def test_unsupported_shape_takes_the_torch_path(monkeypatch):
    sim = Recording()
    sim.waypoint_eval_supported = lambda B, P, Ko, Kd: False
    monkeypatch.setattr(_lib, "_LIB", sim)
    policy, outs, gold = run("waypoint_ppo_update_64", True)
    compare(outs, gold, atol=1e-4, rtol=1e-4)
    assert sim.calls == [] and policy.eval_flags is None


def test_dispatch_option_switches_the_fused_path_on(monkeypatch):
    """the "waypoint_dist" option (VLNCE_WAYPOINT_DIST / lib.options(waypoint_dist=1)) is the same
    switch as the attribute"""
    class WithOptions(Recording):
        value = 1

        def effective_option(self, name):
            return self.value if name == "waypoint_dist" else 0

    sim = WithOptions()
    monkeypatch.setattr(_lib, "_LIB", sim)
    _, outs, gold = run("waypoint_hpn_c_64", False)
    compare(outs, gold, atol=1e-4, rtol=1e-4)
    assert sim.calls == ["waypoint_eval"]
    sim.value = 0
    run("waypoint_hpn_c_64", False)
    assert sim.calls == ["waypoint_eval"]
    assert "waypoint_dist" in _lib.HipLib.OPTION_NAMES and "waypoint_dist" not in _lib.HipLib.PER_LAUNCH


def test_fused_and_default_parameter_gradients_agree(monkeypatch):
    monkeypatch.setattr(_lib, "_LIB", WaypointSim())
    grads = {}
    for fused in (False, True):
        policy, outs, _ = run("waypoint_ppo_update_64", fused)
        grads[fused] = ({n: p.grad.clone() for n, p in policy.named_parameters()
                         if p.grad is not None}, outs["ppo_stats"])
    assert set(grads[True][0]) == set(grads[False][0])
    assert torch.allclose(grads[True][1], grads[False][1], rtol=1e-5, atol=1e-6)
    for n, g in grads[False][0].items():
        assert torch.allclose(grads[True][0][n], g, rtol=1e-4, atol=1e-6), n


# ---- flags: a policy whose net hands back given head outputs
def stub_policy(overrides, B, seed=0):
    cfg = vlnce_amd.make_config("WaypointPolicy", **overrides)
    obs_space, act_space = vlnce_amd.make_spaces(64, 64, pano=True)
    policy = vlnce_amd.WaypointPolicy.from_config(cfg, obs_space, act_space)
    policy.fused_distributions = True
    wc, P = policy.wypt_cfg, 12
    g = torch.Generator().manual_seed(seed)
    lim = math.pi / P
    heads = {"logits": torch.randn(B, P + 1, generator=g)}
    actions = {"pano": torch.randint(0, P + 1, (B, 1), generator=g)}
    actions["pano"][0] = P          # a STOP row
    for part, cont, K, (lo, hi), (vlo, vhi) in (
            ("offset", wc.continuous_offset, wc.discrete_offsets, (-lim, lim),
             (wc.min_offset_var, wc.max_offset_var)),
            ("distance", wc.continuous_distance, wc.discrete_distances,
             (wc.min_distance_prediction, wc.max_distance_prediction),
             (wc.min_distance_var, wc.max_distance_var))):
        if cont:
            heads[part] = (lo + (hi - lo) * torch.rand(B, P, generator=g),
                           vlo + (vhi - vlo) * torch.rand(B, P, generator=g))
            actions[part] = lo + (hi - lo) * torch.rand(B, 1, generator=g)
        else:
            heads[part] = (torch.randn(B, P, K, generator=g), None)
            actions[part] = torch.randint(0, K, (B, 1), generator=g)
    features = torch.randn(B, policy.net.output_size, generator=g)
    seen = {}

    def forward(observations, rnn_states, prev_actions, masks, raw_pano_logits=False):
        seen["raw"] = raw_pano_logits
        first = heads["logits"] if raw_pano_logits else CustomFixedCategorical(logits=heads["logits"])
        return (first, *heads["offset"], *heads["distance"], features, rnn_states)

    policy.net.forward = forward
    return policy, heads, actions, seen


def evaluate(policy, actions):
    return policy.evaluate_actions({}, torch.zeros(1), {}, None, actions)


CONT, DISC = {}, {"WAYPOINT.continuous_distance": False, "WAYPOINT.continuous_offset": False}


def test_stub_policy_fused_equals_torch_path_and_is_silent(monkeypatch):
    monkeypatch.setattr(_lib, "_LIB", WaypointSim())
    for overrides in (CONT, DISC):
        policy, heads, actions, seen = stub_policy(overrides, 5)
        v1, lp1, ent1, _ = evaluate(policy, actions)
        assert seen["raw"] is True
        policy.check_eval_flags()
        assert int(policy.eval_flags.abs().sum()) == 0
        policy.fused_distributions = False
        v0, lp0, ent0, _ = evaluate(policy, actions)
        assert seen["raw"] is False
        assert torch.equal(v0, v1) and torch.allclose(lp0, lp1, rtol=1e-5, atol=1e-6)
        assert float(ent1["offset"][0].abs().sum()) == 0.0    # the STOP row: gate 0
        assert float(ent1["distance"][0].abs().sum()) == 0.0
        for k in ent0:
            assert ent0[k].shape == ent1[k].shape and torch.allclose(ent0[k], ent1[k], rtol=1e-5, atol=1e-6)


def defects():
    lim = math.pi / 12

    def loc(part, value):
        def f(heads, actions):
            heads[part][0][1, int(actions["pano"][1]) % 12] = value
        return f

    def var(part):
        def f(heads, actions):
            heads[part][1][1, int(actions["pano"][1]) % 12] = -0.01
        return f

    def elem(part, value):
        def f(heads, actions):
            actions[part][1] = value
        return f

    def pano(heads, actions):
        actions["pano"][1] = 12 + 5

    return [
        ("loc-distance", CONT, loc("distance", 4.2), WP_FLAG_LOC << 8, r"loc is out of range \(0\.25, 4\.0\)"),
        ("loc-offset", CONT, loc("offset", -0.3), WP_FLAG_LOC << 4,
         rf"loc is out of range \({-lim}, {lim}\)"),
        ("variance-distance", CONT, var("distance"), WP_FLAG_VARIANCE << 8, "scale is negative"),
        ("variance-offset", CONT, var("offset"), WP_FLAG_VARIANCE << 4, "scale is negative"),
        ("element-distance", CONT, elem("distance", 0.2), WP_FLAG_ELEMENT << 8,
         "value is out of truncation range and has an undefined log_prob."),
        ("element-offset", CONT, elem("offset", 0.27), WP_FLAG_ELEMENT << 4,
         "value is out of truncation range and has an undefined log_prob."),
        ("pano", CONT, pano, WP_FLAG_PANO, "pano index is outside"),
        ("class-distance", DISC, elem("distance", 6), WP_FLAG_CLASS << 8, "distance class index is outside"),
        ("class-offset", DISC, elem("offset", -1), WP_FLAG_CLASS << 4, "offset class index is outside"),
    ]


@pytest.mark.parametrize("what,overrides,spoil,bit,message", defects(), ids=[d[0] for d in defects()])
def test_check_eval_flags_raises_the_reference_messages(monkeypatch, what, overrides, spoil, bit, message):
    """each flag bit comes from its own defect, NaNs its row alone, and check_eval_flags() raises
    what the torch path raises inside the call (the reference's assertion text)"""
    monkeypatch.setattr(_lib, "_LIB", WaypointSim())
    policy, heads, actions, _ = stub_policy(overrides, 4, seed=3)
    actions["pano"][1] = 7   # the spoilt row is a GO row
    _, clean_lp, clean_ent, _ = evaluate(policy, actions)
    spoil(heads, actions)
    _, lp, ent, _ = evaluate(policy, actions)
    assert policy.eval_flags.tolist() == [0, bit, 0, 0]
    keep = torch.tensor([0, 2, 3])
    assert torch.isnan(lp[1]).all() and torch.equal(lp[keep], clean_lp[keep])
    for k in ent:
        if ent[k].dim() == 2:   # a discrete part's [B, B]: column j is row j's categorical
            assert torch.isnan(ent[k][:, 1]).all() and torch.equal(ent[k][:, keep], clean_ent[k][:, keep]) \
                or what == "pano"
            if what == "pano":   # ... and row i carries row i's gate
                assert torch.isnan(ent[k][1]).all() and torch.isnan(ent[k][:, 1]).all()
                assert torch.equal(ent[k][keep][:, keep], clean_ent[k][keep][:, keep])
            continue
        assert torch.isnan(ent[k][1]) and torch.equal(ent[k][keep], clean_ent[k][keep]), k
    with pytest.raises(AssertionError, match=message):
        policy.check_eval_flags()
    if what.startswith(("loc", "variance", "element")):
        policy.fused_distributions = False   # the torch path raises the same text, inside the call
        with pytest.raises(AssertionError, match=message):
            evaluate(policy, actions)


def test_flags_are_raised_on_weight_zero_and_stop_rows(monkeypatch):
    """the reference asserts on every row, whatever its weight: predict_distance off, and a STOP row"""
    monkeypatch.setattr(_lib, "_LIB", WaypointSim())
    policy, heads, actions, _ = stub_policy({"WAYPOINT.predict_distance": False}, 3, seed=5)
    actions["distance"][2] = 4.5
    actions["offset"][0] = 1.0      # row 0 is the STOP row
    evaluate(policy, actions)
    assert policy.eval_flags.tolist() == [WP_FLAG_ELEMENT << 4, 0, WP_FLAG_ELEMENT << 8]
    with pytest.raises(AssertionError, match="undefined log_prob"):
        policy.check_eval_flags()


def test_backward_is_dense_and_nan_in_a_flagged_row(monkeypatch):
    monkeypatch.setattr(_lib, "_LIB", WaypointSim())
    from vlnce_amd.waypoint_dist import WaypointEvalFn

    policy, heads, actions, _ = stub_policy(CONT, 3, seed=7)
    actions["pano"][1], actions["pano"][2] = 4, 9
    actions["distance"][2] = 9.0
    leaves = [heads["logits"], *heads["offset"], *heads["distance"]]
    for t in leaves:
        t.requires_grad_(True)
    lp, ep, eo, ed, flags = WaypointEvalFn.apply(*leaves, actions["pano"], actions["offset"],
                                                 actions["distance"], policy._eval_spec())
    assert not flags.requires_grad and flags.tolist() == [0, 0, WP_FLAG_ELEMENT << 8]
    (lp[:2].sum() + 2 * eo[:2].sum() + 3 * ed[:2].sum() + 0.5 * ep[:2].sum()).backward()
    for t in leaves:
        assert t.grad.shape == t.shape and torch.isnan(t.grad[2]).all()
    for t in leaves[1:]:
        assert float(t.grad[0].abs().sum()) == 0.0     # STOP row: gate 0
        assert int((t.grad[1] != 0).sum()) == 1 and float(t.grad[1, 4]) != 0.0
