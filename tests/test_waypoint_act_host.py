"""CPU tier: the host side of the one-launch WaypointPolicy.act (waypoint_act.launch, policy.fused_act,
the "waypoint_act" option, the flag messages) and of ppo_harness.act_for_rollout, run through a
tensor-level simulator of the two new entry points.  `reference_act` and `WaypointActSim` below ARE
their written contract (include/vlnce_hip.h, ABI 154) in plain torch: the panorama choice, the
inverse-CDF draw of the truncated normal, and this package's own TruncatedNormal /
CustomFixedCategorical (utils.py) for log_prob, variance and mode.  The kernels are held to the same
function, evaluated in fp64, by tests/test_waypoint_act_gpu.py."""
import math
import os
import types

import pytest
import torch

import cases
import hostsim
import vlnce_amd
from oracle import thirdparty as tp
from test_oracle_golden import compare
from test_waypoint_dist_host import CONT, DISC, stub_policy
from vlnce_amd import _lib, ppo_harness, waypoint_act
from vlnce_amd._lib import (WP_ABSENT, WP_CONTINUOUS, WP_FLAG_LOC, WP_FLAG_PANO, WP_FLAG_SHIFT,
                            WP_FLAG_VARIANCE)
from vlnce_amd.utils import CustomFixedCategorical, TruncatedNormal, batched_index_select

GOLD = os.path.join(os.path.dirname(__file__), "golden")
torch.distributions.Distribution.set_default_validate_args(False)
WAYPOINT_GOLDENS = ["waypoint_64", "waypoint_discrete_64", "waypoint_hpn_64", "waypoint_hpn_c_64"]
TWO_PI = 2.0 * math.pi


def draw_class(z, u):
    """the contract's categorical draw.  z [B, n] (any float dtype), u [B] fp32 uniforms: the first k
    with sum_{j<=k} p_j > u S, p_j = exp(z_j - max z), the sums running in index order; the last
    class of non-zero probability when there is none.  Also returns, per row, the distance of u S to
    the nearest cumulative boundary as a fraction of S."""
    p = torch.exp(z - z.max(dim=1, keepdim=True).values)
    cum = torch.cumsum(p, dim=1)
    S = cum[:, -1:]
    t = u.to(z.dtype).view(-1, 1) * S
    over = cum > t
    first = over.int().argmax(dim=1)
    n = z.shape[1]
    last = (n - 1) - (p > 0).flip(1).int().argmax(dim=1)
    c = torch.where(over.any(dim=1), first, last)
    margin = ((cum - t).abs() / S).min(dim=1).values
    return c, margin


def reference_act(logits, offset, distance, offset_x, distance_x, deterministic, u, P,
                  dtype=torch.float64, given=None):
    """vlnce_waypoint_act's contract on the CPU in `dtype`.  offset / distance: WaypointPart tuples
    (fp32 tensors), offset_x / distance_x: WaypointActPart tuples (outputs unused).  given: the
    "choices" of another evaluation to take instead of drawing (the fp32 evaluation follows the fp64
    one's classes, so that its error is rounding and not another class).  Returns {name:
    tensor}: integer results as int64, float results in `dtype` except the continuous elements and
    everything derived from them being taken from the element ROUNDED to fp32."""
    B = logits.shape[0]
    nan = math.nan
    bad = ~torch.isfinite(logits).all(dim=1)
    flags = bad.to(torch.int32) * WP_FLAG_PANO
    z = torch.where(bad[:, None], torch.zeros_like(logits), logits).to(dtype)
    head = CustomFixedCategorical(logits=z)
    margins, choices = {}, {}
    if given is not None:
        c = given["pano"]
    elif deterministic:
        c = z.argmax(dim=1)
    else:
        c, margins["pano"] = draw_class(z, u[:, 0])
    c = choices["pano"] = torch.where(bad, torch.full_like(c, P), c)
    h = (c % P).view(B, 1)
    gate = (c != P).to(dtype).view(B, 1)
    log_prob = head.log_prob(c.view(B, 1))
    out = {}
    # (the reference's order: distance, then offset)
    for col, name, part, x in ((2, "distance", distance, distance_x), (1, "offset", offset, offset_x)):
        if part.kind == WP_ABSENT:
            out[name] = dict(metric=torch.full((B,), x.off_metric, dtype=dtype),
                             logged=torch.full((B,), x.off_element, dtype=dtype),
                             variance=torch.zeros(B, dtype=dtype))
            continue
        on = part.weight != 0
        if part.kind == WP_CONTINUOUS:
            lo, hi = part.lo, part.hi
            loc32 = part.first.view(B, P).gather(1, h)
            var32 = part.second.view(B, P).gather(1, h)
            bits = (~((loc32 >= lo) & (loc32 <= hi))).int() * WP_FLAG_LOC \
                | (~(var32.sqrt() >= 0.0)).int() * WP_FLAG_VARIANCE
            ok = bits == 0
            loc = torch.where(ok, loc32, torch.full_like(loc32, 0.5 * (lo + hi))).to(dtype)
            scale = torch.where(ok, var32, torch.ones_like(var32)).to(dtype).sqrt()
            d = TruncatedNormal(loc=loc, scale=scale, smin=lo, smax=hi)
            if deterministic:
                value = d.mode()
            else:
                a, b = (lo - loc) / scale, (hi - loc) / scale
                fa, fb = torch.special.ndtr(a), torch.special.ndtr(b)
                value = loc + scale * torch.special.ndtri(fa + u[:, col:col + 1].to(dtype) * (fb - fa))
            element = value.float().clamp(lo, hi)          # ONE rounding, then the window
            logp = d.log_prob(element.to(dtype))
            r = dict(element=element.view(B), mode=d.mode().view(B), metric=element.to(dtype).view(B),
                     logged=element.to(dtype).view(B), variance=d.variance.view(B))
            if not on:
                r.update(element=torch.full((B,), x.off_element),
                         metric=torch.full((B,), x.off_metric, dtype=dtype),
                         logged=torch.full((B,), x.off_element, dtype=dtype),
                         variance=torch.zeros(B, dtype=dtype))
        else:
            K = part.K
            bits = torch.zeros(B, 1, dtype=torch.int32)
            rows = batched_index_select(part.first.view(B, P, K), dim=1, index=h).to(dtype)
            d = CustomFixedCategorical(logits=rows)
            if given is not None:
                k = given[name]
            elif deterministic:
                k = rows.argmax(dim=1)
            else:
                k, margins[name] = draw_class(rows, u[:, col])
            choices[name] = k
            logp = d.log_prob(k.view(B, 1))
            centre = (x.bin_lo + k.to(dtype) * ((x.bin_hi - x.bin_lo) / (K - 1)))
            r = dict(element=k, mode=d.mode().view(B), metric=centre, logged=centre,
                     variance=d.variance.view(B).to(dtype))     # Categorical.variance: NaN, [B]
            if not on:
                r.update(element=torch.zeros_like(k), metric=torch.full((B,), x.off_metric, dtype=dtype),
                         logged=torch.full((B,), x.bin_lo, dtype=dtype),
                         variance=torch.zeros(B, dtype=dtype))
        flags = flags | (bits.view(B) << WP_FLAG_SHIFT[name])
        if on:
            log_prob = log_prob + gate * part.weight * logp
        out[name] = r
    flagged = flags != 0
    theta = torch.remainder(h.view(B).to(dtype) * (TWO_PI / P) + out["offset"]["metric"].float().to(dtype),
                            TWO_PI)
    stop = ((c == P) | flagged).to(dtype)
    host = torch.stack([stop, out["distance"]["metric"].float().to(dtype), theta,
                        out["distance"]["logged"].float().to(dtype),
                        out["offset"]["logged"].float().to(dtype), out["distance"]["variance"],
                        out["offset"]["variance"], flags.to(dtype)], dim=1)
    host[flagged, 1:7] = nan
    res = {"pano": torch.where(flagged, torch.full_like(c, P), c), "flags": flags, "host_rows": host,
           "log_prob": torch.where(flagged, torch.full_like(log_prob.view(B), nan), log_prob.view(B)),
           "norm_logits": torch.where(flagged[:, None], torch.full_like(head.logits, nan), head.logits),
           "margins": margins, "choices": choices}
    for name in ("offset", "distance"):
        for key in ("element", "mode", "variance"):
            if key not in out[name]:
                continue
            v = out[name][key]
            bad_fill = torch.zeros_like(v) if v.dtype == torch.int64 else torch.full_like(v, nan)
            res[f"{name}_{key}"] = torch.where(flagged, bad_fill, v)
    return res


class WaypointActSim(hostsim.HostSim):
    def __init__(self):
        self.calls = []
        self.option = 0

    def effective_option(self, name):
        return self.option if name == "waypoint_act" else 0

    def waypoint_act_supported(self, B, P, K_offset, K_distance):
        return B >= 1 and 1 <= P <= 63 and 0 <= K_offset <= 32 and 0 <= K_distance <= 32

    def waypoint_act(self, logits, offset, distance, offset_out, distance_out, deterministic, u, B, P,
                     pano, log_prob, norm_logits, host_rows, flags):
        """contract of vlnce_waypoint_act: every row in fp64, one rounding to fp32 per store"""
        self.calls.append("waypoint_act")
        assert self.waypoint_act_supported(B, P, offset.K, distance.K)
        assert (u is None) == bool(deterministic)
        r = reference_act(logits.view(B, P + 1), offset, distance, offset_out, distance_out,
                          deterministic, None if u is None else u.view(B, 3), P)
        pano.copy_(r["pano"])
        flags.copy_(r["flags"])
        log_prob.copy_(r["log_prob"])
        norm_logits.view(B, P + 1).copy_(r["norm_logits"])
        host_rows.view(B, 8).copy_(r["host_rows"])
        for name, part, o in (("offset", offset, offset_out), ("distance", distance, distance_out)):
            if part.kind != WP_ABSENT:
                o.element.copy_(r[name + "_element"])
                o.mode.copy_(r[name + "_mode"])
                o.variance.copy_(r[name + "_variance"])

    def waypoint_history_pick(self, fields, pano, B, P):
        """contract of vlnce_waypoint_history_pick: dst[b] = src[b, pano[b]] for 0 <= pano[b] < P, else 0"""
        self.calls.append("waypoint_history_pick")
        for src, dst in fields:
            assert src.dtype == dst.dtype and src.dtype in (torch.float32, torch.uint8)
            assert dst.shape == (B,) + tuple(src.shape[2:]) and src.shape[1] == P
            for b, p in enumerate(pano.tolist()):
                if 0 <= p < P:
                    dst[b] = src[b, p]
                else:
                    dst[b] = 0


# ---- the four goldens
def run(name, fused_act):
    case = cases.CASES[name]
    obs, prev, masks, extra, gold = cases.load_case(os.path.join(GOLD, name + ".npz"))
    policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                   tp.synth_state_dict)
    policy.fused_act = fused_act
    outs = cases.run_case(policy, case, obs, prev, masks, extra, None, vlnce_amd.AuxLosses)
    return policy, outs, gold


@pytest.mark.parametrize("name", WAYPOINT_GOLDENS)
def test_fused_act_equals_the_default_act_on_the_goldens(monkeypatch, name):
    sim = WaypointActSim()
    monkeypatch.setattr(_lib, "_LIB", sim)
    policy, outs, gold = run(name, True)
    compare(outs, gold, atol=1e-4, rtol=1e-4)
    assert sim.calls == ["waypoint_act"]      # one launch for the whole action
    B = cases.CASES[name]["N"]
    assert len(policy.last_act_rows) == B and all(len(r) == 8 for r in policy.last_act_rows)
    _, default, _ = run(name, False)
    assert sim.calls == ["waypoint_act"]      # the default path issues nothing new
    assert set(default) == set(outs)
    for k, v in default.items():              # the reference's shapes and dtypes
        if isinstance(v, torch.Tensor):
            assert outs[k].shape == v.shape and outs[k].dtype == v.dtype, k
    compare(outs, default, atol=1e-4, rtol=1e-4)


def test_option_and_attribute_are_the_same_switch_and_default_off(monkeypatch):
    sim = WaypointActSim()
    monkeypatch.setattr(_lib, "_LIB", sim)
    assert vlnce_amd.WaypointPolicy.fused_act is False
    assert "waypoint_act" in _lib.HipLib.OPTION_NAMES and "waypoint_act" not in _lib.HipLib.PER_LAUNCH
    policy, _, _, _ = stub_policy(CONT, 4)
    masks = torch.ones(4, 1)
    results = {}
    for attribute, option in ((False, 0), (True, 0), (False, 1)):
        policy.fused_act, sim.option = attribute, option
        sim.calls.clear()
        results[attribute, option] = policy.act({}, torch.zeros(1), {}, masks, deterministic=True)
        assert sim.calls == (["waypoint_act"] if attribute or option else [])
        assert (policy.last_act_rows is not None) == bool(attribute or option)
    a, b = results[True, 0], results[False, 1]
    assert a[1] == b[1] and torch.equal(a[5], b[5])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k])


def test_unsupported_shape_takes_the_torch_path(monkeypatch):
    sim = WaypointActSim()
    sim.waypoint_act_supported = lambda B, P, Ko, Kd: False
    monkeypatch.setattr(_lib, "_LIB", sim)
    policy, outs, gold = run("waypoint_64", True)
    compare(outs, gold, atol=1e-4, rtol=1e-4)
    assert sim.calls == [] and policy.last_act_rows is None


# ---- stub policies: given head outputs
def act(policy, B, deterministic=True):
    return policy.act({}, torch.zeros(1), {}, torch.ones(B, 1), deterministic=deterministic)


@pytest.mark.parametrize("overrides", [CONT, DISC, {"WAYPOINT.predict_distance": False},
                                       {"WAYPOINT.predict_offset": False, **DISC}],
                         ids=["continuous", "discrete", "no-distance", "discrete-no-offset"])
def test_stub_policy_fused_equals_torch_path(monkeypatch, overrides):
    """deterministic act on given head outputs: every member of the 8-tuple, the simulator's actions
    included, and the host rows' logging columns against the trainer's own expressions"""
    monkeypatch.setattr(_lib, "_LIB", WaypointActSim())
    B = 6
    policy, heads, _, seen = stub_policy(overrides, B, seed=11)
    heads["logits"][0, 12] = 9.0       # row 0 stops
    heads["logits"][1, 0] = 9.0        # heading 0
    heads["logits"][2, 11] = 9.0       # heading P - 1
    policy.fused_act = True
    fused = act(policy, B)
    assert seen["raw"] is True
    rows = policy.last_act_rows
    policy.fused_act = False
    default = act(policy, B)
    assert seen["raw"] is False and policy.last_act_rows is None
    assert torch.equal(fused[0], default[0])
    assert [a["action"] == "STOP" for a in fused[1]] == [a["action"] == "STOP" for a in default[1]]
    assert fused[1][0] == {"action": "STOP"} and fused[1][1]["action"]["action"] == "GO_TOWARD_POINT"
    for f, d in zip(fused[1], default[1]):
        if f["action"] != "STOP":
            for k in ("r", "theta"):
                assert f["action"]["action_args"][k] == pytest.approx(d["action"]["action_args"][k],
                                                                      rel=1e-5, abs=1e-6)
    for i in (2, 3, 4):
        assert set(fused[i]) == set(default[i])
        for k, v in default[i].items():
            assert fused[i][k].shape == v.shape and fused[i][k].dtype == v.dtype, (i, k)
            assert torch.allclose(fused[i][k], v, rtol=1e-5, atol=1e-6, equal_nan=True), (i, k)
    assert fused[5].shape == default[5].shape and torch.allclose(fused[5], default[5], rtol=1e-5, atol=1e-5)
    assert torch.allclose(fused[7].logits, default[7].logits, rtol=1e-5, atol=1e-6)
    assert isinstance(fused[7], CustomFixedCategorical)
    for b in range(B):      # what the trainer logs: *_to_continuous of the STORED element
        want = [policy.net.distance_to_continuous(default[2]["distance"][b]).item(),
                policy.net.offset_to_continuous(default[2]["offset"][b]).item(),
                default[4]["distance"][b].item(), default[4]["offset"][b].item()]
        for got, w in zip(rows[b][3:7], want):
            assert got == pytest.approx(w, rel=1e-5, abs=1e-6, nan_ok=True)


def test_sampled_act_is_reproducible_and_inside_the_windows(monkeypatch):
    monkeypatch.setattr(_lib, "_LIB", WaypointActSim())
    B = 64
    policy, heads, _, _ = stub_policy(CONT, B, seed=2)
    policy.fused_act = True
    torch.manual_seed(5)
    a = act(policy, B, deterministic=False)
    torch.manual_seed(5)
    b = act(policy, B, deterministic=False)
    torch.manual_seed(6)
    c = act(policy, B, deterministic=False)
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k])
    assert torch.equal(a[5], b[5]) and a[1] == b[1]
    assert not torch.equal(a[2]["distance"], c[2]["distance"])
    for part in ("distance", "offset"):
        lo, hi = policy._bounds(part)
        assert bool(((a[2][part] >= lo) & (a[2][part] <= hi)).all())
    assert len({int(v) for v in a[2]["pano"]}) > 3
    # the stored log-probability is what evaluate_actions scores for the stored elements
    policy.fused_distributions = False
    _, logp, _, _ = policy.evaluate_actions({}, torch.zeros(1), {}, None, a[2])
    assert torch.allclose(logp, a[5], rtol=1e-5, atol=1e-5)


def defects():
    lim = math.pi / 12

    def loc(part, value):
        def f(heads):
            heads[part][0][1, :] = value
        return f

    def var(part):
        def f(heads):
            heads[part][1][1, :] = -0.01
        return f

    def logit(heads):
        heads["logits"][1, 3] = math.inf

    return [("loc-distance", loc("distance", 4.2), WP_FLAG_LOC << 8, r"loc is out of range \(0\.25, 4\.0\)"),
            ("loc-offset", loc("offset", -0.3), WP_FLAG_LOC << 4, rf"loc is out of range \({-lim}, {lim}\)"),
            ("variance-distance", var("distance"), WP_FLAG_VARIANCE << 8, "scale is negative"),
            ("variance-offset", var("offset"), WP_FLAG_VARIANCE << 4, "scale is negative"),
            ("logit", logit, WP_FLAG_PANO, "panorama logits are not finite")]


@pytest.mark.parametrize("what,spoil,bit,message", defects(), ids=[d[0] for d in defects()])
def test_flags_raise_the_reference_messages(monkeypatch, what, spoil, bit, message):
    """each flag bit comes from its own defect in row 1 of 4; act() raises, from its one read-back,
    what the torch path raises inside its distribution constructors"""
    sim = WaypointActSim()
    monkeypatch.setattr(_lib, "_LIB", sim)
    policy, heads, _, _ = stub_policy(CONT, 4, seed=3)
    policy.fused_act = True
    clean = act(policy, 4)
    spoil(heads)
    with pytest.raises(AssertionError, match=message):
        act(policy, 4)
    assert [int(r[7]) for r in policy.last_act_rows] == [0, bit, 0, 0]
    row = policy.last_act_rows[1]
    assert row[0] == 1.0 and all(math.isnan(v) for v in row[1:7])       # STOP, NaN floats
    res = waypoint_act.launch(heads["logits"], *heads["offset"], *heads["distance"], policy._eval_spec(),
                              policy._act_extras(), True)
    keep = torch.tensor([0, 2, 3])
    assert torch.isnan(res.log_prob[1]).all() and torch.equal(res.log_prob[keep], clean[5][keep])
    assert torch.isnan(res.norm_logits[1]).all() and int(res.pano[1]) == 12
    for k in ("offset", "distance"):
        assert torch.isnan(res.elements[k][1]) and torch.isnan(res.variances[k][1])
        assert torch.equal(res.elements[k][keep], clean[2][k][keep])
    if what != "logit":
        policy.fused_act = False     # the torch path raises the same text
        with pytest.raises(AssertionError, match=message):
            act(policy, 4)


# ---- act_for_rollout
def storage(B, P, step, seed, dtype=torch.float32):
    """the arenas act_for_rollout reads, as both storage classes name them"""
    g = torch.Generator().manual_seed(seed)
    T = 3
    rgb = torch.randint(0, 256, (T + 1, B, P, 5, 7, 3), generator=g).to(dtype)
    depth = torch.rand(T + 1, B, P, 5, 7, 1, generator=g)
    return types.SimpleNamespace(
        step=step, observations={"rgb": rgb, "depth": depth, "angle_features": torch.zeros(T + 1, B, P, 4)},
        prev_actions={k: torch.zeros(T + 1, B, 1) for k in ("pano", "offset", "distance")},
        recurrent_hidden_states=torch.zeros(T + 1, B, 1, 8), masks=torch.ones(T + 1, B, 1))


def reference_loop(policy, rollouts):
    """ddppo_waypoint_trainer.py:160-220, as the trainer writes it"""
    from collections import defaultdict

    step_observation = {k: v[rollouts.step] for k, v in rollouts.observations.items()}
    step_prev_actions = {k: v[rollouts.step] for k, v in rollouts.prev_actions.items()}
    with torch.no_grad():
        outputs = policy.act(step_observation, rollouts.recurrent_hidden_states[rollouts.step],
                             step_prev_actions, rollouts.masks[rollouts.step], deterministic=True)
    (_, actions, action_elements, _, variances, _, _, _) = outputs
    obs_history = {"rgb": torch.zeros_like(step_observation["rgb"][:, 0]),
                   "depth": torch.zeros_like(step_observation["depth"][:, 0])}
    logging_predictions = defaultdict(list)
    for i in range(len(actions)):
        if actions[i]["action"] != "STOP":
            idx = action_elements["pano"][i]
            obs_history["rgb"][i] = step_observation["rgb"][i, idx]
            obs_history["depth"][i] = step_observation["depth"][i, idx]
            logging_predictions["distance_pred"].append(
                policy.net.distance_to_continuous(action_elements["distance"][i]).item())
            logging_predictions["offset_pred"].append(
                policy.net.offset_to_continuous(action_elements["offset"][i]).item())
            logging_predictions["distance_var"].append(variances["distance"][i].item())
            logging_predictions["offset_var"].append(variances["offset"][i].item())
    return outputs, obs_history, logging_predictions


@pytest.mark.parametrize("overrides", [CONT, DISC, {"WAYPOINT.predict_offset": False, **DISC}],
                         ids=["continuous", "discrete", "discrete-no-offset"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "default"])
def test_act_for_rollout_equals_the_reference_loop(monkeypatch, overrides, fused):
    sim = WaypointActSim()
    monkeypatch.setattr(_lib, "_LIB", sim)
    B, P = 5, 12
    policy, heads, _, _ = stub_policy(overrides, B, seed=21)
    heads["logits"][0, P] = 9.0        # STOP: zero history
    heads["logits"][1, 0] = 9.0
    heads["logits"][2, P - 1] = 9.0
    rollouts = storage(B, P, step=2, seed=4)
    policy.fused_act = False
    want_out, want_hist, want_pred = reference_loop(policy, rollouts)
    policy.fused_act = fused
    sim.calls.clear()
    out, hist, pred = ppo_harness.act_for_rollout(policy, rollouts, deterministic=True)
    assert sim.calls == (["waypoint_act", "waypoint_history_pick"] if fused else [])
    assert [a["action"] == "STOP" for a in out[1]] == [a["action"] == "STOP" for a in want_out[1]]
    assert torch.equal(out[2]["pano"], want_out[2]["pano"])
    assert set(hist) == {"rgb", "depth"}
    for k in hist:
        assert hist[k].dtype == want_hist[k].dtype and torch.equal(hist[k], want_hist[k]), k
    assert float(hist["rgb"][0].abs().sum()) == 0.0 and float(hist["rgb"][1].abs().sum()) > 0.0
    assert set(pred) == {"distance_pred", "offset_pred", "distance_var", "offset_var"}
    for k, v in want_pred.items():
        assert len(pred[k]) == len(v) == B - 1
        assert pred[k] == pytest.approx(v, rel=1e-5, abs=1e-6, nan_ok=True), k


def test_act_for_rollout_picks_from_uint8_arenas(monkeypatch):
    """a storage that keeps its RGB arena as uint8: the history keeps the dtype"""
    sim = WaypointActSim()
    monkeypatch.setattr(_lib, "_LIB", sim)
    B, P = 3, 12
    policy, heads, _, _ = stub_policy(CONT, B, seed=8)
    heads["logits"][0, P] = 9.0
    policy.fused_act = True
    rollouts = storage(B, P, step=1, seed=9, dtype=torch.uint8)
    _, hist, _ = ppo_harness.act_for_rollout(policy, rollouts, deterministic=True)
    pano = [int(v) for v in waypoint_act.launch(heads["logits"], *heads["offset"], *heads["distance"],
                                                policy._eval_spec(), policy._act_extras(), True).pano]
    assert hist["rgb"].dtype == torch.uint8 and int(hist["rgb"][0].sum()) == 0
    for b in (1, 2):
        assert torch.equal(hist["rgb"][b], rollouts.observations["rgb"][1, b, pano[b]])
