"""GPU tier: vlnce_waypoint_eval / _bwd (csrc/waypoint_dist.hip) on the MI355X against the torch path
of WaypointPolicy.evaluate_actions -- this package's CustomFixedCategorical / TruncatedNormal, the
lines of waypoint_policy.py -- evaluated IN FP64 ON THE CPU WITH AUTOGRAD from the same fp32 inputs
cast to double, with random incoming gradients on all four outputs.

Bound, per tensor (outputs and every gradient): the larger of (a) the fp32 torch path's own error
against that fp64 evaluation, computed here, and (b) 8 * 2^-24 * max|ref| -- one rounding of a saved
partial derivative, one of its product with the incoming gradient, a sum of up to four terms.  The
windows are the fp32 values of the configured ones ([0.25, 2.75], +-pi/12): torch's fp32 arithmetic
rounds the Python floats to fp32 before it uses them, and the descriptor carries them as fp32.

VLNCE_WAYPOINT_DIST_ERRORS=<file> makes the module write its per-case measured errors there (the
source of profiles/waypoint_dist_errors.txt)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import cases
import vlnce_amd
from oracle import thirdparty as tp
from test_oracle_golden import compare
from vlnce_amd import _lib
from vlnce_amd._lib import (WP_CONTINUOUS, WP_DISCRETE, WP_FLAG_CLASS, WP_FLAG_ELEMENT, WP_FLAG_LOC,
                            WP_FLAG_PANO, WP_FLAG_VARIANCE, WaypointPart, WaypointPartGrad)
from vlnce_amd.ppo_harness import PPOConfig, wddppo_minibatch_update
from vlnce_amd.utils import CustomFixedCategorical, TruncatedNormal, batched_index_select
from vlnce_amd.waypoint_dist import WaypointEvalFn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
torch.distributions.Distribution.set_default_validate_args(False)

FLOOR = 8 * 2.0 ** -24
F32 = lambda v: float(np.float32(v))   # noqa: E731
WINDOW = {"distance": (0.25, 2.75), "offset": (F32(-math.pi / 12), F32(math.pi / 12))}
VARIANCE = {"distance": (0.0625, 3.52), "offset": (0.011, 0.0685)}
CLASSES = {"offset": 7, "distance": 6}
KINDS = {"cc": {"offset": WP_CONTINUOUS, "distance": WP_CONTINUOUS},
         "dd": {"offset": WP_DISCRETE, "distance": WP_DISCRETE},
         "dc": {"offset": WP_DISCRETE, "distance": WP_CONTINUOUS}}
PREDICT = [(True, True), (False, True), (True, False), (False, False)]   # (offset, distance)
LEAVES = ("logits", "offset_first", "offset_second", "distance_first", "distance_second")
OUTPUTS = ("log_prob", "ent_pano", "ent_offset", "ent_distance")
MEASURED = {}   # (case, tensor) -> worst (kernel, fp32 torch path) error over the predict_* settings


@pytest.fixture(scope="module", autouse=True)
def error_report():
    yield
    path = os.environ.get("VLNCE_WAYPOINT_DIST_ERRORS")
    if path and MEASURED:
        with open(path, "w") as f:
            f.write("# tests/test_waypoint_dist_gpu.py::test_outputs_and_gradients_against_fp64, worst over the\n"
                    "# four predict_* settings.  Columns: max|kernel - fp64| / max|fp64|, then the same for the\n"
                    f"# fp32 torch path on the CPU.  Bound: the larger of the second column and {FLOOR:.3e}.\n")
            for (case, name), (k, o) in MEASURED.items():
                f.write(f"{case}: {name:18s} {k:.3e}  {o:.3e}\n")
            worst = max(k for k, _ in MEASURED.values())
            f.write(f"# worst kernel error over all cases and tensors: {worst:.3e}\n")


@functools.lru_cache(maxsize=None)
def inputs(B, P, kinds, stop):
    """fp32 CPU tensors.  stop: "some" (about a quarter STOP rows, row 0 always GO when B > 1 and the
    last row always STOP) | "all".  Means and elements inside the windows, element of row 0 exactly
    on lo and of row 1 exactly on hi; variances across the configured ranges."""
    g = torch.Generator().manual_seed(10000 * B + 100 * P + sum(map(ord, kinds + stop)))
    t = {"logits": torch.randn(B, P + 1, generator=g) * 2}
    pano = torch.randint(0, P, (B,), generator=g)
    pano[torch.rand(B, generator=g) < 0.25] = P
    if B > 1:
        pano[0], pano[-1] = 1, P
    if stop == "all":
        pano[:] = P
    t["pano"] = pano.view(B, 1)
    for part, kind in KINDS[kinds].items():
        if kind == WP_CONTINUOUS:
            lo, hi = WINDOW[part]
            vlo, vhi = VARIANCE[part]
            t[part + "_first"] = (lo + (hi - lo) * torch.rand(B, P, generator=g)).clamp(lo, hi)
            t[part + "_second"] = vlo + (vhi - vlo) * torch.rand(B, P, generator=g)
            elem = (lo + (hi - lo) * torch.rand(B, 1, generator=g)).clamp(lo, hi)
            elem[0] = lo
            elem[1 % B] = hi
        else:
            K = CLASSES[part]
            t[part + "_first"] = torch.randn(B, P, K, generator=g) * 1.5
            t[part + "_second"] = None
            elem = torch.randint(0, K, (B, 1), generator=g)
        t[part] = elem
    t["g"] = [torch.randn(B, 1, generator=g), torch.randn(B, generator=g)]   # incoming gradients
    for part, kind in KINDS[kinds].items():   # (offset, distance): a discrete part's entropy is [B, B]
        shape = (B, B) if kind == WP_DISCRETE and B > 1 else (B,)
        t["g"].append(torch.randn(*shape, generator=g))
    return t


def torch_path(t, P, kinds, predict, dtype):
    """waypoint_policy.py's evaluate_actions between the net and its return, on the CPU in `dtype`,
    and the gradients of its four results for the incoming gradients t["g"]"""
    cast = lambda x: None if x is None else x.detach().clone().to(dtype).requires_grad_(True)   # noqa: E731
    leaves = {n: cast(t[n]) for n in LEAVES}
    choice = t["pano"]
    heading = choice % P
    dist = CustomFixedCategorical(logits=leaves["logits"])
    log_prob = dist.log_prob(choice)
    gate = (choice != P).to(log_prob.dtype)
    entropy = {"pano": dist.entropy()}
    for part, on in (("distance", predict[1]), ("offset", predict[0])):
        first, second = leaves[part + "_first"], leaves[part + "_second"]
        if KINDS[kinds][part] == WP_CONTINUOUS:
            lo, hi = WINDOW[part]
            d = TruncatedNormal(loc=first.gather(1, heading), scale=second.gather(1, heading).sqrt(),
                                smin=lo, smax=hi)
            element = t[part].to(dtype)
        else:
            d = CustomFixedCategorical(logits=batched_index_select(first, dim=1, index=heading))
            element = t[part]
        weight = gate * on
        log_prob = log_prob + weight * d.log_prob(element)
        entropy[part] = (weight * d.entropy()).squeeze(1)
    outs = [log_prob, entropy["pano"], entropy["offset"], entropy["distance"]]
    torch.autograd.backward(outs, [g.to(dtype) for g in t["g"]])
    res = dict(zip(OUTPUTS, (o.detach() for o in outs)))
    res.update({"d_" + n: v.grad for n, v in leaves.items() if v is not None})
    return res


@functools.lru_cache(maxsize=None)
def reference(B, P, kinds, stop, predict):
    """(fp64, fp32) evaluations of the torch path on the CPU; computed once per case and shared"""
    t = inputs(B, P, kinds, stop)
    return torch_path(t, P, kinds, predict, torch.float64), torch_path(t, P, kinds, predict, torch.float32)


def spec_of(P, kinds, predict):
    return P, {part: (kind, CLASSES[part] if kind == WP_DISCRETE else 0, *WINDOW[part],
                      float(predict[i]))
               for i, (part, kind) in enumerate(KINDS[kinds].items())}


def fused(t, P, kinds, predict, backward=True):
    """the two launches on the GPU: the four results, the flags and the five gradients"""
    dev = lambda x: None if x is None else x.detach().clone().to(DEV)   # noqa: E731
    leaves = {n: dev(t[n]) for n in LEAVES}
    for v in leaves.values():
        if v is not None:
            v.requires_grad_(True)
    *outs, flags = WaypointEvalFn.apply(*[leaves[n] for n in LEAVES], dev(t["pano"]), dev(t["offset"]),
                                        dev(t["distance"]), spec_of(P, kinds, predict))
    res = dict(zip(OUTPUTS, (o.detach() for o in outs)))
    res["flags"] = flags
    if backward:
        torch.autograd.backward(outs, [g.to(DEV) for g in t["g"]])
        res.update({"d_" + n: v.grad for n, v in leaves.items() if v is not None})
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("kinds", list(KINDS))
@pytest.mark.parametrize("P", [3, 12])
@pytest.mark.parametrize("B", [1, 2, 65, 257])
def test_outputs_and_gradients_against_fp64(B, P, kinds):
    bad = []
    for stop in ("some", "all") if (B, P) == (65, 12) else ("some",):
        t = inputs(B, P, kinds, stop)
        for predict in PREDICT:
            ref64, ref32 = reference(B, P, kinds, stop, predict)
            got = fused(t, P, kinds, predict)
            assert int(got["flags"].abs().sum()) == 0
            assert set(got) - {"flags"} == set(ref64)
            for name, ref in ref64.items():
                k = got[name].cpu().double()
                assert k.shape == ref.shape and got[name].dtype == torch.float32, name
                scale = ref.abs().max().item()
                err = (k - ref).abs().max().item()
                own = (ref32[name].double() - ref).abs().max().item()
                case = f"B={B} P={P} {kinds} stop={stop}"
                rel = (err / scale, own / scale) if scale else (err, own)
                line = f"{case} predict={tuple(map(int, predict))}: {name}  {rel[0]:.3e}  {rel[1]:.3e}"
                print(line)
                was = MEASURED.get((case, name), (0.0, 0.0))
                MEASURED[case, name] = (max(was[0], rel[0]), max(was[1], rel[1]))
                if not err <= max(own, FLOOR * scale):
                    bad.append(line)
    assert not bad, bad


def test_stop_rows_contribute_the_pano_term_only():
    t = inputs(65, 12, "cc", "all")
    got = fused(t, 12, "cc", (True, True))
    ref64, _ = reference(65, 12, "cc", "all", (True, True))
    assert float(got["ent_offset"].abs().sum()) == 0.0 and float(got["ent_distance"].abs().sum()) == 0.0
    for n in LEAVES[1:]:
        assert float(got["d_" + n].abs().sum()) == 0.0 and float(ref64["d_" + n].abs().sum()) == 0.0


@pytest.mark.parametrize("kinds", list(KINDS))
def test_two_runs_give_the_same_bits(kinds):
    t = inputs(257, 12, kinds, "some")
    a, b = fused(t, 12, kinds, (True, True)), fused(t, 12, kinds, (True, True))
    assert set(a) == set(b)
    for n in a:
        assert torch.equal(a[n], b[n]), n


def guarded(numel, dtype=torch.float32, pad=64):
    """(whole buffer, the view the launch writes): NaN (int: a sentinel) on both sides"""
    fill = math.nan if dtype.is_floating_point else 0x5A5A5A5A
    whole = torch.full((numel + 2 * pad,), fill, device=DEV, dtype=dtype)
    return whole, whole[pad:pad + numel]


def intact(whole, numel, pad=64):
    edges = torch.cat([whole[:pad], whole[pad + numel:]])
    return bool(torch.isnan(edges).all()) if whole.is_floating_point() else bool((edges == 0x5A5A5A5A).all())


@pytest.mark.parametrize("kinds", list(KINDS))
@pytest.mark.parametrize("B,P", [(1, 3), (65, 12), (257, 3)])
def test_guard_bands_stay_intact(B, P, kinds):
    """every output and gradient buffer sits between NaN bands: the launches write their own
    elements, all of them, and nothing else"""
    lib = _lib.get_lib()
    t = inputs(B, P, kinds, "some")
    _, spec = spec_of(P, kinds, (True, True))
    dev = lambda x: None if x is None else x.to(DEV).contiguous()   # noqa: E731
    parts = [WaypointPart(*spec[p], dev(t[p + "_first"]), dev(t[p + "_second"]), dev(t[p].view(-1)))
             for p in ("offset", "distance")]
    sizes = [B, B] + [_lib.waypoint_entropy_floats(B, p) for p in parts]
    S = _lib.waypoint_saved_planes(P, parts)
    bufs = {"out": guarded(sum(sizes)), "saved": guarded(S * B), "flags": guarded(B, torch.int32),
            "d_logits": guarded(B * (P + 1))}
    pano = dev(t["pano"].view(-1))
    lib.waypoint_eval(dev(t["logits"]), pano, parts[0], parts[1], B, P, bufs["out"][1],
                      bufs["saved"][1], bufs["flags"][1])
    grads = []
    for p in parts:
        bufs["df_" + str(len(grads))] = guarded(p.first.numel())
        second = None
        if p.kind == WP_CONTINUOUS:
            bufs["ds_" + str(len(grads))] = guarded(B * P)
            second = bufs["ds_" + str(len(grads))][1]
        grads.append(WaypointPartGrad(p.kind, p.K, p.weight, bufs["df_" + str(len(grads))][1], second))
    lib.waypoint_eval_bwd([g.to(DEV).reshape(-1) for g in t["g"]], pano, bufs["saved"][1],
                          bufs["flags"][1], grads[0], grads[1], B, P, bufs["d_logits"][1])
    torch.cuda.synchronize()
    for name, (whole, view) in bufs.items():
        assert intact(whole, view.numel()), name
        if view.is_floating_point():
            assert not torch.isnan(view).any(), name     # every element was written
        else:
            assert int(view.abs().sum()) == 0, name
    want = fused(t, P, kinds, (True, True))
    assert torch.equal(bufs["d_logits"][1].view(B, P + 1), want["d_logits"])
    assert torch.equal(bufs["out"][1][:B], want["log_prob"].view(-1))


def test_entry_points_refuse_before_they_launch():
    lib = _lib.get_lib()
    assert lib.waypoint_eval_supported(1, 1, 0, 0) and lib.waypoint_eval_supported(100000, 63, 32, 32)
    for bad in ((0, 12, 0, 0), (4, 0, 0, 0), (4, 64, 0, 0), (4, 12, 33, 0), (4, 12, 0, 33), (4, 12, -1, 0)):
        assert not lib.waypoint_eval_supported(*bad), bad
    B, P = 4, 12
    t = inputs(B, P, "cc", "some")
    _, spec = spec_of(P, "cc", (True, True))
    dev = lambda x: x.to(DEV).contiguous()   # noqa: E731
    parts = [WaypointPart(*spec[p], dev(t[p + "_first"]), dev(t[p + "_second"]), dev(t[p].view(-1)))
             for p in ("offset", "distance")]
    out = torch.zeros(4 * B, device=DEV)
    saved = torch.zeros(_lib.waypoint_saved_planes(P, parts) * B, device=DEV)
    flags = torch.zeros(B, device=DEV, dtype=torch.int32)
    args = (dev(t["logits"]), dev(t["pano"].view(-1)))
    with pytest.raises(RuntimeError, match="null"):
        lib.waypoint_eval(*args, parts[0]._replace(second=None), parts[1], B, P, out, saved, flags)
    with pytest.raises(RuntimeError, match="kind"):
        lib.waypoint_eval(*args, parts[0]._replace(kind=WP_DISCRETE, K=33, element=args[1], second=None,
                                                   first=torch.zeros(B, P, 33, device=DEV)),
                          parts[1], B, P, out, saved, flags)
    with pytest.raises(RuntimeError, match="saved holds"):
        lib.waypoint_eval(*args, parts[0], parts[1], B, P, out, saved[:-1], flags)
    with pytest.raises(RuntimeError, match="out holds"):
        lib.waypoint_eval(*args, parts[0], parts[1], B, P, out[:-1], saved, flags)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and float(saved.abs().sum()) == 0.0   # nothing ran
    dl = torch.zeros(B, P + 1, device=DEV)
    g = WaypointPartGrad(WP_CONTINUOUS, 0, 1.0, torch.zeros(B, P, device=DEV), torch.zeros(B, P, device=DEV))
    with pytest.raises(RuntimeError, match="null"):
        lib.waypoint_eval_bwd([None] * 4, args[1], saved, flags, g._replace(d_second=None), g, B, P, dl)
    with pytest.raises(RuntimeError, match="null"):
        lib.waypoint_eval_bwd([None] * 4, args[1], saved, flags, g._replace(d_first=None), g, B, P, dl)


def defect_cases():
    P = 12

    def at_heading(name, value):
        def f(t):
            t[name][2, int(t["pano"][2]) % P] = value
        return f

    def elem(name, value):
        def f(t):
            t[name][2] = value
        return f

    return [("loc-distance", "cc", at_heading("distance_first", 2.76), WP_FLAG_LOC << 8),
            ("loc-offset", "cc", at_heading("offset_first", -0.27), WP_FLAG_LOC << 4),
            ("loc-nan", "cc", at_heading("offset_first", math.nan), WP_FLAG_LOC << 4),
            ("variance-distance", "cc", at_heading("distance_second", -0.5), WP_FLAG_VARIANCE << 8),
            ("variance-offset", "cc", at_heading("offset_second", -1e-3), WP_FLAG_VARIANCE << 4),
            ("element-distance", "cc", elem("distance", 0.2), WP_FLAG_ELEMENT << 8),
            ("element-offset", "cc", elem("offset", 0.3), WP_FLAG_ELEMENT << 4),
            ("pano-above", "cc", elem("pano", P + 5), WP_FLAG_PANO),
            ("pano-above-discrete", "dd", elem("pano", P + 5), WP_FLAG_PANO),
            ("pano-negative", "dc", elem("pano", -3), WP_FLAG_PANO),
            ("class-K-distance", "dd", elem("distance", 6), WP_FLAG_CLASS << 8),
            ("class-K-offset", "dc", elem("offset", 7), WP_FLAG_CLASS << 4),
            ("class-negative", "dd", elem("offset", -1), WP_FLAG_CLASS << 4)]


@pytest.mark.parametrize("what,kinds,spoil,bit", defect_cases(), ids=[c[0] for c in defect_cases()])
def test_a_flagged_row_is_nan_and_its_neighbours_are_untouched(what, kinds, spoil, bit):
    """each bit from its own defect, in row 2 of 5 (a GO row); an index outside its range (pano = P +
    5, class = K, negative ones) is never read through.  Both predict weights are 0 in the second
    pass: the reference asserts whatever the weight."""
    B, P = 5, 12
    base = inputs(B, P, kinds, "some")
    clean_t = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in base.items()}
    # (a choice outside [0, P] has no gate: in a discrete part's column sums it counts as a STOP row)
    clean_t["pano"][2] = P if what.startswith("pano") else 7
    t = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in clean_t.items()}
    spoil(t)
    keep = torch.tensor([0, 1, 3, 4], device=DEV)
    for predict in ((True, True), (False, False)):
        clean, got = fused(clean_t, P, kinds, predict), fused(t, P, kinds, predict)
        assert clean["flags"].tolist() == [0] * B and got["flags"].tolist() == [0, 0, bit, 0, 0]
        for n, v in got.items():
            if n == "flags":
                continue
            if v.dim() == 2 and v.shape == (B, B):   # a discrete part's broadcast: column j is row j's
                assert torch.isnan(v[:, 2]).all(), n
                if what.startswith("pano"):
                    assert torch.isnan(v[2]).all(), n
                    assert torch.equal(v[keep][:, keep], clean[n][keep][:, keep]), n
                else:
                    assert torch.equal(v[:, keep], clean[n][:, keep]), n
                continue
            assert torch.isnan(v[2]).all(), n
            assert torch.equal(v[keep], clean[n][keep]), n


# ---- end to end
def to_dev(x):
    if isinstance(x, dict):
        return {k: to_dev(v) for k, v in x.items()}
    return x.to(DEV) if isinstance(x, torch.Tensor) else x


def hip_ppo(policy, sample):
    stats = wddppo_minibatch_update(policy, None, sample, PPOConfig(**cases.PPO), step_grad=False,
                                    clip_grads=False)
    return [float(v) for v in stats]


def run_case(name, fused_distributions):
    case = cases.CASES[name]
    obs, prev, masks, extra, gold = cases.load_case(os.path.join(GOLD, name + ".npz"))
    policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                   tp.synth_state_dict)
    policy.to(DEV)
    policy.fused_distributions = fused_distributions
    outs = cases.run_case(policy, case, to_dev(obs), to_dev(prev), to_dev(masks), to_dev(extra), None,
                          vlnce_amd.AuxLosses, ppo_fn=hip_ppo)
    return policy, outs, gold


@pytest.mark.parametrize("name", ["waypoint_64", "waypoint_discrete_64", "waypoint_hpn_c_64",
                                  "waypoint_hpn_64", "waypoint_ppo_update_64", "waypoint_update_n32_256"])
def test_fused_distributions_match_reference_golden(name):
    policy, outs, gold = run_case(name, True)
    compare(outs, gold, atol=1e-4, rtol=1e-4)
    assert policy.eval_flags is not None and policy.eval_flags.is_cuda
    policy.check_eval_flags()


def test_fused_and_default_parameter_gradients_agree():
    grads = {}
    for mode in (False, True):
        policy, _, _ = run_case("waypoint_ppo_update_64", mode)
        grads[mode] = {n: p.grad.clone() for n, p in policy.named_parameters() if p.grad is not None}
    assert set(grads[True]) == set(grads[False]) and len(grads[True]) > 20
    for n, g in grads[False].items():
        assert torch.allclose(grads[True][n], g, rtol=1e-4, atol=1e-6), n


def test_dispatch_option_switches_the_fused_path_on():
    lib = _lib.get_lib()
    case = cases.CASES["waypoint_hpn_c_64"]
    obs, prev, masks, extra, _ = cases.load_case(os.path.join(GOLD, "waypoint_hpn_c_64.npz"))
    policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                   tp.synth_state_dict)
    policy.to(DEV)
    assert lib.option_default("waypoint_dist") == 0 and policy.fused_distributions is False
    with lib.options(waypoint_dist=1):
        cases.run_case(policy, case, to_dev(obs), to_dev(prev), to_dev(masks), to_dev(extra))
        assert policy.eval_flags is not None
    policy.eval_flags = None
    cases.run_case(policy, case, to_dev(obs), to_dev(prev), to_dev(masks), to_dev(extra))
    assert policy.eval_flags is None


def test_fused_evaluate_actions_and_backward_make_no_host_synchronisation():
    """torch.cuda.set_sync_debug_mode("error") raises on every synchronising call.  A cached-instruction
    batch: the instruction encoder (whose packed-sequence lengths cost one read-back, as upstream)
    hands back the encoding it computed before the mode was switched on.  The fused path then runs
    evaluate_actions, the one-launch PPO loss and backward() without a single synchronisation; the
    default path stops at TruncatedNormal's first bool(...)."""
    name = "waypoint_ppo_update_64"
    case = cases.CASES[name]
    obs, prev, masks, extra, _ = cases.load_case(os.path.join(GOLD, name + ".npz"))
    obs, prev, masks, extra = to_dev(obs), to_dev(prev), to_dev(masks), to_dev(extra)
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            works = False
        except RuntimeError:
            works = True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not works:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() with this runtime")

    def build(fused_distributions):
        policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                       tp.synth_state_dict)
        policy.to(DEV)
        policy.fused_distributions = fused_distributions
        with torch.no_grad():
            cached = policy.net.instruction_encoder(obs)
        policy.net.instruction_encoder.forward = lambda observations: cached
        h0 = extra["h0"][:, :policy.net.num_recurrent_layers].contiguous()

        def step():
            pa = {k: v.clone() for k, v in prev.items()}
            policy.zero_grad(set_to_none=True)
            return wddppo_minibatch_update(policy, None, cases.ppo_sample(obs, pa, masks, extra, h0),
                                           PPOConfig(**cases.PPO), step_grad=False, clip_grads=False)

        for _ in range(3):   # eager, graph capture, replay
            step()
        torch.cuda.synchronize()
        return policy, step

    policy, step = build(True)
    torch.cuda.set_sync_debug_mode("error")
    try:
        stats = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(math.isfinite(float(v)) for v in stats)
    policy.check_eval_flags()
    assert policy.critic.fc.weight.grad is not None

    policy, step = build(False)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError, match="synchroniz"):
            step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
