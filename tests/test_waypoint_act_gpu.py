"""GPU tier: vlnce_waypoint_act / vlnce_waypoint_history_pick (csrc/waypoint_act.hip) on the MI355X.

The act kernel is held to `reference_act` of tests/test_waypoint_act_host.py -- the written contract,
through torch.special.ndtr / ndtri and this package's TruncatedNormal / CustomFixedCategorical --
evaluated IN FP64 ON THE CPU from the same fp32 inputs and the same uploaded noise.  Integer outputs
(panorama, classes, modes) must be EQUAL; the test first asserts that every row's u S keeps at least
1e-9 S from every cumulative boundary (no row is excluded).  Float outputs follow the bound of
tests/test_waypoint_dist_gpu.py: the larger of (a) the same function's own error in fp32 against its
fp64 evaluation (following the fp64 classes, so that it measures rounding) and (b) 8 * 2^-24 *
max|ref|.

VLNCE_WAYPOINT_ACT_ERRORS=<file> makes the module write its measured errors there (the source of
profiles/waypoint_act_errors.txt)."""
import functools
import math
import os
import types

import pytest
import torch

import cases
import vlnce_amd
from oracle import thirdparty as tp
from test_oracle_golden import compare
from test_waypoint_act_host import reference_act, reference_loop
from test_waypoint_dist_gpu import CLASSES, FLOOR, KINDS, PREDICT, VARIANCE, WINDOW, spec_of, to_dev
from vlnce_amd import _lib, ppo_harness, waypoint_act
from vlnce_amd._lib import WP_CONTINUOUS, WaypointActPart, WaypointPart
from vlnce_amd.waypoint_dist import WaypointEvalFn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
torch.distributions.Distribution.set_default_validate_args(False)

# (metric of class 0, of the last class, the `predict_* = False` metric and stored element)
EXTRAS = {"offset": (-math.pi / 12, math.pi / 12, 0.0, 0.0), "distance": (0.25, 2.75, 0.25, 0.25)}
MEASURED = {}   # (case, tensor) -> worst (kernel, fp32 path) relative error


@pytest.fixture(scope="module", autouse=True)
def error_report():
    yield
    path = os.environ.get("VLNCE_WAYPOINT_ACT_ERRORS")
    if path and MEASURED:
        with open(path, "w") as f:
            f.write("# tests/test_waypoint_act_gpu.py::test_act_against_fp64, worst over the four predict_*\n"
                    "# settings.  Columns: max|kernel - fp64| / max|fp64|, then the same for the fp32\n"
                    f"# evaluation on the CPU.  Bound: the larger of the second column and {FLOOR:.3e}.\n")
            for (case, name), (k, o) in MEASURED.items():
                f.write(f"{case}: {name:18s} {k:.3e}  {o:.3e}\n")
            f.write(f"# worst kernel error: {max(k for k, _ in MEASURED.values()):.3e}\n")


@functools.lru_cache(maxsize=None)
def inputs(B, P, kinds, stop):
    """fp32 CPU tensors: logits, the heads' outputs across the configured windows and variance ranges,
    and the noise u (row 0 all zeros when B > 1).  stop == "all": the STOP logit dominates every
    row (and no u is zero: u = 0 takes the first class of non-zero probability, whatever its size)."""
    g = torch.Generator().manual_seed(20000 * B + 100 * P + sum(map(ord, kinds + stop)))
    t = {"logits": torch.randn(B, P + 1, generator=g) * 2}
    if stop == "all":
        t["logits"][:, P] = 60.0
    for part, kind in KINDS[kinds].items():
        if kind == WP_CONTINUOUS:
            lo, hi = WINDOW[part]
            vlo, vhi = VARIANCE[part]
            t[part + "_first"] = (lo + (hi - lo) * torch.rand(B, P, generator=g)).clamp(lo, hi)
            t[part + "_second"] = vlo + (vhi - vlo) * torch.rand(B, P, generator=g)
        else:
            t[part + "_first"] = torch.randn(B, P, CLASSES[part], generator=g) * 1.5
            t[part + "_second"] = None
    u = torch.rand(B, 3, generator=g)
    if B > 1 and stop != "all":
        u[0] = 0.0
    t["u"] = u
    return t


def descriptors(t, P, kinds, predict, device="cpu"):
    _, spec = spec_of(P, kinds, predict)
    mv = lambda x: None if x is None else x.to(device)   # noqa: E731
    parts = {p: WaypointPart(*spec[p], mv(t[p + "_first"]), mv(t[p + "_second"]), None)
             for p in ("offset", "distance")}
    extras = {p: WaypointActPart(*EXTRAS[p], None, None, None) for p in parts}
    return parts, extras


@functools.lru_cache(maxsize=None)
def reference(B, P, kinds, stop, predict, deterministic):
    """(fp64, fp32) evaluations of the contract on the CPU; computed once per case and shared"""
    t = inputs(B, P, kinds, stop)
    parts, extras = descriptors(t, P, kinds, predict)
    args = (t["logits"], parts["offset"], parts["distance"], extras["offset"], extras["distance"],
            deterministic, None if deterministic else t["u"], P)
    r64 = reference_act(*args, dtype=torch.float64)
    return r64, reference_act(*args, dtype=torch.float32, given=r64["choices"])


def kernel(t, P, kinds, predict, deterministic):
    _, spec = spec_of(P, kinds, predict)
    dev = lambda x: None if x is None else x.to(DEV)   # noqa: E731
    res = waypoint_act.launch(dev(t["logits"]), dev(t["offset_first"]), dev(t["offset_second"]),
                              dev(t["distance_first"]), dev(t["distance_second"]), (P, spec),
                              {p: EXTRAS[p] for p in EXTRAS}, deterministic,
                              None if deterministic else dev(t["u"]))
    torch.cuda.synchronize()
    B = t["logits"].shape[0]
    got = {"pano": res.pano.view(B), "flags": res.flags, "log_prob": res.log_prob.view(B),
           "norm_logits": res.norm_logits, "host_rows": res.host_rows}
    for p in ("offset", "distance"):
        got[p + "_element"], got[p + "_mode"] = res.elements[p].view(B), res.modes[p].view(B)
        got[p + "_variance"] = res.variances[p].view(B)
    return {k: v.cpu() for k, v in got.items()}


CASES = [(B, P, kinds, "some") for B in (1, 3, 67) for P in (12, 1) for kinds in KINDS] \
    + [(67, 12, kinds, "all") for kinds in KINDS]


@pytest.mark.parametrize("B,P,kinds,stop", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_act_against_fp64(B, P, kinds, stop):
    t = inputs(B, P, kinds, stop)
    bad = []
    for predict in PREDICT:
        for deterministic in (True, False):
            ref64, ref32 = reference(B, P, kinds, stop, predict, deterministic)
            for part, margin in ref64["margins"].items():   # no draw sits on a class boundary
                assert float(margin.min()) >= 1e-9, (part, float(margin.min()))
            got = kernel(t, P, kinds, predict, deterministic)
            assert int(got["flags"].abs().sum()) == 0
            if stop == "all":
                assert got["pano"].tolist() == [P] * B and got["host_rows"][:, 0].tolist() == [1.0] * B
            case = f"B={B} P={P} {kinds} stop={stop}"
            tag = f"{case} predict={tuple(map(int, predict))} det={int(deterministic)}"
            for name, ref in ref64.items():
                if name in ("margins", "choices"):
                    continue
                k = got[name]
                assert k.shape == ref.shape, (name, k.shape, ref.shape)
                if not ref.dtype.is_floating_point:      # panorama, classes, modes, flags
                    assert torch.equal(k.to(ref.dtype), ref), (tag, name, k.tolist(), ref.tolist())
                    continue
                assert k.dtype == torch.float32, name
                k, ref, own = k.double(), ref.double(), ref32[name].double()
                assert torch.equal(torch.isnan(k), torch.isnan(ref)), (tag, name)   # Categorical.variance
                k, ref, own = torch.nan_to_num(k), torch.nan_to_num(ref), torch.nan_to_num(own)
                scale = ref.abs().max().item()
                err, own = (k - ref).abs().max().item(), (own - ref).abs().max().item()
                rel = (err / scale, own / scale) if scale else (err, own)
                line = f"{tag}: {name}  {rel[0]:.3e}  {rel[1]:.3e}"
                print(line)
                was = MEASURED.get((case, name), (0.0, 0.0))
                MEASURED[case, name] = (max(was[0], rel[0]), max(was[1], rel[1]))
                if not err <= max(own, FLOOR * scale):
                    bad.append(line)
            if not deterministic:
                for part, kind in KINDS[kinds].items():
                    if kind == WP_CONTINUOUS and predict[part == "distance"]:
                        lo, hi = WINDOW[part]
                        e = got[part + "_element"]
                        assert bool(((e >= lo) & (e <= hi)).all()), part
                        if B > 1 and stop != "all":   # u = 0: the window's lower end
                            assert float(e[0]) == pytest.approx(lo, abs=1e-6), part
    assert not bad, bad


@pytest.mark.parametrize("kinds", list(KINDS))
def test_two_runs_give_the_same_bits(kinds):
    t = inputs(67, 12, kinds, "some")
    a, b = (kernel(t, 12, kinds, (True, True), False) for _ in range(2))
    for n in a:   # (a discrete part's variance is NaN)
        assert torch.equal(torch.isnan(a[n]), torch.isnan(b[n])), n
        assert torch.equal(torch.nan_to_num(a[n]), torch.nan_to_num(b[n])), n


@pytest.mark.parametrize("kinds", list(KINDS))
@pytest.mark.parametrize("predict", PREDICT, ids=[f"{int(o)}{int(d)}" for o, d in PREDICT])
def test_eval_scores_the_drawn_elements_with_the_same_number(kinds, predict):
    """vlnce_waypoint_eval on the drawn elements returns the act kernel's log_prob within the floor,
    and raises none of evaluate_actions' range flags: the first PPO ratio is 1"""
    B, P = 67, 12
    t = inputs(B, P, kinds, "some")
    got = kernel(t, P, kinds, predict, False)
    dev = lambda x: None if x is None else x.to(DEV)   # noqa: E731
    lp, _, _, _, flags = WaypointEvalFn.apply(
        dev(t["logits"]), dev(t["offset_first"]), dev(t["offset_second"]), dev(t["distance_first"]),
        dev(t["distance_second"]), dev(got["pano"]), dev(got["offset_element"]),
        dev(got["distance_element"]), spec_of(P, kinds, predict))
    assert int(flags.abs().sum()) == 0
    act_lp = got["log_prob"].double()
    err = (lp.view(B).cpu().double() - act_lp).abs().max().item()
    print(f"{kinds} predict={predict}: |eval - act| = {err:.3e}, floor {FLOOR * act_lp.abs().max().item():.3e}")
    assert err <= FLOOR * act_lp.abs().max().item()


# ---- the distribution of the draws: 4096 rows that share one set of head outputs
N_ROWS = 4096
KS_BOUND = math.sqrt(-math.log(5e-7) / 2) / math.sqrt(N_ROWS)     # the 1e-6 critical value, 0.0421
Z_1E6 = 4.753424
CHI2_BOUND = 12 * (1 - 2 / (9 * 12) + Z_1E6 * math.sqrt(2 / (9 * 12))) ** 3   # Wilson-Hilferty, ~51.8
PANO_LOGITS = [0.3 * ((5 * i) % 13) - 2.4 for i in range(13)]
SHAPES = {   # (position of loc in the window, variance): little truncation | heavy truncation at an edge
    "wide": {"distance": (0.45, VARIANCE["distance"][0]), "offset": (0.5, VARIANCE["offset"][0])},
    "narrow": {"distance": (0.05, VARIANCE["distance"][1]), "offset": (0.97, VARIANCE["offset"][1])},
}


@functools.lru_cache(maxsize=None)
def shared_heads(shape):
    g = torch.Generator().manual_seed(1234)
    t = {"logits": torch.tensor(PANO_LOGITS).repeat(N_ROWS, 1), "u": torch.rand(N_ROWS, 3, generator=g)}
    for part, (pos, var) in SHAPES[shape].items():
        lo, hi = WINDOW[part]
        t[part + "_first"] = torch.full((N_ROWS, 12), lo + pos * (hi - lo)).clamp(lo, hi)
        t[part + "_second"] = torch.full((N_ROWS, 12), var)
    return t


def ks_distance(x, loc, var, lo, hi):
    """sup |F_n - F| of the sample x against the truncated normal's CDF, in fp64"""
    x = x.double().sort().values
    s = math.sqrt(var)
    ndtr = torch.special.ndtr
    fa, fb = ndtr(torch.tensor((lo - loc) / s).double()), ndtr(torch.tensor((hi - loc) / s).double())
    F = (ndtr((x - loc) / s) - fa) / (fb - fa)
    n = x.numel()
    i = torch.arange(1, n + 1, dtype=torch.float64)
    return max(float((i / n - F).max()), float((F - (i - 1) / n).max()))


def chi_square(choices):
    p = torch.softmax(torch.tensor(PANO_LOGITS).double(), 0)
    expected = p * N_ROWS
    counts = torch.bincount(choices, minlength=13).double()
    return float(((counts - expected) ** 2 / expected).sum()), float(expected.min())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_draws_follow_their_distributions(shape):
    t = shared_heads(shape)
    parts, extras = descriptors(t, 12, "cc", (True, True))
    ref = reference_act(t["logits"], parts["offset"], parts["distance"], extras["offset"],
                        extras["distance"], False, t["u"], 12)
    stats = {}
    for who, r in (("cpu", ref), ("gpu", None)):
        if r is None:   # the reference figures stand before the GPU's are looked at
            r = kernel(t, 12, "cc", (True, True), False)
        for part in ("distance", "offset"):
            pos, var = SHAPES[shape][part]
            lo, hi = WINDOW[part]
            loc = float(t[part + "_first"][0, 0])
            stats[who, part] = ks_distance(r[part + "_element"], loc, float(t[part + "_second"][0, 0]), lo, hi)
            print(f"{shape} {who} KS {part}: {stats[who, part]:.4f} (bound {KS_BOUND:.4f})")
            assert stats[who, part] < KS_BOUND, (who, part)
        chi, smallest = chi_square(r["pano"])
        print(f"{shape} {who} chi-square over 13 classes: {chi:.2f} (bound {CHI2_BOUND:.1f}), "
              f"smallest expected count {smallest:.1f}")
        assert smallest >= 5.0 and chi < CHI2_BOUND, who
    assert abs(KS_BOUND - 0.0421) < 1e-4 and abs(CHI2_BOUND - 51.8) < 0.1


# ---- the history pick, bit for bit against the Python loop
def python_pick(src, pano, P):
    out = torch.zeros((src.shape[0],) + tuple(src.shape[2:]), dtype=src.dtype)
    for b, p in enumerate(pano.tolist()):
        if 0 <= p < P:
            out[b] = src[b, p]
    return out


@pytest.mark.parametrize("strided", [False, True], ids=["rows", "arena-slice"])
def test_history_pick_bit_for_bit(strided):
    """E = 105 (no 16-byte path), 256 (16-byte path), 4104 (two chunks), fp32 and uint8, one launch for
    the six fields; B = 3: a STOP row, pano = 0, pano = P - 1.  The destinations sit between guard
    bands."""
    lib = _lib.get_lib()
    B, P, T = 3, 12, 3
    g = torch.Generator().manual_seed(7)
    pano = torch.tensor([P, 0, P - 1])
    fields, want, bands = [], [], []
    for E in (105, 256, 4104):
        for dtype in (torch.float32, torch.uint8):
            shape = (B, T, P, E) if strided else (T, B, P, E)
            arena = torch.randint(1, 256, shape, generator=g).to(dtype)
            src = arena.to(DEV)
            src = src[:, 1] if strided else src[1]
            assert src.shape == (B, P, E) and src.is_contiguous() != strided
            whole = torch.full((B * E + 128,), 90, device=DEV, dtype=dtype)    # 64 guard elements a side
            fields.append((src, whole[64:64 + B * E].view(B, E)))
            bands.append((whole, B * E))
            want.append(python_pick(arena[:, 1] if strided else arena[1], pano, P))
    lib.waypoint_history_pick(fields, pano.to(DEV), B, P)
    torch.cuda.synchronize()
    for (src, dst), ref, (whole, n) in zip(fields, want, bands):
        assert torch.equal(dst.cpu(), ref), (dst.dtype, dst.shape)
        assert float(dst[0].float().abs().sum()) == 0.0 and float(dst[1].float().abs().sum()) > 0.0
        assert bool((torch.cat([whole[:64], whole[64 + n:]]) == 90).all())


def test_entry_points_refuse_before_they_launch():
    lib = _lib.get_lib()
    assert lib.waypoint_act_supported(1, 1, 0, 0) and lib.waypoint_act_supported(100000, 63, 32, 32)
    for bad in ((0, 12, 0, 0), (4, 0, 0, 0), (4, 64, 0, 0), (4, 12, 33, 0), (4, 12, 0, 33)):
        assert not lib.waypoint_act_supported(*bad), bad
    B, P = 4, 12
    t = inputs(3, P, "cc", "some")
    parts, _ = descriptors(t, P, "cc", (True, True), DEV)
    f = lambda n: torch.zeros(n, device=DEV)   # noqa: E731
    outs = [WaypointActPart(*EXTRAS[p], f(3), f(3), f(3)) for p in ("offset", "distance")]
    args = dict(pano=torch.zeros(3, device=DEV, dtype=torch.int64), log_prob=f(3),
                norm_logits=f(3 * 13), host_rows=f(24), flags=torch.zeros(3, device=DEV, dtype=torch.int32))
    logits = t["logits"].to(DEV)
    with pytest.raises(RuntimeError, match="null noise"):
        lib.waypoint_act(logits, parts["offset"], parts["distance"], *outs, False, None, 3, P, **args)
    with pytest.raises(RuntimeError, match="null"):
        lib.waypoint_act(logits, parts["offset"]._replace(second=None), parts["distance"], *outs, True,
                         None, 3, P, **args)
    with pytest.raises(RuntimeError, match="null output"):
        lib.waypoint_act(logits, parts["offset"], parts["distance"], outs[0]._replace(variance=None),
                         outs[1], True, None, 3, P, **args)
    torch.cuda.synchronize()
    assert float(args["host_rows"].abs().sum()) == 0.0     # nothing ran
    src, dst = torch.zeros(B, P, 8, device=DEV), torch.zeros(B, 8, device=DEV)
    with pytest.raises(RuntimeError, match="fields"):
        lib.waypoint_history_pick([(src, dst)] * 9, torch.zeros(B, device=DEV, dtype=torch.int64), B, P)


# ---- policy level
def run_case(name, fused_act):
    case = cases.CASES[name]
    obs, prev, masks, extra, gold = cases.load_case(os.path.join(GOLD, name + ".npz"))
    policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                   tp.synth_state_dict)
    policy.to(DEV)
    policy.fused_act = fused_act
    outs = cases.run_case(policy, case, to_dev(obs), to_dev(prev), to_dev(masks), to_dev(extra), None,
                          vlnce_amd.AuxLosses)
    return policy, outs, gold


@pytest.mark.parametrize("name", ["waypoint_64", "waypoint_discrete_64", "waypoint_hpn_64", "waypoint_hpn_c_64"])
def test_fused_act_matches_reference_golden(name):
    policy, outs, gold = run_case(name, True)
    compare(outs, gold, atol=1e-4, rtol=1e-4)
    assert policy.last_act_rows is not None and len(policy.last_act_rows) == cases.CASES[name]["N"]
    assert vlnce_amd.WaypointPolicy.fused_act is False and _lib.get_lib().option_default("waypoint_act") == 0


@functools.lru_cache(maxsize=None)
def live_policy(name="waypoint_64"):
    case = cases.CASES[name]
    obs, prev, masks, extra, _ = cases.load_case(os.path.join(GOLD, name + ".npz"))
    policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                   tp.synth_state_dict)
    policy.to(DEV)
    h0 = extra["h0"][:, :policy.net.num_recurrent_layers].contiguous()
    return policy, to_dev(obs), to_dev(prev), to_dev(masks), h0.to(DEV)


def test_sampled_act_is_seeded_and_stays_inside_the_windows():
    """same seed, same bits; another seed, another batch.  The net is run ONCE and its outputs are held
    for the three calls: on the same inputs its own outputs move in their last bits from call to call
    (measured: up to 3.6e-7 on the logits), which is not what this test is about."""
    policy, obs, prev, masks, h0 = live_policy()
    with torch.no_grad():
        held = policy.net(obs, h0, {k: v.clone() for k, v in prev.items()}, masks, raw_pano_logits=True)
    held = [None if t is None else t.clone() for t in held]

    def sample(seed):
        torch.manual_seed(seed)
        with torch.no_grad():
            return policy.act(obs, h0, {k: v.clone() for k, v in prev.items()}, masks, deterministic=False)

    policy.fused_act = True
    policy.net.forward = lambda *a, raw_pano_logits=False: tuple(held)
    try:
        a, b, c = sample(3), sample(3), sample(4)
    finally:
        del policy.net.forward
        policy.fused_act = False
    assert a[1] == b[1] and torch.equal(a[5], b[5]) and torch.equal(a[0], b[0])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    assert not all(torch.equal(a[2][k], c[2][k]) for k in a[2])
    for part in ("distance", "offset"):
        lo, hi = policy._bounds(part)
        for run in (a, c):
            assert bool(((run[2][part] >= lo) & (run[2][part] <= hi)).all()), part


def test_option_switches_the_fused_act_on():
    lib = _lib.get_lib()
    policy, obs, prev, masks, h0 = live_policy()
    policy.fused_act = False
    with torch.no_grad():
        with lib.options(waypoint_act=1):
            policy.act(obs, h0, {k: v.clone() for k, v in prev.items()}, masks, deterministic=True)
            assert policy.last_act_rows is not None
        policy.act(obs, h0, {k: v.clone() for k, v in prev.items()}, masks, deterministic=True)
    assert policy.last_act_rows is None


def test_act_for_rollout_against_the_default_path():
    """one step out of vlnce_amd.ActionDictRolloutStorage: the fused step against the reference's loop
    over the default act()"""
    policy, obs, prev, masks, h0 = live_policy()
    N = masks.shape[0]
    space = types.SimpleNamespace(spaces={k: types.SimpleNamespace(shape=tuple(v.shape[1:]))
                                          for k, v in obs.items()})
    rollouts = vlnce_amd.ActionDictRolloutStorage(2, N, space, h0.shape[-1],
                                                  num_recurrent_layers=h0.shape[1], device=DEV)
    rollouts.step = 1
    for k, v in rollouts.observations.items():
        v[1].copy_(obs[k])
    rollouts.recurrent_hidden_states[1].copy_(h0)
    rollouts.masks[1].copy_(masks)
    for k, v in rollouts.prev_actions.items():
        v[1].copy_(prev[k])
    # both of the fixture's environments stop: the STOP logit's bias is lowered for the length of this test
    bias = policy.net.stop_linear.bias
    try:
        with torch.no_grad():
            bias.sub_(4.0)
        policy.fused_act = False
        want_out, want_hist, want_pred = reference_loop(policy, rollouts)
        stops = [a["action"] == "STOP" for a in want_out[1]]
        policy.fused_act = True
        out, hist, pred = ppo_harness.act_for_rollout(policy, rollouts, deterministic=True)
    finally:
        policy.fused_act = False
        with torch.no_grad():
            bias.add_(4.0)
    assert not all(stops)
    assert [a["action"] == "STOP" for a in out[1]] == stops
    assert torch.equal(out[2]["pano"], want_out[2]["pano"])
    for k in ("rgb", "depth"):
        assert hist[k].shape == want_hist[k].shape and torch.equal(hist[k], want_hist[k]), k
    for k, v in want_pred.items():
        assert pred[k] == pytest.approx(v, rel=1e-4, abs=1e-5, nan_ok=True), k
    for i in (2, 3, 4):
        for k, v in want_out[i].items():
            assert torch.allclose(out[i][k].float(), v.float(), rtol=1e-4, atol=1e-5, equal_nan=True), (i, k)
    assert torch.allclose(out[5], want_out[5], rtol=1e-4, atol=1e-4)
