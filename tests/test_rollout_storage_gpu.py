"""GPU tier of the device rollout storage: vlnce_rollout_copy / vlnce_rollout_gather against torch
indexing, bit for bit, over the shapes where they can go wrong; vlnce_ppo_advantages against the same
formula in fp64; the reference's golden script, a pass under torch's synchronisation debug mode and
an end-to-end WDDPPO update through the real class.

Every arena, source and output of the kernel tests lives inside a larger buffer filled with a
sentinel, and after each call the WHOLE buffer equals the expected clone: nothing outside the target
rows changed.

VLNCE_ROLLOUT_STORAGE_ERRORS=<file> makes the module write what it measured there (the committed
copy is profiles/rollout_storage_errors.txt)."""
import os
import warnings

import numpy as np
import pytest
import torch

import cases
import rollout_cases as rc
import vlnce_amd
from oracle import thirdparty as tp
from vlnce_amd import _lib
from vlnce_amd._lib import RolloutCopyField, RolloutGatherField
from vlnce_amd.optim import Adam
from vlnce_amd.ppo_harness import PPOConfig, wddppo_minibatch_update, wddppo_update
from vlnce_amd.rollout_storage import ActionDictRolloutStorage

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
GUARD = 64           # elements either side: a multiple of 16 bytes for every dtype
MEASURED = []        # lines of the error report
SENTINEL = {torch.float32: -777.0, torch.int64: -777, torch.uint8: 0xA5, torch.float16: -7.0}
# single element, no 16-byte multiple (840 bytes), one whole chunk, more than one chunk with a ragged end
ROW_SIZES = (1, 210, 4096, 70001)
PAIRS = ((torch.float32, torch.float32), (torch.int64, torch.int64), (torch.uint8, torch.uint8),
         (torch.bool, torch.uint8), (torch.int64, torch.float32), (torch.uint8, torch.float32),
         (torch.bool, torch.float32), (torch.float32, torch.int64), (torch.float32, torch.uint8))
torch.distributions.Distribution.set_default_validate_args(False)


@pytest.fixture(scope="module", autouse=True)
def error_report():
    yield
    path = os.environ.get("VLNCE_ROLLOUT_STORAGE_ERRORS")
    if path and MEASURED:
        with open(path, "w") as f:
            f.write("# tests/test_rollout_storage_gpu.py.  vlnce_ppo_advantages, normalised: worst over the\n"
                    "# elements of |kernel - fp64| / (2^-23 |fp64| + 2^-40 max|fp64|), which the test holds\n"
                    "# to 1.  Then the end-to-end WDDPPO update: the two torch-indexed baseline runs against\n"
                    "# each other, and the storage's run against the first.\n")
            f.write("\n".join(MEASURED) + "\n")


def lib():
    return _lib.get_lib()


def values(numel, dtype, gen, target=None):
    """values on the CPU; for a narrowing pair only what the target represents exactly"""
    if dtype == torch.float32:
        if target == torch.uint8:
            return torch.randint(0, 256, (numel,), generator=gen).float()
        if target == torch.int64:
            return torch.randint(-2 ** 20, 2 ** 20, (numel,), generator=gen).float()
        return torch.randn(numel, generator=gen) * 100
    if dtype == torch.int64:
        return torch.randint(-2 ** 40, 2 ** 40, (numel,), generator=gen)
    if dtype == torch.bool:
        return torch.rand(numel, generator=gen) > 0.5
    if dtype == torch.float16:
        return torch.randn(numel, generator=gen).half()
    return torch.randint(0, 256, (numel,), generator=gen).to(torch.uint8)


def guarded(numel, dtype, shift=0):
    """(buffer, view of numel elements `shift` elements past the guard): sentinel everywhere"""
    store = torch.uint8 if dtype == torch.bool else dtype
    buf = torch.full((numel + 2 * GUARD + shift,), SENTINEL[store], dtype=store, device=DEV)
    view = buf[GUARD + shift:GUARD + shift + numel]
    return buf, (view.view(torch.bool) if dtype == torch.bool else view)


def copy_case(E, sdt, ddt, n_rows, layout, gen):
    """one field: rows 1 of a [3, n_rows, E] arena <- n_rows source rows; returns (field, check)"""
    shift = 1 if layout == "shifted" else 0
    # a crop of a wider tensor: with E a multiple of 4 the fp32 row stride stays a multiple of 16 bytes
    width = 2 * E + 4 if layout == "row stride" else E
    sbuf, sview = guarded(n_rows * width, sdt, shift)
    src_cpu = values(n_rows * width, sdt, gen, ddt).view(n_rows, width)
    sview.copy_(src_cpu.view(-1))
    src = sview.view(n_rows, width)[:, :E]
    abuf, aview = guarded(3 * n_rows * E, ddt)
    arena = aview.view(3, n_rows, E)
    want_buf, want_view = abuf.clone(), None
    want_view = want_buf[GUARD:GUARD + 3 * n_rows * E].view(3, n_rows, E)
    want_view[1] = src_cpu[:, :E].to(ddt).to(DEV)
    src_before = sbuf.clone()
    field = RolloutCopyField(src, arena[1], E, width, E)

    def check():
        assert torch.equal(abuf, want_buf), f"E={E} {sdt}->{ddt} rows={n_rows} {layout}"
        assert torch.equal(sbuf, src_before), "the source changed"

    return field, check


# ------------------------------------------------------------------ vlnce_rollout_copy
@pytest.mark.parametrize("layout", ["contiguous", "shifted", "row stride"])
@pytest.mark.parametrize("n_rows", [1, 3])
def test_copy_every_row_size_in_one_launch(n_rows, layout):
    gen = torch.Generator().manual_seed(n_rows)
    made = [copy_case(E, torch.float32, torch.float32, n_rows, layout, gen) for E in ROW_SIZES]
    made += [copy_case(E, torch.uint8, torch.uint8, n_rows, layout, gen) for E in (1, 4096 + 16, 70001)]
    made += [copy_case(E, torch.int64, torch.int64, n_rows, layout, gen) for E in (1, 210, 4097)]
    lib().rollout_copy([f for f, _ in made], n_rows)
    torch.cuda.synchronize()
    for _, check in made:
        check()


@pytest.mark.parametrize("sdt,ddt", PAIRS)
def test_copy_every_supported_pair(sdt, ddt):
    assert lib().rollout_copy_supported(sdt, ddt)
    gen = torch.Generator().manual_seed(7)
    made = [copy_case(E, sdt, ddt, 3, layout, gen)
            for E, layout in ((1, "contiguous"), (5, "row stride"), (300, "contiguous"),
                              (4096, "contiguous"), (4096, "shifted"), (4100, "row stride"))]
    lib().rollout_copy([f for f, _ in made], 3)
    torch.cuda.synchronize()
    for _, check in made:
        check()


def test_copy_supported_says_no_to_everything_else():
    ok = set(PAIRS)
    for s in (torch.float32, torch.int64, torch.uint8, torch.bool, torch.float16, torch.float64,
              torch.int32):
        for d in (torch.float32, torch.int64, torch.uint8, torch.float16, torch.float64, torch.int32):
            assert lib().rollout_copy_supported(s, d) == ((s, d) in ok), (s, d)


def test_copy_of_a_full_table_and_refusals():
    gen = torch.Generator().manual_seed(3)
    made = [copy_case(1 + 37 * k, torch.float32, torch.float32, 2, "contiguous", gen) for k in range(32)]
    lib().rollout_copy([f for f, _ in made], 2)
    torch.cuda.synchronize()
    for _, check in made:
        check()
    with pytest.raises(RuntimeError, match="33 fields"):
        lib().rollout_copy([f for f, _ in made] + [made[0][0]], 2)
    with pytest.raises(RuntimeError, match="bad argument"):
        lib().rollout_copy([made[0][0]], 0)
    for _, check in made:   # a refused call launched nothing
        check()


# ------------------------------------------------------------------ vlnce_rollout_gather
def gather_case(E, dtype, rows, N, T, envs, gen, shift=0, once=False, out_N=None, column=0):
    """one field: arena [rows, N, E] (rows >= T), out [T_f, out_N, E] written from `column` on"""
    n = len(envs)
    out_N = n if out_N is None else out_N
    Tf = 1 if once else T
    abuf, aview = guarded(rows * N * E, dtype, shift)
    arena_cpu = values(rows * N * E, dtype, gen).view(rows, N, E)
    aview.copy_(arena_cpu.view(-1))
    obuf, oview = guarded(Tf * out_N * E, dtype)
    want_buf = obuf.clone()
    want = want_buf[GUARD:GUARD + Tf * out_N * E].view(Tf, out_N, E)
    want[:, column:column + n] = arena_cpu[:Tf][:, envs].to(DEV)
    arena_before = abuf.clone()
    field = RolloutGatherField(aview.view(rows, N, E), oview.view(Tf, out_N, E), E, N, out_N, column, once)

    def check():
        assert torch.equal(obuf, want_buf), f"E={E} {dtype} T={T} envs={envs} shift={shift} once={once}"
        assert torch.equal(abuf, arena_before), "the arena changed"

    return field, check


@pytest.mark.parametrize("T,envs", [(3, [2]), (3, [4, 0, 3, 1, 2]), (1, [1, 3]), (2, [3, 3, 0])],
                         ids=["one env", "all envs", "one step", "partial rollout"])
def test_gather_every_row_size_in_one_launch(T, envs):
    gen = torch.Generator().manual_seed(T)
    rows, N = 4, 5   # the arenas carry the bootstrap row; a partial rollout leaves more rows unread
    made = [gather_case(E, torch.float32, rows, N, T, envs, gen) for E in ROW_SIZES]
    made += [gather_case(4096, torch.float32, rows, N, T, envs, gen, shift=1),
             gather_case(70001, torch.float32, rows, N, T, envs, gen, shift=1)]
    made += [gather_case(E, torch.uint8, rows, N, T, envs, gen) for E in (1, 4096 + 16, 70001)]
    made += [gather_case(E, torch.int64, rows, N, T, envs, gen) for E in (1, 210, 4098)]
    made += [gather_case(E, torch.float16, rows, N, T, envs, gen) for E in (3, 8200)]
    made += [gather_case(2 * 8, torch.float32, rows, N, T, envs, gen, once=True),
             gather_case(5000, torch.float32, rows, N, T, envs, gen, once=True)]
    lib().rollout_gather([f for f, _ in made], envs, T)
    torch.cuda.synchronize()
    for _, check in made:
        check()


def test_gather_into_a_column_block_of_a_wider_output():
    """the host's split over more than 64 environments: 70 of 80, as calls of 64 and 6"""
    gen = torch.Generator().manual_seed(11)
    N, T = 80, 2
    envs = torch.randperm(N, generator=gen)[:70].tolist()
    fields = []
    for E, dtype in ((1, torch.int64), (33, torch.float32), (4096, torch.float32), (300, torch.uint8)):
        arena_cpu = values(3 * N * E, dtype, gen).view(3, N, E)
        obuf, oview = guarded(T * 70 * E, dtype)
        fields.append((arena_cpu, arena_cpu.to(DEV), obuf, oview.view(T, 70, E), E))
    for j0 in (0, 64):
        part = envs[j0:j0 + 64]
        lib().rollout_gather([RolloutGatherField(a, o, E, N, 70, j0, False) for _, a, _, o, E in fields],
                             part, T)
    torch.cuda.synchronize()
    for arena_cpu, _, obuf, out, E in fields:
        assert torch.equal(out.cpu(), arena_cpu[:T][:, envs])
        assert (obuf[:GUARD] == SENTINEL[obuf.dtype]).all() and (obuf[-GUARD:] == SENTINEL[obuf.dtype]).all()


def test_gather_refuses_what_it_cannot_index():
    gen = torch.Generator().manual_seed(2)
    field, check = gather_case(7, torch.float32, 3, 4, 2, [0, 1], gen)
    with pytest.raises(RuntimeError, match="environment 4 outside"):
        lib().rollout_gather([field], [0, 4], 2)
    wide, _ = gather_case(7, torch.float32, 3, 4, 2, [0, 1], gen, out_N=80)
    with pytest.raises(RuntimeError, match="65 environments"):
        lib().rollout_gather([wide], [0] * 65, 2)
    torch.cuda.synchronize()
    assert (field.out == SENTINEL[torch.float32]).all() and (wide.out == SENTINEL[torch.float32]).all()


def test_byte_offsets_beyond_4_gib():
    """a sensor arena [2, 2, 2^28 + 4] fp32: the last row starts 3.2 GB in and ends past 2^32.  One
    allocation of each buffer, slices checked."""
    E, edge = 2 ** 28 + 4, 5000
    arena = torch.empty((2, 2, E), dtype=torch.float32, device=DEV)
    src = torch.empty((2, E), dtype=torch.float32, device=DEV)
    gen = torch.Generator().manual_seed(9)
    spans = (slice(0, edge), slice(E // 2 - edge, E // 2 + edge), slice(E - edge, E))
    parts = {}
    for r in range(2):
        arena[0, r, :edge] = -777.0
        arena[0, r, E - edge:] = -777.0
        for s in spans:
            parts[r, s.start] = torch.randn(s.stop - s.start, generator=gen)
            src[r, s] = parts[r, s.start].to(DEV)
    lib().rollout_copy([RolloutCopyField(src, arena[1], E, E, E)], 2)
    torch.cuda.synchronize()
    for r in range(2):
        for s in spans:
            assert torch.equal(arena[1, r, s].cpu(), parts[r, s.start]), (r, s)
        assert (arena[0, r, :edge] == -777.0).all() and (arena[0, r, E - edge:] == -777.0).all()
    # the minibatch of environment 1 over both steps, into the source's memory: [2, 1, E]
    out = src.view(2, 1, E)
    out[:, :, :edge] = 0.0
    out[:, :, E - edge:] = 0.0
    lib().rollout_gather([RolloutGatherField(arena, out, E, 2, 1, 0, False)], [1], 2)
    torch.cuda.synchronize()
    for s in (spans[0], spans[2]):
        assert torch.equal(out[1, 0, s].cpu(), parts[1, s.start]), s
        assert (out[0, 0, s] == -777.0).all(), s


# ------------------------------------------------------------------ vlnce_ppo_advantages
def advantage_inputs(T, N, seed, offset=False):
    gen = torch.Generator().manual_seed(seed)
    if offset:   # a large common offset: mean 1e3, spread 1e-2
        returns = 1e3 + torch.randn(T + 1, N, 1, generator=gen) * 1e-2
        value_preds = torch.randn(T + 1, N, 1, generator=gen) * 1e-2
    else:
        value_preds = torch.randn(T + 1, N, 1, generator=gen)
        returns = value_preds + torch.randn(T + 1, N, 1, generator=gen) * 0.3
    return returns, value_preds


def run_advantages(returns, value_preds, T, N, normalize):
    buf, view = guarded(T * N, torch.float32)
    lib().ppo_advantages(returns.to(DEV), value_preds.to(DEV), view, T, N, normalize, 1e-5)
    torch.cuda.synchronize()
    assert (buf[:GUARD] == -777.0).all() and (buf[GUARD + T * N:] == -777.0).all()
    return view.cpu().view(T, N, 1)


SHAPES = [(1, 2), (3, 4), (16, 8), (128, 64)]


@pytest.mark.parametrize("T,N", SHAPES + [(1, 1)])
def test_advantages_plain_is_torchs_subtraction(T, N):
    returns, value_preds = advantage_inputs(T, N, T * N)
    got = run_advantages(returns, value_preds, T, N, False)
    assert torch.equal(got, returns[:-1] - value_preds[:-1])


@pytest.mark.parametrize("offset", [False, True], ids=["centred", "offset 1e3"])
@pytest.mark.parametrize("T,N", SHAPES)
def test_advantages_normalised_against_fp64(T, N, offset):
    returns, value_preds = advantage_inputs(T, N, T + N, offset)
    got = run_advantages(returns, value_preds, T, N, True)
    d = (returns[:-1] - value_preds[:-1]).double()               # the fp32 differences, widened
    eps = float(np.float32(1e-5))                                # the entry point takes a float
    ref = (d - d.mean()) / (d.std() + eps)                       # unbiased, as torch.std
    # one fp32 rounding of an fp64 result (2^-24 relative), with a factor 2 of slack; the second term
    # covers the cancellation near the mean
    bound = 2.0 ** -23 * ref.abs() + 2.0 ** -40 * ref.abs().max()
    ratio = ((got.double() - ref).abs() / bound).max().item()
    MEASURED.append(f"advantages T={T} N={N} {'offset 1e3' if offset else 'centred'}: {ratio:.3f}")
    print(MEASURED[-1])
    assert ratio <= 1.0
    again = run_advantages(returns, value_preds, T, N, True)
    assert torch.equal(got, again), "two runs differ"


def test_advantages_of_one_value_are_nan():
    returns, value_preds = advantage_inputs(1, 1, 0)
    got = run_advantages(returns, value_preds, 1, 1, True)
    assert torch.isnan(got).all()
    d = returns[:-1] - value_preds[:-1]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (std(): degrees of freedom is <= 0)
        assert torch.isnan((d - d.mean()) / (d.std() + 1e-5)).all()   # as torch does


# ------------------------------------------------------------------ the whole class
def on_device(*a, **kw):
    return ActionDictRolloutStorage(*a, device=DEV, **kw)


@pytest.mark.parametrize("name", ["cont", "disc"])
def test_golden_variant_bit_for_bit(name):
    st = rc.replay(name, DEV, on_device)
    assert all(v.is_cuda for v in st.observations.values()) and st.masks.is_cuda


def test_golden_variant_after_to():
    def moved(*a, **kw):
        st = ActionDictRolloutStorage(*a, **kw)
        assert not st.masks.is_cuda
        st.to(torch.device(DEV))
        return st

    assert rc.replay("cont", DEV, moved).returns.is_cuda


def test_no_call_synchronises():
    g = rc.sub(rc.golden(), "cont")
    steps = [{k: ({kk: vv.to(DEV) for kk, vv in v.items()} if isinstance(v, dict) else v.to(DEV))
              for k, v in g[f"insert{i}"].items()} for i in range(3)]
    next_value = g["next_value0"].to(DEV)
    st = on_device(rc.NUM_STEPS, rc.N, rc.space(), rc.H, num_recurrent_layers=rc.L)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for s in steps:
            st.insert(s["obs"], s["hidden"], s["action"], s["logp"], s["value"], s["reward"], s["mask"])
        st.compute_returns(next_value, True, 0.99, 0.95)
        for normalize in (False, True):
            adv = st.get_advantages(normalize)
        batches = list(st.recurrent_generator(adv, 2))
        st.after_update()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(batches) == 2 and st.step == 0
    with pytest.raises(RuntimeError):   # the mode does catch a synchronising call
        torch.cuda.set_sync_debug_mode("error")
        try:
            st.returns.sum().item()
        finally:
            torch.cuda.set_sync_debug_mode("default")


def build_policy(name):
    case = cases.CASES[name]
    policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                   tp.synth_state_dict)
    return policy.to(DEV)


def test_wddppo_update_end_to_end_against_torch_indexed_minibatches():
    name = "waypoint_ppo_update_64"
    case = cases.CASES[name]
    obs, _, masks, extra, _ = cases.load_case(os.path.join(GOLD, name + ".npz"))
    cfg = PPOConfig(**cases.PPO)
    # policies from the same state, each with a fresh optimizer (deep copies at step 0): one collects
    # the rollout, one runs the update under test, two are the baselines
    collector, *policies = [build_policy(name) for _ in range(4)]
    opts = [Adam([p for p in pol.parameters() if p.requires_grad], lr=2.5e-4, eps=1e-5,
                 max_grad_norm=cfg.max_grad_norm) for pol in policies]
    h0 = extra["h0"][:, :collector.net.num_recurrent_layers].contiguous().to(DEV)
    torch.manual_seed(0)   # policy.act samples
    st = rc.collect_with_policy(collector, {k: v.to(DEV) for k, v in obs.items()}, masks.to(DEV), h0,
                                case["N"], case["T"], DEV, ActionDictRolloutStorage)
    st.check_returns()

    def flat(pol):
        return torch.cat([p.detach().reshape(-1) for p in pol.parameters()]).double().cpu()

    before = flat(policies[1])
    perm = torch.tensor([1, 0])
    with rc.fixed_randperm([perm]):
        got = wddppo_update(policies[0], opts[0], st, cfg, ppo_epoch=1, num_mini_batch=2)
    adv = st.get_advantages(False)
    assert torch.equal(adv, st.returns[:-1] - st.value_preds[:-1])
    base = []
    for pol, opt in zip(policies[1:], opts[1:]):
        total = None
        for sample in rc.torch_minibatches(st, adv, 2, perm):
            stats = torch.stack(wddppo_minibatch_update(pol, opt, sample, cfg))
            total = stats if total is None else total + stats
        base.append(tuple(v / 2 for v in total.tolist()))
    assert all(np.isfinite(got)) and all(np.isfinite(base[0]))

    stats = [torch.tensor(v, dtype=torch.float64) for v in (got, base[0], base[1])]
    params = [flat(pol) for pol in policies]
    assert not torch.equal(params[1], before), "the update moved nothing"
    own_s, own_p = (stats[1] - stats[2]).abs(), (params[1] - params[2]).abs()
    new_s, new_p = (stats[0] - stats[1]).abs(), (params[0] - params[1]).abs()
    MEASURED.append(f"wddppo_update baselines vs each other: statistics max|d| {own_s.max():.3e}, "
                    f"parameters max|d| {own_p.max():.3e} ({int((own_p != 0).sum())} of {own_p.numel()} differ)")
    MEASURED.append(f"wddppo_update storage vs baseline:     statistics max|d| {new_s.max():.3e}, "
                    f"parameters max|d| {new_p.max():.3e} ({int((new_p != 0).sum())} of {new_p.numel()} differ)")
    print("\n".join(MEASURED[-2:]))
    # bit for bit if the baselines agree bit for bit; otherwise within 4x their own difference plus
    # 2^-23 relative, of either.  "Their own difference" is the largest over the tensor: run-to-run
    # differences (the order of atomic adds) land on other elements in every run.
    for own, vals in ((own_s, stats), (own_p, params)):
        for b in (1, 2):
            d = (vals[0] - vals[b]).abs()
            if own.max() == 0:
                assert d.max() == 0, f"{int((d != 0).sum())} values differ from a bit-identical baseline"
            else:
                assert (d <= 4 * own.max() + 2.0 ** -23 * vals[b].abs()).all()
