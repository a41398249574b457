"""GPU tier: vlnce_il_loss and vlnce_pair_mse (csrc/il_loss.hip) on the MI355X against the reference
trainer's formulas (base_il_trainer.py:159-172; aux_losses.py:24-32 over the [B] x [B,1] broadcast
of cma_policy.py:296-307) evaluated by torch IN FP64 ON THE CPU WITH AUTOGRAD, the loss multiplied
by 3 before backward() so that the upstream gradient is exercised.

Tolerances (error relative to the reference tensor's max, the `close` convention of
test_kernels_gpu.py without its absolute slack): 2e-6 for the loss / stats / the pair value, 1e-5
for gradients -- the project's numbers for vlnce_ppo_loss.  torch's own fp32 evaluation of these
formulas on the CPU is within 2e-7 of fp64 at every shape here."""
import functools
import os

import pytest
import torch
import torch.nn.functional as F

import cases
import vlnce_amd
from oracle import thirdparty as tp
from test_oracle_golden import compare
from vlnce_amd import _lib
from vlnce_amd.aux_losses import AuxLossRegistry, PairMSEFn
from vlnce_amd.il_harness import ILLossFn, il_loss, update_agent

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
torch.distributions.Distribution.set_default_validate_args(False)
TOL_VALUE, TOL_GRAD = 2e-6, 1e-5

SHAPES = [(1, 1, 4),      # smallest
          (1, 64, 4),     # the headline batch
          (3, 2, 4),      # the goldens' shape
          (5, 3, 6),      # A != 4, ragged lengths
          (300, 5, 4),    # T above the workgroup size: a thread takes several steps of a column
          (2, 70, 16)]    # N crosses a wave, the largest A


@pytest.fixture(scope="module")
def hip():
    return _lib.get_lib()


def close(got, ref, tol, what):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(ref.abs().max().item(), 1e-30)
    err = (got - ref).abs().max().item()
    print(f"{what}: max|d| = {err:.3e}, reference max = {scale:.3e}, ratio {err / scale:.3e}")
    assert err <= tol * scale, f"{what}: max|d|={err:.3e} scale={scale:.3e}"


@functools.lru_cache(maxsize=None)
def loss_inputs(T, N, A, raw):
    """ragged episode lengths (zero weights past the end, column 0 full length), weights from
    {1, 3.2} with 3.2 at t = 0, logits normalised or raw (x 2)"""
    g = torch.Generator().manual_seed(1000 * T + 10 * N + A + int(raw))
    z = torch.randn(T, N, A, generator=g)
    logits = z * 2 if raw else torch.log_softmax(z, dim=-1)
    targets = torch.randint(0, A, (T, N), generator=g)
    lens = torch.randint(1, T + 1, (N,), generator=g)
    lens[0] = T
    weights = torch.where(torch.rand(T, N, generator=g) < 0.3, 3.2, 1.0)
    weights[0] = 3.2
    weights = weights * (torch.arange(T).view(T, 1) < lens.view(1, N))
    return logits, targets, weights.float()


AUX_VALUE = 0.4321


@functools.lru_cache(maxsize=None)
def loss_reference(T, N, A, raw, with_aux, scalar):
    """fp64, CPU, autograd; computed once per case and shared"""
    logits, targets, weights = loss_inputs(T, N, A, raw)
    z = logits.double().requires_grad_(True)
    w = weights.double()
    ce = F.cross_entropy(z.permute(0, 2, 1), targets, reduction="none")
    action = ((w * ce).sum(0) / w.sum(0)).mean()
    aux = torch.tensor(AUX_VALUE).double().requires_grad_(True)   # the fp32 value, widened
    loss = (action + (aux if with_aux else 0.0)) / scalar
    (loss * 3).backward()
    stats = torch.stack([loss, action, aux if with_aux else torch.zeros((), dtype=torch.float64)])
    return loss.detach(), stats.detach(), z.grad, (aux.grad if with_aux else None)


def run_loss(T, N, A, raw, with_aux, scalar):
    logits, targets, weights = (t.to(DEV) for t in loss_inputs(T, N, A, raw))
    logits = logits.clone().requires_grad_(True)   # (the cached inputs stay as they are)
    aux = torch.tensor(AUX_VALUE, device=DEV, requires_grad=True) if with_aux else 0.0
    loss, stats = il_loss(logits, targets, weights, aux, loss_accumulation_scalar=scalar)
    (loss * 3).backward()
    return loss, stats, logits.grad, (aux.grad if with_aux else None)


@pytest.mark.parametrize("scalar", [1, 4])
@pytest.mark.parametrize("with_aux", [False, True])
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("T,N,A", SHAPES)
def test_il_loss_and_gradients_match_fp64(hip, T, N, A, raw, with_aux, scalar):
    assert hip.il_loss_supported(T, N, A)
    loss, stats, dlogits, daux = run_loss(T, N, A, raw, with_aux, scalar)
    rloss, rstats, rdlogits, rdaux = loss_reference(T, N, A, raw, with_aux, scalar)
    assert not stats.requires_grad
    close(loss, rloss, TOL_VALUE, "loss")
    close(stats, rstats, TOL_VALUE, "stats")
    close(dlogits, rdlogits, TOL_GRAD, "dlogits")
    if with_aux:
        close(daux, rdaux, TOL_GRAD, "daux")
    # a padded row is multiplied by its zero weight: its gradient is exactly zero
    _, _, weights = loss_inputs(T, N, A, raw)
    assert float(dlogits.cpu()[weights == 0].abs().sum()) == 0.0


@pytest.mark.parametrize("T,N,A", SHAPES)
def test_il_loss_is_bit_identical_between_runs(hip, T, N, A):
    a = run_loss(T, N, A, True, True, 4)
    b = run_loss(T, N, A, True, True, 4)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_il_loss_supported_bounds(hip):
    assert hip.il_loss_supported(1, 1024, 16) and hip.il_loss_supported(100000, 1, 1)
    assert not hip.il_loss_supported(1, 1025, 4) and not hip.il_loss_supported(1, 4, 17)
    assert not hip.il_loss_supported(0, 4, 4)


def test_il_loss_widest_supported_batch(hip):
    """N = 1024: every thread walks four whole columns (the N >= 256 route) -- and N = 300, where
    the last pass of that route is partial"""
    for N in (1024, 300):
        T, A = 2, 4
        loss, stats, dlogits, _ = run_loss(T, N, A, True, False, 1)
        rloss, rstats, rdlogits, _ = loss_reference(T, N, A, True, False, 1)
        close(stats, rstats, TOL_VALUE, f"stats N={N}")
        close(dlogits, rdlogits, TOL_GRAD, f"dlogits N={N}")


def test_target_outside_the_row_gives_nan_for_that_row_only(hip):
    T, N, A = 3, 2, 4
    logits, targets, weights = (t.clone() for t in loss_inputs(T, N, A, True))
    weights = torch.ones_like(weights)
    targets[1, 0], targets[2, 1] = A + 3, -1
    stats = torch.empty(3, device=DEV)
    dlogits = torch.empty(T * N, A, device=DEV)
    hip.il_loss(logits.to(DEV), targets.to(DEV), weights.to(DEV), None, 1.0, T, N, A, stats, dlogits)
    d = dlogits.cpu().view(T, N, A)
    bad = torch.zeros(T, N, dtype=torch.bool)
    bad[1, 0] = bad[2, 1] = True
    assert bool(torch.isnan(d[bad]).all()) and bool(torch.isfinite(d[~bad]).all())
    assert bool(torch.isnan(stats.cpu()[:2]).all())
    # the rows that are in range keep their gradient: (softmax - onehot) * w / sum_t w / N
    z = logits.double()
    want = (torch.softmax(z, -1) - F.one_hot(targets.clamp(0, A - 1), A)) / T / N
    close(d[~bad], want[~bad], TOL_GRAD, "dlogits of the rows in range")


# ---------------------------------------------------------------------------- the pair term
PAIRS = [(1, 1), (6, 6), (500, 500), (21, 42)]


@functools.lru_cache(maxsize=None)
def pair_inputs(E, R, full_mask, near):
    g = torch.Generator().manual_seed(7 * E + R + int(near))
    target = torch.rand(R, 1, generator=g)
    if near:   # estimates sitting on the targets: the cancelling case of the closed form
        base = target.view(-1)[torch.arange(E) % R]
        estimate = torch.tanh(base + 0.01 * torch.randn(E, generator=g))
    else:
        estimate = torch.tanh(torch.randn(E, generator=g))
    mask = torch.ones(E, dtype=torch.bool) if full_mask else torch.rand(E, generator=g) < 0.6
    mask[0] = True
    return estimate, target, mask


@functools.lru_cache(maxsize=None)
def pair_reference(E, R, full_mask, near):
    estimate, target, mask = pair_inputs(E, R, full_mask, near)
    e = estimate.double().requires_grad_(True)
    e2, t2 = torch.broadcast_tensors(e, target.double())     # register_progress_loss
    value = ((e2 - t2) ** 2).masked_select(mask).mean()       # AuxLossRegistry.reduce
    (value * 3).backward()
    return value.detach(), e.grad


def run_pair(E, R, full_mask, near):
    estimate, target, mask = (t.to(DEV) for t in pair_inputs(E, R, full_mask, near))
    estimate = estimate.clone().requires_grad_(True)
    value = PairMSEFn.apply(estimate, target, mask)
    (value * 3).backward()
    return value, estimate.grad


@pytest.mark.parametrize("near", [False, True])
@pytest.mark.parametrize("full_mask", [True, False])
@pytest.mark.parametrize("E,R", PAIRS)
def test_pair_mse_and_gradient_match_fp64(hip, E, R, full_mask, near):
    value, grad = run_pair(E, R, full_mask, near)
    rvalue, rgrad = pair_reference(E, R, full_mask, near)
    close(value, rvalue, TOL_VALUE, "value")
    close(grad, rgrad, TOL_GRAD, "d_estimate")
    _, _, mask = pair_inputs(E, R, full_mask, near)
    assert float(grad.cpu()[~mask].abs().sum()) == 0.0
    again = run_pair(E, R, full_mask, near)
    assert torch.equal(again[0], value) and torch.equal(again[1], grad)


def test_pair_term_never_builds_the_matrix(hip):
    """E = R = 2 500: the materialised path holds several 6.25 M-element tensors, the fused one
    nothing of that size -- and both give the fp64 value"""
    E = R = 2500
    estimate, target, mask = (t.to(DEV) for t in pair_inputs(E, R, False, True))
    matrix_bytes = E * R * 4

    def peak(fused):
        e = estimate.clone().requires_grad_(True)
        reg = AuxLossRegistry()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with reg.active():
            if fused:
                with reg.fused():
                    reg.register_pair_loss("pm", e, target, 0.5)
                    value = reg.reduce(mask)
            else:
                reg.register_pair_loss("pm", e, target, 0.5)
                value = reg.reduce(mask)
        (value * 3).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, value.detach(), e.grad

    fused_peak, fused_value, fused_grad = peak(True)
    plain_peak, plain_value, plain_grad = peak(False)
    print(f"peak bytes above the inputs: fused {fused_peak}, materialised {plain_peak}, "
          f"one [R, E] fp32 matrix {matrix_bytes}")
    assert fused_peak < matrix_bytes <= plain_peak
    rvalue, rgrad = pair_reference(E, R, False, True)
    close(fused_value, 0.5 * rvalue, TOL_VALUE, "value at 2500")
    close(fused_grad, 0.5 * rgrad, TOL_GRAD, "d_estimate at 2500")
    print(f"materialised fp32 value {float(plain_value):.9g}, fp64 reference {0.5 * float(rvalue):.9g}")


# ---------------------------------------------------------------------------- end to end
def to_dev(x):
    if isinstance(x, dict):
        return {k: to_dev(v) for k, v in x.items()}
    return x.to(DEV) if isinstance(x, torch.Tensor) else x


@pytest.mark.parametrize("name", ["cma_update_64", "seq2seq_update_64"])
def test_fused_update_matches_reference_golden(hip, name):
    """the progress-monitor goldens of the real reference classes through fused_loss=True: the
    loss triple and every gradient `compare` covers, at the existing 1e-4 / 1e-4"""
    calls = []

    def fused_update(policy, obs, prev, masks, targets, weights):
        hs = policy.net.model_config.STATE_ENCODER.hidden_size
        inner = {n: getattr(hip, n) for n in ("il_loss", "pair_mse")}
        for n, f in inner.items():
            setattr(hip, n, lambda *a, _n=n, _f=f: (calls.append(_n), _f(*a))[1])
        try:
            return update_agent(policy, None, obs, prev, masks, targets, weights, hs,
                                step_grad=False, fused_loss=True)
        finally:
            for n in inner:
                delattr(hip, n)

    case = cases.CASES[name]
    obs, prev, masks, extra, gold = cases.load_case(os.path.join(GOLD, name + ".npz"))
    policy, _ = cases.build_policy(vlnce_amd, case, vlnce_amd.make_config, vlnce_amd.make_spaces,
                                   tp.synth_state_dict)
    policy.to(DEV)
    outs = cases.run_case(policy, case, to_dev(obs), to_dev(prev), to_dev(masks), to_dev(extra),
                          fused_update, vlnce_amd.AuxLosses)
    compare(outs, gold, atol=1e-4, rtol=1e-4)
    assert sorted(calls) == ["il_loss", "pair_mse"]


def test_function_signature_matches_ppo_loss_shape(hip):
    """ILLossFn.apply(logits, targets, weights, aux | None, inv_scalar) -> (loss [], stats [3])"""
    logits, targets, weights = (t.to(DEV) for t in loss_inputs(3, 2, 4, False))
    loss, stats = ILLossFn.apply(logits, targets, weights, None, 0.25)
    assert loss.shape == () and stats.shape == (3,) and float(stats[2]) == 0.0
    assert float(loss) == pytest.approx(float(stats[1]) * 0.25, rel=1e-6)
