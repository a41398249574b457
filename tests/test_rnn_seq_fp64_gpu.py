"""The packed-sequence RNN kernels of csrc/rnn_seq.hip -- rnn_seq_{fwd,bwd}_kernel<KIND, H, NW> in all
eight instances, dseq_to_time_major_kernel, zero_tails -- and its five entry points
vlnce_rnn_seq_fwd, _bwd, _fwd2, _bwd2, _wgrad, called directly through _lib.get_lib() and held END
TO END to the fp64 reference of tests/rnn_seq_ref.py: forward outputs and saved state as produced,
dgi / dgh / dW / db / dx against the reference's autograd gradients of the same dseq / dh_final.

Every buffer a call may write is NaN before the call and sits between NaN guards
(test_rnn_seq_ref_host.drive): what must be zero past a row's length (out_tm, seq, dgi, dgh) must
be exactly 0.0 afterwards, what is compared must be finite, the guards must still be NaN.

Bound per tensor X:  err(X) = max|X - X64| / max(max|X64|, 1e-30)  <=  K * max(E32(X), 2^-23),
E32(X) the same measure of tests/hostsim.py's fp32 result on the same inputs, K = 8: the gate
non-linearities run on the hardware exp2 / rcp, documented at < 3e-7 absolute against ~6e-8 for
fp32 libm -- a factor of five, rounded up to a power of two; the six-plane bf16 product is as
precise as fp32.  Every figure is printed (pytest -s).  Lengths stay within the contract
0 <= len <= L: a longer one is never run (the reverse walk would index before its buffers).

Largest err / max(E32, 2^-23) per tensor kind measured on an MI355X over the whole file (bound: 8):
    out_tm 4.87  seq 4.87  h_final 5.99  gates 5.27  aux 4.89  dgi 2.58  dgh 1.83
    dw_ih 2.10  db_ih 1.49  dw_hh 3.10  db_hh 1.49  dx 1.78
(largest: h_final of LSTM-H128-NW8 d2 B1 L9, err 7.1e-7 against E32 1.1e-7; the per-step slices of
the precision cases reach 2.58).  Scratch mutants of rnn_seq.hip, one run each: skipping plane
product q = 0, 1 or 2 of X3_PA / X3_PB in both MFMA loops fails all four precision cases in every
slice, forward (gates, aux, out_tm: ratios 14-37) and backward (dgi, dgh: 14-28), and 71-74 more
tests; self_zero forced to 0 in vlnce_rnn_seq_fwd2 fails 86 tests on "out_tm[0] tail not zero".
"""
import collections

import pytest
import torch

from test_rnn_seq_ref_host import (compared, drive, err, gpu_cases, pairs, reference, simulated)
from vlnce_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 8
FLOOR = 2.0 ** -23
WORST = collections.defaultdict(float)   # tensor kind -> largest ratio seen in this session


@pytest.fixture(scope="module")
def hip():
    lib = _lib.get_lib()
    yield lib
    print("\nlargest err / max(E32, 2^-23) per tensor kind: "
          + ", ".join(f"{k} {v:.2f}" for k, v in sorted(WORST.items())))


def judge(case, label, kind, g, want, s, failures):
    """one tensor against the reference under the K * max(E32, 2^-23) bound; prints its figures"""
    e, e32 = err(g, want), err(s, want)
    ratio = e / max(e32, FLOOR)
    bound = K * max(e32, FLOOR)
    print(f"{case.id} {label}: err={e:.3e} E32={e32:.3e} ratio={ratio:.2f} bound={bound:.3e}")
    WORST[kind] = max(WORST[kind], ratio)
    if not e <= bound:
        failures.append(f"{label}: err={e:.3e} E32={e32:.3e} ratio={ratio:.2f} > K={K}")


def held(case, got, names, failures, what="", **opts):
    """compare `names` of a drive() result with the fp64 reference; E32 from the simulator's result
    of the same call sequence"""
    ref = reference(case, opts.get("grad", "both"))
    sim = simulated(case, **opts)
    for (label, kind, g, want), (_, _, s, _) in zip(pairs(got, ref, names), pairs(sim, ref, names)):
        judge(case, what + label, kind, g, want, s, failures)


def same_bits(a, b, names, what):
    for (label, _, x, y) in pairs(a, b, names):
        assert torch.equal(x, y), f"{what}: {label} is not bit-identical"


def saved_names(case):
    return ["dgi"] + (["dgh"] if case.kind == 1 else [])


# dx is NOT in any bit-for-bit comparison: its GEMM (rows x E outputs, a reduction over G*H) splits
# the reduction over workgroups that add their parts with atomics, in whatever order they finish,
# so two launches of the same call differ in the last bits.  Each dx is held to fp64 instead.  The
# parameter gradients of the `variant` cases reduce over L*B = 153 rows, below the split threshold.
PARAM_GRADS = ["dw_ih", "db_ih", "dw_hh", "db_hh"]


# ------------------------------------------------------------------ the whole chain, every instance
@pytest.mark.parametrize("case", gpu_cases("chain"), ids=lambda c: c.id)
def test_rnn_seq_fwd2_bwd2_wgrad_vs_fp64(hip, case):
    """vlnce_rnn_seq_fwd2 (saving, seq) -> _bwd2 (dseq through dseq_to_time_major_kernel, dh_final)
    -> _wgrad (all directions, dx) on poisoned buffers (zero_tails writes the tails)."""
    got = drive(hip, DEV, case)
    failures = []
    held(case, got, compared(case), failures)
    assert not failures, "\n".join([case.id] + failures)


@pytest.mark.parametrize("case", gpu_cases("precision"), ids=lambda c: c.id)
def test_rnn_seq_plane_products_vs_fp64(hip, case):
    """One recurrent product per direction and pass, seen before saturation: the GRU's aux IS
    W_hn h + b_hn, the LSTM's gates of the second step sit on the steep part of their
    non-linearities, and the first step's dgi is what came back through dgates W_hh.  Compared per
    step, so that the step without a product does not set the scale.  A plane product of order
    2^-16 that goes missing moves these by ~1e-5; the bound is ~1e-6."""
    opts = dict(wgrad=None)
    got = drive(hip, DEV, case, **opts)
    ref, sim = reference(case), simulated(case, **opts)
    failures = []
    held(case, got, compared(case), failures, **opts)
    for d in range(case.dirs):
        first, second = (0, 1) if d == 0 else (1, 0)   # time index of the step processed first / second
        slices = [("gates", second), ("aux", second), ("out_tm", second), ("dgi", first)]
        if case.kind == 1:
            slices.append(("dgh", first))
        for name, t in slices:
            judge(case, f"{name}[{d}][t={t}]", name, got[name][d][t], ref[name][d][t], sim[name][d][t], failures)
    assert not failures, "\n".join([case.id] + failures)


# ------------------------------------------------------------------ forward arms
@pytest.mark.parametrize("case", gpu_cases("variant"), ids=lambda c: c.id)
def test_rnn_seq_fwd2_null_gates_is_bit_identical(hip, case):
    """gates_save / aux_save null is the inference path: out_tm, seq, h_final as in the saving call"""
    saving = drive(hip, DEV, case, grad=None)
    infer = drive(hip, DEV, case, grad=None, save=False)
    same_bits(infer, saving, ["out_tm", "seq", "h_final"], case.id)


@pytest.mark.parametrize("case", gpu_cases("variant"), ids=lambda c: c.id)
def test_rnn_seq_fwd2_strided_seq_and_null_seq(hip, case):
    """seq as a [:, :L, :dirs*H] slice of a [B, L+3, dirs*H+8] buffer (nothing outside the slice is
    written: checked in drive), and seq null: the other outputs do not change"""
    contig = drive(hip, DEV, case, grad=None)
    strided = drive(hip, DEV, case, grad=None, seq_mode="strided")
    none = drive(hip, DEV, case, grad=None, seq_mode="none")
    same_bits(strided, contig, ["out_tm", "seq", "h_final", "gates", "aux"], case.id + " strided seq")
    same_bits(none, contig, ["out_tm", "h_final", "gates", "aux"], case.id + " null seq")
    assert "seq" not in none
    failures = []
    held(case, strided, ["seq", "out_tm", "h_final"], failures, what="strided ", grad=None, seq_mode="strided")
    assert not failures, "\n".join([case.id] + failures)


# ------------------------------------------------------------------ backward arms
@pytest.mark.parametrize("grad", ["dseq", "dhf", "both", "dhf0", "dhf1"],
                         ids=["dseq_only", "dh_final_only", "both", "dh_final_t_None", "dh_final_None_t"])
@pytest.mark.parametrize("case", gpu_cases("variant"), ids=lambda c: c.id)
def test_rnn_seq_bwd2_gradient_arms_vs_fp64(hip, case, grad):
    """dseq only, dh_final only, both, and dh_final with one direction None (what
    set_materialize_grads(False) hands over), each through _wgrad as well"""
    got = drive(hip, DEV, case, grad=grad)
    failures = []
    held(case, got, compared(case), failures, what=f"{grad} ", grad=grad)
    assert not failures, "\n".join([case.id] + failures)


@pytest.mark.parametrize("case", gpu_cases("variant"), ids=lambda c: c.id)
def test_rnn_seq_bwd2_dseq_to_time_major_unaligned_slice(hip, case):
    """dseq as a slice of a longer padded buffer whose data pointer is 4 bytes off a 16-byte
    boundary: dseq_to_time_major_kernel reads it with scalar loads"""
    plain = drive(hip, DEV, case, wgrad=None)
    got = drive(hip, DEV, case, wgrad=None, dseq_mode="unaligned")
    same_bits(got, plain, saved_names(case), case.id)
    failures = []
    held(case, got, saved_names(case), failures, what="unaligned ", wgrad=None, dseq_mode="unaligned")
    assert not failures, "\n".join([case.id] + failures)


@pytest.mark.parametrize("case", gpu_cases("variant"), ids=lambda c: c.id)
def test_rnn_seq_bwd2_ignores_saved_state_past_the_lengths(hip, case):
    """gates / aux past a length are unspecified (here: still NaN from the poisoning); zeroing them
    before the backward changes nothing downstream"""
    nan_tails = drive(hip, DEV, case)
    clean = drive(hip, DEV, case, clean_saved=True)
    same_bits(nan_tails, clean, saved_names(case) + PARAM_GRADS, case.id)
    failures = []
    held(case, nan_tails, ["dx"], failures, what="NaN tails ")
    assert not failures, "\n".join([case.id] + failures)


# ------------------------------------------------------------------ wgrad arms
@pytest.mark.parametrize("case", gpu_cases("variant"), ids=lambda c: c.id)
def test_rnn_seq_wgrad_first_dir_two_calls(hip, case):
    """dirs = 2 in one call against two calls of dirs = 1 with first_dir 0 and 1 (what ops.RNNLayerFn
    issues on two streams): the same parameter gradients bit for bit, dx the sum of the two"""
    one = drive(hip, DEV, case)
    two = drive(hip, DEV, case, wgrad="two")
    same_bits(two, one, PARAM_GRADS, case.id)
    failures = []
    two["dx"] = two["dx_parts"][0] + two["dx_parts"][1]
    held(case, two, ["dx"], failures, what="sum of two calls ")
    held(case, one, ["dx"], failures, what="one call ")
    assert not failures, "\n".join([case.id] + failures)


@pytest.mark.parametrize("case", [c for c in gpu_cases("variant") if c.kind == 0], ids=lambda c: c.id)
def test_rnn_seq_wgrad_db_ih_aliasing_db_hh(hip, case):
    """LSTM: dGh = dgi, so the caller may pass one buffer for both bias gradients"""
    plain = drive(hip, DEV, case)
    alias = drive(hip, DEV, case, alias_db=True)
    same_bits(alias, plain, PARAM_GRADS, case.id)
    failures = []
    held(case, alias, PARAM_GRADS + ["dx"], failures, what="aliased ")
    assert not failures, "\n".join([case.id] + failures)


@pytest.mark.parametrize("case", gpu_cases("variant"), ids=lambda c: c.id)
def test_rnn_seq_wgrad_ldx_and_null_dx(hip, case):
    """x_tm rows with a pitch ldx > E (the columns past E are random, not zeros), and dx_tm null"""
    plain = drive(hip, DEV, case)
    wide = drive(hip, DEV, case, ldx_pad=3)
    nodx = drive(hip, DEV, case, want_dx=False)
    same_bits(wide, plain, PARAM_GRADS, case.id + " ldx")
    same_bits(nodx, plain, PARAM_GRADS, case.id + " null dx")
    assert "dx" not in nodx
    failures = []
    held(case, wide, ["dw_ih", "dx"], failures, what="ldx>E ", ldx_pad=3)
    assert not failures, "\n".join([case.id] + failures)


@pytest.mark.parametrize("case", gpu_cases("l1"), ids=lambda c: c.id)
def test_rnn_seq_wgrad_L1_dw_hh_is_zero(hip, case):
    """L = 1: no previous state anywhere, dW_hh is exactly zero (vlnce_zero, not a GEMM), and the
    prefetches fetch(s + 1) / fetch_prev(Lt - 2) reach past both ends"""
    got = drive(hip, DEV, case)
    for d in range(case.dirs):
        assert bool((got["dw_hh"][d] == 0).all()), f"{case.id}: dw_hh[{d}] not exactly zero"
    failures = []
    held(case, got, compared(case), failures)
    assert not failures, "\n".join([case.id] + failures)


# ------------------------------------------------------------------ first generation
@pytest.mark.parametrize("case", gpu_cases("variant"), ids=lambda c: c.id)
def test_rnn_seq_fwd_bwd_first_generation_is_bit_identical(hip, case):
    """vlnce_rnn_seq_fwd / _bwd (pre-zeroed buffers, transposed weights, time-major dout) launch the
    same kernels as _fwd2 / _bwd2: the same bits in out, h_final, gates, aux, dgi, dgh.  The test a
    unification of the two generations keeps passing until it deletes the old pair."""
    new = drive(hip, DEV, case, wgrad=None)
    old = drive(hip, DEV, case, wgrad=None, generation=1)
    same_bits(old, new, ["out_tm", "h_final", "gates", "aux"] + saved_names(case), case.id)
    failures = []
    held(case, old, ["out_tm", "h_final", "gates", "aux"] + saved_names(case), failures,
         what="first generation ", wgrad=None, generation=1)
    assert not failures, "\n".join([case.id] + failures)
