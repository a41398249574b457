"""The attention family of csrc/attn.hip -- attn_fwd_kernel, attn_bwd_kernel, segment_sum_kernel,
rowzero_mask_kernel behind vlnce_attn_fwd, _fwd_shared, _bwd, _bwd_shared, vlnce_segment_sum and
vlnce_rowzero_mask -- called directly through _lib.get_lib() and held to the fp64 reference of
tests/attention_ref.py on every code path: the case table there states which of the vector / scalar
paths each case takes (checked against the pointers actually passed, test_attention_ref_host.drive).

Every buffer a call may write is NaN before the call and sits between NaN guards (the padding
columns of padded rows are guards too): what must be written is finite afterwards, the guards are
still NaN, a mode-2 fully masked row has dq = dK = 0 and an unattended block sums to zeros exactly,
a mode-1 fully masked row attends uniformly (the fp32 absorption of the logits into -1e8).

Bound per tensor X:  err(X) = max|X - X64| / max(max|X64|, 1e-30)  <=  K * max(E32(X), 2^-23),
E32(X) the same measure of tests/hostsim.py's fp32 result on the same inputs, K = 8 as in
tests/test_rnn_seq_fp64_gpu.py.  There it covers the hardware exp2 / rcp; these kernels call
library expf and differ from the simulator in summation order only, so 8 is an upper limit, not a
target.  The backward runs twice: from the forward's own attention (the product's chain) and from
the fp64 attention rounded to fp32 (the backward kernel alone).  Every figure is printed
(pytest -s).

Largest err / max(E32, 2^-23) per tensor kind measured on an MI355X over the whole file (bound: 8):
    (to be measured)
"""
import collections
import functools

import pytest
import torch

import attention_ref as ar
from test_attention_ref_host import (CASES, SIM, Buffers, drive, drive_segment_sum, err, exact_expectations, ids,
                                     names, reference, segment_inputs, simulated, uniform_rows_error)
from vlnce_amd import _lib, ops

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


def judge(cid, label, kind, g, want, s, failures):
    """one tensor against the reference under the K * max(E32, 2^-23) bound; prints its figures"""
    e, e32 = err(g, want), err(s, want)
    ratio = e / max(e32, FLOOR)
    bound = K * max(e32, FLOOR)
    print(f"{cid} {label}: err={e:.3e} E32={e32:.3e} ratio={ratio:.2f} bound={bound:.3e}")
    WORST[kind] = max(WORST[kind], ratio)
    if not e <= bound:
        failures.append(f"{label}: err={e:.3e} E32={e32:.3e} ratio={ratio:.2f} > K={K}")


def held(case, got, src, failures, what=""):
    """a drive() result against the fp64 reference; E32 from the simulator's run of the same calls"""
    ref, sim = reference(case, src), simulated(case, src)
    exact_expectations(case, got)
    for name in names(case):
        judge(case.id, what + name, name, got[name], ref[name], sim[name], failures)
    u, u32 = uniform_rows_error(case, got), uniform_rows_error(case, sim)
    if ar.full_rows(case) and "attn" in got:
        print(f"{case.id} {what}fully masked rows: |attn P - 1| = {u:.3e} (simulator {u32:.3e})")
        if not u <= K * max(u32, FLOOR):
            failures.append(f"fully masked rows are not uniform: |attn P - 1| = {u:.3e}")


@functools.lru_cache(maxsize=None)
def on_gpu(case, src="own"):
    """the library's first run of a case (cached: shared between the tests, never modified)"""
    return drive(_lib.get_lib(), case, DEV, attn_src=src)


# ------------------------------------------------------------------ the kernels, every path
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_attention_fwd_bwd_chain_vs_fp64(hip, case):
    """forward, backward from the forward's own attention, the segment sums of the shared form"""
    failures = []
    held(case, on_gpu(case), "own", failures)
    assert not failures, "\n".join([case.id] + failures)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_attention_bwd_alone_vs_fp64(hip, case):
    """backward from the fp64 attention rounded to fp32: no forward error to hide behind"""
    failures = []
    held(case, on_gpu(case, "given"), "given", failures, what="given attn: ")
    assert not failures, "\n".join([case.id] + failures)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_attention_two_calls_are_bit_identical(hip, case):
    """no atomics anywhere in csrc/attn.hip: the same inputs give the same bits"""
    first, again = on_gpu(case), drive(hip, case, DEV)
    for name in names(case):
        assert torch.equal(first[name], again[name]), f"{case.id}: {name} differs between two calls"


@pytest.mark.parametrize("row_elems", ar.SEG_ROW_ELEMS)
def test_segment_sum_alone(hip, row_elems):
    """one strip, the last full strip, strip + 1 float4, four strips + 1: blocks 1, 2 and 4 of the
    NaN-filled output have no row and must come back as zeros"""
    x, index = segment_inputs(row_elems)
    got, again = drive_segment_sum(hip, row_elems, DEV), drive_segment_sum(hip, row_elems, DEV)
    assert torch.equal(got, again)
    assert bool((got[[1, 2, 4]] == 0).all()), "an unattended block is not zero"
    failures = []
    judge(f"segment_sum-{row_elems}", "out", "segment_sum", got, ar.segment_sum(x, index, 5, 5, row_elems),
          drive_segment_sum(SIM, row_elems), failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------ rowzero_mask
ROW_PATTERNS = ("zeros", "random", "negative zeros", "one NaN", "one inf", "one denormal", "last column")


def _rowzero_input(rows, C, ld):
    g = ar._gen("rowzero", rows, C, ld)
    x = torch.randn(rows, ld, generator=g) + 3.0        # junk in the padding is never zero
    kinds = [(r + C) % len(ROW_PATTERNS) for r in range(rows)]
    for r, k in enumerate(kinds):
        if k == 1:
            continue
        x[r, :C] = -0.0 if k == 2 else 0.0
        col = int(torch.randint(0, C, (1,), generator=g))
        if k == 3:
            x[r, col] = float("nan")
        elif k == 4:
            x[r, col] = float("inf")
        elif k == 5:
            x[r, col] = 1e-40
        elif k == 6:
            x[r, C - 1] = -2.5
    return x, kinds


@pytest.mark.parametrize("pad", [0, 3], ids=["ld=C", "ld=C+3"])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 121])
def test_rowzero_mask_edges(hip, rows, C, pad):
    """rows around the four-row workgroup, columns around the 64-lane stride, a row pitch beyond C
    with non-zero junk, and the rows a comparison can get wrong: -0.0 is zero; NaN, inf, a 1e-40
    denormal and a lone last column are not"""
    x, kinds = _rowzero_input(rows, C, C + pad)
    if rows == 121:
        assert set(kinds) == set(range(len(ROW_PATTERNS)))
    if 5 in kinds:
        assert float(x[kinds.index(5), :C].abs().max()) > 0, "the denormal did not survive on the host"
    want = (x[:, :C] == 0).all(-1)
    guard = 64
    flat = torch.full((rows + 2 * guard,), 0xAB, dtype=torch.uint8, device=DEV)
    hip.rowzero_mask(x.to(DEV), C + pad, rows, C, flat[guard:guard + rows])
    got = flat.cpu()
    assert bool((got[:guard] == 0xAB).all()) and bool((got[guard + rows:] == 0xAB).all()), "wrote outside the mask"
    wrong = [(r, ROW_PATTERNS[kinds[r]]) for r in range(rows) if bool(got[guard + r]) != bool(want[r])]
    assert torch.equal(got[guard:guard + rows], want.to(torch.uint8)), f"rows {wrong}"


# ------------------------------------------------------------------ the autograd layer
def _case(group, **kw):
    hits = [c for c in CASES if c.group == group and all(getattr(c, k) == v for k, v in kw.items())]
    assert len(hits) == 1, (group, kw, [c.id for c in hits])
    return hits[0]


KV_CASES = [c for c in CASES if c.layout == "kv"]
OPS_CASES = ([_case("Dk", Dk=260), _case("mixed", Dk=6), _case("P", P=257, mode=1)]
             + [c for c in CASES if c.U is not None and not c.nulls])


def _ops_inputs(case):
    inp = ar.make_inputs(case)
    q = inp["q"].to(DEV).requires_grad_()
    mask = None if inp["mask"] is None else inp["mask"].to(DEV)
    index = None if inp["index"] is None else inp["index"].to(DEV)
    return q, mask, index, inp


def _judge_ops(case, got, failures, what):
    ref, sim = reference(case), simulated(case)
    for name, t in got.items():
        judge(case.id, what + name, name, t.detach().cpu(), ref[name], sim[name], failures)


@pytest.mark.parametrize("case", OPS_CASES, ids=ids)
def test_ops_attention_vs_fp64(hip, case):
    """ops.attention on contiguous K / V, and with `index` (the gradients of K and V summed per block)"""
    q, mask, index, inp = _ops_inputs(case)
    Kd, Vd = inp["K"].to(DEV).requires_grad_(), inp["V"].to(DEV).requires_grad_()
    out = ops.attention(q, Kd, Vd, mask, case.mode, case.scale, index=index)
    (out * inp["dout"].to(DEV)).sum().backward()
    sfx = "u" if index is not None else ""
    failures = []
    _judge_ops(case, {"out": out, "dq": q.grad, "dK" + sfx: Kd.grad, "dV" + sfx: Vd.grad}, failures, "ops.attention ")
    assert not failures, "\n".join([case.id] + failures)


@pytest.mark.parametrize("case", KV_CASES, ids=ids)
def test_ops_attention_strided_views_vs_fp64(hip, case):
    """ops.attention on K and V as the two column ranges of one tensor (read in place through ldk / ldv)"""
    q, mask, index, inp = _ops_inputs(case)
    kv = torch.cat([inp["K"], inp["V"]], 2).to(DEV).requires_grad_()
    out = ops.attention(q, kv[..., :case.Dk], kv[..., case.Dk:], mask, case.mode, case.scale)
    (out * inp["dout"].to(DEV)).sum().backward()
    failures = []
    _judge_ops(case, {"out": out, "dq": q.grad, "dK": kv.grad[..., :case.Dk], "dV": kv.grad[..., case.Dk:]},
               failures, "ops.attention views ")
    assert not failures, "\n".join([case.id] + failures)


@pytest.mark.parametrize("case", KV_CASES, ids=ids)
def test_ops_attention_kv_vs_fp64(hip, case):
    """ops.attention_kv: dK and dV land in the two column ranges of ONE torch.empty d kv
    (lddk = lddv = Dk + Dv); every element of it is compared"""
    q, mask, index, inp = _ops_inputs(case)
    kv = torch.cat([inp["K"], inp["V"]], 2).to(DEV).requires_grad_()
    out = ops.attention_kv(q, kv, case.Dk, mask, case.mode, case.scale)
    (out * inp["dout"].to(DEV)).sum().backward()
    assert kv.grad.shape == kv.shape and bool(torch.isfinite(kv.grad).all())
    failures = []
    _judge_ops(case, {"out": out, "dq": q.grad, "dK": kv.grad[..., :case.Dk], "dV": kv.grad[..., case.Dk:]},
               failures, "ops.attention_kv ")
    assert not failures, "\n".join([case.id] + failures)


@pytest.mark.parametrize("kv_form", [False, True], ids=["attention", "attention_kv"])
def test_ops_attention_mask_forms(hip, kv_form):
    """a bool mask and a column slice of a wider uint8 mask give the bits of the contiguous uint8
    mask (and so the reference's result); a float mask or a mask of another shape is refused"""
    case = _case("layout", layout="kv", Dk=128, mode=1)
    inp = ar.make_inputs(case)
    q, dout, m = inp["q"].to(DEV), inp["dout"].to(DEV), inp["mask"].to(DEV)
    kv0 = torch.cat([inp["K"], inp["V"]], 2).to(DEV)

    def run(mask):
        kv = kv0.clone().requires_grad_()
        qd = q.clone().requires_grad_()
        if kv_form:
            out = ops.attention_kv(qd, kv, case.Dk, mask, 1, case.scale)
        else:
            out = ops.attention(qd, kv[..., :case.Dk], kv[..., case.Dk:], mask, 1, case.scale)
        (out * dout).sum().backward()
        return out.detach(), qd.grad, kv.grad

    base = run(m)
    failures = []
    _judge_ops(case, {"out": base[0], "dq": base[1], "dK": base[2][..., :case.Dk], "dV": base[2][..., case.Dk:]},
               failures, "uint8 mask ")
    assert not failures, "\n".join(failures)
    wide = torch.ones(case.B, case.P + 5, dtype=torch.uint8, device=DEV)
    wide[:, 2:2 + case.P] = m
    sliced = wide[:, 2:2 + case.P]
    assert not sliced.is_contiguous()
    for what, mask in (("bool", m.bool()), ("column slice", sliced), ("bool column slice", sliced.bool())):
        for a, b in zip(base, run(mask)):
            assert torch.equal(a, b), f"{what} mask changes the result"
    for bad, exc in ((m.float(), TypeError), (m.to(torch.int64), TypeError), (m[:, :-1], ValueError),
                     (m.view(-1), ValueError), (m[:-1], ValueError)):
        with pytest.raises(exc):
            run(bad)


# ------------------------------------------------------------------ arguments refused before any launch
BAD_ARGS = [dict(P=ar.MAXP + 1), dict(P=0), dict(B=0), dict(mask_mode=3), dict(Dk=0), dict(Dv=0)]


@pytest.mark.parametrize("shared", [False, True], ids=["plain", "shared"])
@pytest.mark.parametrize("bad", BAD_ARGS + [dict(lddk=7), dict(lddv=7)], ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_attention_refuses_bad_arguments_and_writes_nothing(hip, bad, shared):
    """each entry point returns the library's error and leaves its (NaN) outputs alone.  Only what is
    refused BEFORE a launch is tried here: nothing launches with bad sizes."""
    B, P, Dk, Dv = 2, 7, 8, 8
    t = lambda *s: torch.ones(*s, device=DEV)   # noqa: E731
    q, Kt, Vt, dout, a = t(B, Dk), t(B, P, Dk), t(B, P, Dv), t(B, Dv), t(B, P) / P
    mask = torch.zeros(B, P, dtype=torch.uint8, device=DEV)
    index = torch.arange(B, device=DEV) if shared else None
    buf = Buffers(DEV)
    out, attn, dq, dK, dV = buf.new(B, Dv), buf.new(B, P), buf.new(B, Dk), buf.new(B, P, Dk), buf.new(B, P, Dv)
    sc = dict(B=B, P=P, Dk=Dk, Dv=Dv, mask_mode=1, lddk=Dk, lddv=Dv)
    sc.update(bad)
    refused = "bad shape|bad mask_mode|row pitch below"
    entry = "_shared failed" if shared else " failed"
    if "lddk" not in bad and "lddv" not in bad:
        with pytest.raises(RuntimeError, match=f"vlnce_attn_fwd{entry}.*({refused})"):
            hip.attn_fwd(q, Kt, Dk, Vt, Dv, mask, sc["mask_mode"], 0.5, out, attn, sc["B"], sc["P"], sc["Dk"], sc["Dv"],
                         kv_index=index)
    with pytest.raises(RuntimeError, match=f"vlnce_attn_bwd{entry}.*({refused})"):
        hip.attn_bwd(dout, q, Kt, Dk, Vt, Dv, mask, sc["mask_mode"], 0.5, a, dq, dK, sc["lddk"], dV, sc["lddv"],
                     sc["B"], sc["P"], sc["Dk"], sc["Dv"], kv_index=index)
    torch.cuda.synchronize()
    for what, x in (("out", out), ("attn", attn), ("dq", dq), ("dK", dK), ("dV", dV)):
        assert bool(x.isnan().all()), f"{what} was written by a refused call"
    assert buf.guards_intact()
