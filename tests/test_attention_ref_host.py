"""CPU tier for the attention family (csrc/attn.hip): runs anywhere.

1. tests/attention_ref.py, the fp64 reference the GPU file holds the kernels to, agrees with fp64
   torch.softmax / einsum autograd to 1e-12 on every case without a fully masked mode-1 row (there
   the fp32 absorption step IS the contract and plain fp64 disagrees: asserted below).
2. tests/hostsim.py's attn_fwd / attn_bwd / segment_sum -- the fp32 contract the rest of the suite
   leans on -- stay below 1e-3 of the reference on every case, strided and null-output forms
   included.
3. The preconditions of the fully masked rows, and what the case table must cover.
4. `drive` is the one call sequence (forward -> backward -> segment sums on NaN-poisoned, guarded
   buffers) that both the simulator and the HIP library are put through.
"""
import functools

import pytest
import torch

import attention_ref as ar
import hostsim

SIM = hostsim.HostSim()
NAN = float("nan")
GUARD = 64           # floats of NaN on either side of every writable buffer (256 B: keeps 16-byte alignment)
CASES = ar.cases()
ids = lambda c: c.id  # noqa: E731


class Buffers:
    """NaN-poisoned buffers between NaN guards; shift = 1 starts the buffer one float off 16 bytes."""

    def __init__(self, dev):
        self.dev, self.flat = dev, []

    def new(self, *shape, shift=0):
        n = 1
        for s in shape:
            n *= s
        flat = torch.full((n + 2 * GUARD + shift,), NAN, device=self.dev)
        self.flat.append((flat, GUARD + shift, n))
        return flat[GUARD + shift:GUARD + shift + n].view(*shape)

    def guards_intact(self):
        return all(bool(f[:o].isnan().all()) and bool(f[o + n:].isnan().all()) for f, o, n in self.flat)


def _shifted(t, dev):
    """t's values in a buffer that starts one float past a 16-byte boundary (NaN around it)"""
    flat = torch.full((t.numel() + 8,), NAN, device=dev)
    v = flat[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _padded(t, dev):
    """t [n, P, D] as the leading columns of a [n, P, D + 4] buffer whose padding is NaN"""
    full = torch.full(t.shape[:2] + (t.size(2) + 4,), NAN, device=dev)
    full[..., :t.size(2)] = t
    return full[..., :t.size(2)]


def names(case, backward=True):
    """the tensors a run of `case` produces and is compared on"""
    ns = ["out"] + [n for n in ("attn",) if n not in case.nulls]
    if backward:
        ns += [n for n in ("dq", "dK", "dV") if n not in case.nulls]
        if case.U is not None:
            ns += [n + "u" for n in ("dK", "dV") if n not in case.nulls]
    return ns


def rounded_attn(case):
    """the reference attention rounded to fp32: the input of a backward judged on its own"""
    return reference(case)["attn"].to(torch.float32)


def drive(lib, case, dev=None, attn_src="own"):
    """One pass forward -> backward -> (shared form) segment sums of `lib` (tests/hostsim.HostSim or
    the HIP library) over `case`.  Every writable buffer is NaN before its call and sits between NaN
    guards; the padding columns of the padded layout are guards too.  Asserts that the paths the
    kernels take on these buffers are the ones the table states and that no guard was written;
    returns the tensors as CPU copies in their logical shapes.

    attn_src: "own" = the backward reads the attention the forward just wrote (the product's chain;
    where the case passes attn_out = null there is none and the rounded reference stands in);
    "given" = it reads the fp64 reference attention rounded to fp32 (the backward on its own)."""
    if dev is None:
        dev = "cpu" if lib.name == "hostsim" else "cuda:0"
    B, P, Dk, Dv, mode, nulls = case.B, case.P, case.Dk, case.Dv, case.mode, case.nulls
    U = case.U if case.U is not None else B
    inp = ar.make_inputs(case)
    off = case.layout[4:].split(",") if case.layout.startswith("off:") else []
    assert all(n in ar.OFFSETTABLE for n in off)
    put = lambda name: (_shifted(inp[name], dev) if name in off else inp[name].to(dev).contiguous())  # noqa: E731
    q, dout = put("q"), put("dout")
    mask = None if inp["mask"] is None else inp["mask"].to(dev)
    index = None if inp["index"] is None else inp["index"].to(dev)
    buf = Buffers(dev)
    wide = {}          # name -> the whole buffer of an output that is a view (padding / the other half)
    if case.layout == "kv":
        kv = torch.cat([inp["K"], inp["V"]], 2).to(dev)
        K, V, ldk, ldv = kv[..., :Dk], kv[..., Dk:], Dk + Dv, Dk + Dv
        dkv = buf.new(B, P, Dk + Dv)
        dK, dV, lddk, lddv = dkv[..., :Dk], dkv[..., Dk:], Dk + Dv, Dk + Dv
    elif case.layout == "pad":
        K, V, ldk, ldv = _padded(inp["K"], dev), _padded(inp["V"], dev), Dk + 4, Dv + 4
        wide["dK"], wide["dV"] = buf.new(B, P, Dk + 4), buf.new(B, P, Dv + 4)
        dK, dV, lddk, lddv = wide["dK"][..., :Dk], wide["dV"][..., :Dv], Dk + 4, Dv + 4
    else:
        K, V, ldk, ldv = put("K"), put("V"), Dk, Dv
        dK, dV = buf.new(B, P, Dk, shift="dK" in off), buf.new(B, P, Dv, shift="dV" in off)
        lddk, lddv = (1, 1) if case.layout == "nullld" else (Dk, Dv)
    dq = buf.new(B, Dk, shift="dq" in off)
    out = buf.new(B, Dv)
    attn = buf.new(B, P)
    dq, dK, dV = (None if n in nulls else t for n, t in (("dq", dq), ("dK", dK), ("dV", dV)))
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    pt = ar.paths(Dk, Dv, ldk, ldv, lddk, lddv, *(ptr(t) for t in (q, K, V, dout, dq, dK, dV)))
    assert ar.path_code(pt) == case.path, f"{case.id}: takes {ar.path_code(pt)}, table says {case.path}"
    res = {}

    lib.attn_fwd(q, K, ldk, V, ldv, mask, mode, case.scale, out, None if "attn" in nulls else attn,
                 B, P, Dk, Dv, kv_index=index)
    res["out"] = out.cpu()
    if "attn" in nulls:
        assert bool(attn.isnan().all()), f"{case.id}: a buffer that was not passed has been written"
    else:
        res["attn"] = attn.cpu()
    assert buf.guards_intact(), f"{case.id}: forward wrote into a guard region"

    if attn_src == "given" or "attn" in nulls:
        attn = rounded_attn(case).to(dev)
    lib.attn_bwd(dout, q, K, ldk, V, ldv, mask, mode, case.scale, attn, dq, dK, lddk, dV, lddv,
                 B, P, Dk, Dv, kv_index=index)
    for n, t in (("dq", dq), ("dK", dK), ("dV", dV)):
        if t is not None:
            res[n] = t.cpu()
    for n, full in wide.items():
        D = Dk if n == "dK" else Dv
        assert bool(full[..., D:].isnan().all()), f"{case.id}: {n} wrote into its row padding"
    assert buf.guards_intact(), f"{case.id}: backward wrote into a guard region"

    if case.U is not None:
        assert case.layout == "contig"
        for n, t, D in (("dK", dK, Dk), ("dV", dV, Dv)):
            if t is not None:
                summed = buf.new(U, P, D)
                lib.segment_sum(t, index, B, U, P * D, summed)
                res[n + "u"] = summed.cpu()
        assert buf.guards_intact(), f"{case.id}: segment_sum wrote into a guard region"
    if dev != "cpu":
        torch.cuda.synchronize()
    assert sorted(res) == sorted(names(case))
    return res


def drive_segment_sum(lib, row_elems, dev=None):
    """vlnce_segment_sum alone: B = U = 5, the unsorted index that leaves blocks 1, 2 and 4 out"""
    if dev is None:
        dev = "cpu" if lib.name == "hostsim" else "cuda:0"
    x, index = segment_inputs(row_elems)
    buf = Buffers(dev)
    got = buf.new(5, row_elems)
    lib.segment_sum(x.to(dev), index.to(dev), 5, 5, row_elems, got)
    res = got.cpu()
    assert buf.guards_intact(), f"segment_sum {row_elems}: wrote into a guard region"
    return res


@functools.lru_cache(maxsize=None)
def segment_inputs(row_elems):
    x = torch.randn(5, row_elems, generator=ar._gen("segment", row_elems))
    return x, torch.tensor(ar.SEG_INDEX, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def reference(case, attn_src="own"):
    """fp64 reference of a case (cached: computed once, shared, never modified).  "own": the
    backward follows the fp64 forward; "given": it starts from the fp32-rounded attention, the very
    values the kernel is handed."""
    inp = ar.make_inputs(case)
    B, P, Dk, Dv = case.B, case.P, case.Dk, case.Dv
    args = (inp["q"], inp["K"], Dk, inp["V"], Dv, inp["mask"], case.mode, case.scale)
    out, attn = ar.attn_fwd(*args, B, P, Dk, Dv, kv_index=inp["index"], U=case.U)
    a = attn if attn_src == "own" else attn.to(torch.float32)
    res = ar.attn_bwd(inp["dout"], *args, a, B, P, Dk, Dv, kv_index=inp["index"], U=case.U)
    res.update(out=out, attn=attn)
    return res


@functools.lru_cache(maxsize=None)
def simulated(case, attn_src="own"):
    """hostsim's fp32 result of the same call sequence on the same inputs (cached, shared)"""
    return drive(SIM, case, attn_src=attn_src)


def err(x, x64):
    """max|X - X64| / max(max|X64|, 1e-30); non-finite X -> inf"""
    x, x64 = x.detach().double(), x64.detach().double()
    assert x.shape == x64.shape, (x.shape, x64.shape)
    if not bool(torch.isfinite(x).all()):
        return float("inf")
    return (x - x64).abs().max().item() / max(x64.abs().max().item(), 1e-30)


def exact_expectations(case, res):
    """what must hold to the bit: a mode-2 fully masked row has dq = dK = 0, a block no query
    attends sums to zeros"""
    if case.mode == 2:
        for b in ar.full_rows(case):
            for n in ("dq", "dK"):
                if n in res:
                    assert bool((res[n][b] == 0).all()), f"{case.id}: {n}[{b}] of a fully masked row is not zero"
    if case.U is not None:
        for u in set(range(case.U)) - set(case.index):
            for n in ("dKu", "dVu"):
                if n in res:
                    assert bool((res[n][u] == 0).all()), f"{case.id}: {n}[{u}] of an unattended block is not zero"


def uniform_rows_error(case, res):
    """largest |attn P - 1| over the fully masked rows (0.0 if there are none or attn is not produced)"""
    rows = ar.full_rows(case)
    if not rows or "attn" not in res:
        return 0.0
    return (res["attn"][rows].double() * case.P - 1).abs().max().item()


# ------------------------------------------------------------------ 1. reference vs fp64 autograd
def _has_absorbed_row(case):
    return case.mode == 1 and case.mask == "full"


def _autograd(case):
    inp = ar.make_inputs(case)
    idx = inp["index"] if inp["index"] is not None else torch.arange(case.B)
    q, K, V = (inp[n].double().requires_grad_() for n in ("q", "K", "V"))
    s = torch.einsum("bd,bpd->bp", q, K[idx])
    if inp["mask"] is not None and case.mode == 1:
        s = s - inp["mask"][idx].double() * 1e8
    if inp["mask"] is not None and case.mode == 2:
        s = s * inp["mask"][idx].double()
    a = torch.softmax(s * case.scale, 1)
    out = torch.einsum("bp,bpd->bd", a, V[idx])
    (out * inp["dout"].double()).sum().backward()
    return dict(out=out, attn=a, dq=q.grad, dK=K.grad, dV=V.grad)


@pytest.mark.parametrize("case", [c for c in CASES if not _has_absorbed_row(c)], ids=ids)
def test_reference_matches_fp64_autograd(case):
    ref, auto = reference(case), _autograd(case)
    sfx = "u" if case.U is not None else ""     # autograd sums the shared blocks' gradients itself
    for name, want in (("out", auto["out"]), ("attn", auto["attn"]), ("dq", auto["dq"]),
                       ("dK" + sfx, auto["dK"]), ("dV" + sfx, auto["dV"])):
        e = err(ref[name], want)
        print(f"{case.id} {name}: err={e:.3e}")
        assert e <= 1e-12, (case.id, name, e)


def test_reference_segment_sum_and_path_mirror():
    x, index = segment_inputs(1028)
    want = torch.zeros(5, 1028, dtype=torch.float64).index_add_(0, index, x.double())
    assert err(ar.segment_sum(x, index, 5, 5, 1028), want) <= 1e-15
    base = dict(Dk=8, Dv=8, ldk=8, ldv=8, lddk=8, lddv=8, q=64, K=128, V=256, dout=512, dq=1024, dK=2048, dV=4096)
    code = lambda **kw: ar.path_code(ar.paths(**{**base, **kw}))   # noqa: E731
    assert code() == "vvv" and ar.paths(**base)["strips"] == (0,)
    assert code(Dk=6) == "svs" and code(Dv=6) == "vsv" and code(ldk=10) == "svs" and code(ldv=10) == "vsv"
    assert code(lddk=10) == "vvs" and code(lddv=10) == "vsv"
    assert code(lddk=10, dK=None) == "vvv" and code(lddv=10, dV=0) == "vvv"
    assert code(q=68) == "svs" and code(K=132) == "svs" and code(V=260) == "vsv" and code(dout=516) == "vsv"
    assert code(dq=1028) == "vvs" and code(dK=2052) == "vvs" and code(dV=4100) == "vsv"
    assert code(Dk=1024, ldk=1024, lddk=1024) == "vvv" and code(Dk=1028, ldk=1028, lddk=1028) == "vvs"
    strips = lambda Dk: ar.paths(**{**base, "Dk": Dk, "ldk": Dk, "lddk": Dk})["strips"]   # noqa: E731
    assert [strips(d) for d in (256, 260, 768, 1024, 1028)] == [(0,), (0, 1), (0, 1, 2), (0, 1, 2, 3), ()]


# ------------------------------------------------------------------ 2. hostsim pinned to the reference
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_hostsim_attention_below_1e_3_of_reference(case):
    for src in ("own", "given"):
        ref, sim = reference(case, src), simulated(case, src)
        exact_expectations(case, sim)
        assert uniform_rows_error(case, sim) <= 2.0 ** -22, case.id
        for name in names(case):
            e = err(sim[name], ref[name])
            print(f"{case.id} {src} {name}: E32={e:.3e}")
            assert e < 1e-3, f"{case.id} {src} {name}: hostsim err {e:.3e}"


@pytest.mark.parametrize("row_elems", ar.SEG_ROW_ELEMS)
def test_hostsim_segment_sum(row_elems):
    x, index = segment_inputs(row_elems)
    got = drive_segment_sum(SIM, row_elems)
    assert err(got, ar.segment_sum(x, index, 5, 5, row_elems)) <= 2.0 ** -22
    assert bool((got[[1, 2, 4]] == 0).all())


# ------------------------------------------------------------------ 3. preconditions and coverage
@pytest.mark.parametrize("case", [c for c in CASES if c.mask == "full"], ids=ids)
def test_fully_masked_row_preconditions(case):
    inp = ar.make_inputs(case)
    rows, blocks = ar.full_rows(case), ar.blocks_of(case)
    assert rows, f"{case.id}: no query attends the fully masked block"
    assert len(rows) < case.B, f"{case.id}: no ordinary row beside the fully masked ones"
    m = inp["mask"]
    assert bool((m[case.full] == (1 if case.mode == 1 else 0)).all())
    for u in set(blocks) - {case.full}:       # every other attended row is partial
        assert 0 < int(m[u].sum()) < case.P or case.P == 1
    ref = reference(case)
    if case.mode == 1:
        s = ar.logits64(inp["q"], inp["K"], case.Dk, None, case.B, case.P, case.Dk, inp["index"], case.U)
        assert s[rows].abs().max().item() <= 2.0, "a logit of 4 or more would survive the fp32 subtraction"
        # fp32 absorbs these logits, the reference with it: exactly uniform.  Plain fp64 does not.
        assert bool((ref["attn"][rows] == 1.0 / case.P).all())
        naive = torch.softmax((s[rows] - 1e8) * case.scale, 1)
        assert (naive * case.P - 1).abs().max().item() > 1e-4
    else:
        assert bool((ref["attn"][rows] == 1.0 / case.P).all())
        assert bool((ref["dq"][rows] == 0).all()) and bool((ref["dK"][rows] == 0).all())
    assert float(ref["dV"][rows].abs().max()) > 0


def test_case_table_covers_what_it_must():
    assert len({c.id for c in CASES}) == len(CASES), "duplicate case id"
    plain = lambda c: c.layout == "contig" and not c.nulls and c.U is None   # noqa: E731
    for c in CASES:
        assert 1 <= c.B <= 5 and 1 <= c.P <= ar.MAXP and c.Dk >= 1 and c.Dv >= 1, c.id
        assert c.B * c.P * max(c.Dk, c.Dv) <= 2 * 1024 * 8 * 2, f"{c.id}: not tiny"
        if c.U is not None:
            assert len(c.index) == c.B and all(0 <= u < c.U for u in c.index), c.id
            assert c.P * c.Dk % 4 == 0 and c.P * c.Dv % 4 == 0, c.id
    for P in ar.P_EDGES:
        assert {c.mode for c in CASES if c.group == "P" and c.P == P and (c.Dk, c.Dv) == (8, 8)} == {0, 1, 2}, P
    for Dk in ar.DK_VEC + ar.DK_SCALAR:
        assert any(c.Dk == Dk and plain(c) for c in CASES), Dk
    for Dv in ar.DV_VEC + ar.DV_SCALAR:
        assert any(c.Dv == Dv and plain(c) for c in CASES), Dv
    assert {c.path for c in CASES if c.Dk in ar.DK_VEC and plain(c) and c.Dv == 8} == {"vvv", "vvs"}
    assert {c.path for c in CASES if c.Dk in ar.DK_SCALAR and plain(c) and c.Dv == 8} == {"svs"}
    for i, kind in enumerate(("forward vec", "vec_v", "vec_k")):
        assert {c.path[i] for c in CASES} == {"v", "s"}, kind
    assert {c.path for c in CASES} >= {"vvv", "sss", "vsv", "svs", "vvs", "vss"}      # they disagree, too
    for t in range(4):       # the strips of the vec_k backward
        assert any(c.path[2] == "v" and c.Dk > t * 256 for c in CASES), t
    assert any(c.path == "vvs" and c.Dk > 1024 and c.Dk % 4 == 0 for c in CASES)   # the Dk <= 1024 term
    assert any(c.path[0] == "v" and c.Dk > 256 for c in CASES)      # second trip of the float4 dot product
    assert any(c.P <= 256 for c in CASES) and any(c.P > 256 for c in CASES)
    assert any(c.P == ar.MAXP for c in CASES) and any(c.P < 4 for c in CASES)
    assert {c.mode for c in CASES} == {0, 1, 2}
    assert any(c.mode == 0 and c.mask for c in CASES)
    for mode in (1, 2):
        assert any(c.mode == mode and c.mask == "partial" for c in CASES)
        assert any(c.mode == mode and c.mask == "full" for c in CASES)
    for nulls in ar.NULL_PATTERNS:
        assert {c.path for c in CASES if c.nulls == nulls} >= {"vvv", "sss"}, nulls
    assert {(dk, dv) for (dk, dv) in ar.KV_SPLITS} == {(c.Dk, c.Dv) for c in CASES if c.layout == "kv"}
    assert {c.mode for c in CASES if c.layout == "kv"} == {0, 1}
    assert {"contig", "kv", "pad"} <= {c.layout for c in CASES}
    for name in ar.OFFSETTABLE:     # each misaligned alone, on a shape that is vector otherwise
        assert any(c.layout == "off:" + name and c.Dk % 4 == 0 and c.Dv % 4 == 0 for c in CASES), name
    shared = [c for c in CASES if c.U is not None]
    assert shared and any(c.U is None for c in CASES)
    assert any(c.U == 5 and set(c.index) == {0, 3} and list(c.index) != sorted(c.index) for c in shared)
    assert any(c.B < c.U for c in shared) and any(c.B == 1 for c in shared) and any(c.U == 1 for c in shared)
    assert any(c.scale == 1.0 and c.qs * c.ks >= 16 for c in CASES)
    assert {1e-20, 1e20} <= {c.ds for c in CASES}


def test_conditioning_case_has_logits_in_the_hundreds():
    (case,) = [c for c in CASES if c.scale == 1.0 and c.group == "cond"]
    inp = ar.make_inputs(case)
    s = ar.logits64(inp["q"], inp["K"], case.Dk, None, case.B, case.P, case.Dk)
    assert 100 <= s.abs().max().item() <= 1000


# ------------------------------------------------------------------ 5. the autograd layer on the simulator
@pytest.fixture
def sim_lib(monkeypatch):
    from vlnce_amd import _lib

    monkeypatch.setattr(_lib, "_LIB", SIM)
    return SIM


@pytest.mark.parametrize("case", [c for c in CASES if c.layout == "kv"], ids=ids)
def test_ops_attention_kv_writes_both_halves_of_d_kv(sim_lib, case):
    """ops.attention_kv through the simulator: out, dq and EVERY element of d kv against the reference"""
    from vlnce_amd import ops

    inp, ref = ar.make_inputs(case), reference(case)
    q = inp["q"].clone().requires_grad_()
    kv = torch.cat([inp["K"], inp["V"]], 2).requires_grad_()
    out = ops.attention_kv(q, kv, case.Dk, inp["mask"], case.mode, case.scale)
    (out * inp["dout"]).sum().backward()
    for name, got in (("out", out), ("dq", q.grad), ("dK", kv.grad[..., :case.Dk]), ("dV", kv.grad[..., case.Dk:])):
        assert err(got, ref[name]) < 1e-3, (case.id, name)


@pytest.mark.parametrize("kv_form", [False, True], ids=["attention", "attention_kv"])
def test_ops_attention_accepts_bool_and_sliced_masks_only(sim_lib, monkeypatch, kv_form):
    """bool and uint8 masks of shape [rows, P], contiguous or not, are what the kernels can read;
    anything else is refused before a call is made"""
    from vlnce_amd import ops

    (case,) = [c for c in CASES if c.layout == "kv" and c.Dk == 8 and c.mode == 1]
    inp = ar.make_inputs(case)
    kv, m = torch.cat([inp["K"], inp["V"]], 2), inp["mask"]

    def run(mask):
        if kv_form:
            return ops.attention_kv(inp["q"], kv, case.Dk, mask, 1, case.scale)
        return ops.attention(inp["q"], kv[..., :case.Dk], kv[..., case.Dk:], mask, 1, case.scale)

    base = run(m)
    assert err(base, reference(case)["out"]) < 1e-3
    wide = torch.ones(case.B, case.P + 5, dtype=torch.uint8)
    wide[:, 2:2 + case.P] = m
    for mask in (m.bool(), wide[:, 2:2 + case.P], wide[:, 2:2 + case.P].bool()):
        assert torch.equal(run(mask), base)
    calls = []
    monkeypatch.setattr(SIM, "attn_fwd", lambda *a, **k: calls.append(1))
    for bad, exc in ((m.float(), TypeError), (m.to(torch.int64), TypeError), (m[:, :-1], ValueError),
                     (m.view(-1), ValueError), (m[:-1], ValueError)):
        with pytest.raises(exc):
            run(bad)
    assert calls == [], "a refused mask reached the library"
