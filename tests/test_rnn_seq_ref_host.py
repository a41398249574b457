"""CPU tier for the packed-sequence RNN layer (csrc/rnn_seq.hip): runs anywhere.

1. tests/rnn_seq_ref.py, the fp64 reference the GPU file holds the kernels to, agrees with torch's
   own nn.LSTM / nn.GRU in double() under pack_padded_sequence / pad_packed_sequence to 1e-12.
2. The length-0 semantics the kernels implement (torch's packing rejects such rows) are written
   down and asserted on the reference.
3. tests/hostsim.py's five rnn_seq_* methods -- the fp32 contract the rest of the suite leans on --
   stay within the fp32 floor of the reference on every case of the GPU file.
4. The case lists of tests/test_rnn_seq_fp64_gpu.py are generated HERE (gpu_cases) and checked for
   what they must cover; `drive` is the one call sequence (fwd2 -> bwd2 -> wgrad on NaN-poisoned,
   guarded buffers) that both the simulator and the HIP library are put through.
"""
import collections
import functools
import zlib

import pytest
import torch

import hostsim
import rnn_seq_ref

SIM = hostsim.HostSim()
NAN = float("nan")
GUARD = 64           # floats of NaN on either side of every buffer a call may write (256 B: keeps 16-byte alignment)
KINDS = ("LSTM", "GRU")
PATTERNS = ("full", "ones", "rand_full", "rand_zero", "zero_tile", "short_tile")

Case = collections.namedtuple("Case", "id kind H dirs B L E pattern lengths precision")


def instance(kind, H):
    """the rnn_seq_{fwd,bwd}_kernel<KIND, H, NW> instance pair a (kind, H) launches"""
    return f"{KINDS[kind]}-H{H}-NW{4 if H == 64 else 8}"


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def make_lengths(pattern, B, L, key):
    g = _gen("len", pattern, B, L, key)
    r = lambda lo, hi, n: torch.randint(lo, hi + 1, (n,), generator=g).tolist()  # noqa: E731
    if pattern == "full":
        return [L] * B
    if pattern == "ones":
        return [1] * B
    if pattern == "rand_full":
        ln = r(1, L, B)
        ln[B // 2] = L
        return ln
    if pattern == "rand_zero":
        assert B >= 2
        ln = r(1, L, B)
        ln[B // 3] = 0
        return ln
    assert B > 16 and pattern in ("zero_tile", "short_tile")
    live = r(1, L, B - 16)
    live[(B - 16) // 2] = L
    if pattern == "zero_tile":       # a whole 16-row tile of zeros beside a live tile
        return [0] * 16 + live
    assert L >= 2                    # a tile whose longest row is < L beside one that reaches L
    return r(1, L - 1, 16) + live


def _case(op, kind, H, dirs, B, L, pattern, E=11, precision=False):
    cid = f"{op}-{instance(kind, H)}-d{dirs}-B{B}-L{L}-{pattern}"
    return Case(cid, kind, H, dirs, B, L, E, pattern, tuple(make_lengths(pattern, B, L, cid)), precision)


_CHAIN_SHAPES = [  # (dirs, B, L, pattern): run for each of the four (kind, H)
    (2, 17, 9, "rand_full"), (1, 33, 9, "rand_zero"), (2, 33, 9, "zero_tile"), (1, 17, 9, "short_tile"),
    (2, 16, 2, "full"), (1, 1, 1, "full"), (2, 1, 9, "full"), (1, 16, 9, "ones"), (2, 17, 1, "full"),
    (1, 17, 2, "rand_zero"), (2, 33, 2, "short_tile"), (1, 16, 9, "rand_full"),
]
_KH = [(0, 64), (0, 128), (1, 64), (1, 128)]


def gpu_cases(group):
    """THE case lists of tests/test_rnn_seq_fp64_gpu.py.

    chain:     fwd2 (saving, contiguous seq) -> bwd2 (dseq and dh_final) -> wgrad (one call, dx)
    variant:   one ragged two-tile case per kernel instance for the argument arms (null gates,
               strided / null seq, dseq only / dh_final only / one direction None, unaligned dseq,
               wgrad first_dir / aliasing / ldx / null dx, first-generation equivalence)
    l1:        L = 1 (wgrad's zero-fill arm; fetch(s+1) and fetch_prev(Lt-2) past the ends)
    precision: L = 2, all lengths 2, B = 16: one recurrent product, compared before saturation"""
    if group == "chain":
        return [_case("fwd2+bwd2+wgrad", k, H, *s, E=(24 if s[1] == 33 else 11))
                for (k, H) in _KH for s in _CHAIN_SHAPES]
    if group == "variant":
        return [_case("arms", k, H, 2, 17, 9, "rand_zero", E=13) for (k, H) in _KH]
    if group == "l1":
        return [_case("L1", k, H, 2, 17, 1, "rand_zero", E=13) for (k, H) in _KH]
    if group == "precision":
        return [_case("precision", k, H, 2, 16, 2, "full", precision=True) for (k, H) in _KH]
    raise KeyError(group)


GROUPS = ("chain", "variant", "l1", "precision")
FWD_NAMES = ("out_tm", "seq", "h_final", "gates", "aux")


def compared(case):
    """every tensor a full run of `case` is compared on"""
    names = list(FWD_NAMES) + ["dgi"] + (["dgh"] if case.kind == 1 else [])
    if not case.precision:
        names += ["dw_ih", "db_ih", "dw_hh", "db_hh", "dx"]
    return names


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """fp32 CPU inputs of a case, weights at torch's default scale U(-1/sqrt(H), 1/sqrt(H))."""
    kind, H, dirs, B, L, E = case.kind, case.H, case.dirs, case.B, case.L, case.E
    GH = (4 if kind == 0 else 3) * H
    g = _gen("inputs", case.id)
    k = H ** -0.5
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k  # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g)               # noqa: E731
    inp = dict(x=n(L * B, E), w_ih=[u(GH, E) for _ in range(dirs)], b_ih=[u(GH) for _ in range(dirs)],
               w_hh=[u(GH, H) for _ in range(dirs)], b_hh=[u(GH) for _ in range(dirs)],
               dseq=n(B, L, dirs * H), dhf=[n(B, H) for _ in range(dirs)])
    # what the kernels are fed: the fp32 projection (the reference runs on these VALUES)
    inp["gi"] = [(inp["x"] @ inp["w_ih"][d].t() + inp["b_ih"][d]).view(L, B, GH) for d in range(dirs)]
    if case.precision:
        # the step processed first (h = 0: no recurrent product) drives the gates hard so that h
        # is large; the second step's input is small, so its gates sit where the non-linearities
        # are steepest and the recurrent product h W_hh^T is what they show.  The output gradient
        # arrives at the step processed last only, so the first step's dgi is what came back
        # through dgates W_hh.
        assert L == 2
        inp["gi"] = [n(L, B, GH) for _ in range(dirs)]
        for d in range(dirs):
            first, second = (0, 1) if d == 0 else (1, 0)
            inp["gi"][d][first] *= 3.0
            inp["gi"][d][second] *= 0.05
            inp["dseq"][:, first, d * H:(d + 1) * H] = 0.0
    return inp


def _grads(inp, grad, dirs):
    dseq = inp["dseq"] if grad in ("both", "dseq") else None
    dhf = {"both": list(inp["dhf"]), "dhf": list(inp["dhf"]), "dseq": None, None: None,
           "dhf0": [inp["dhf"][0], None], "dhf1": [None, inp["dhf"][-1]]}[grad]
    if dhf is not None:
        dhf = dhf[:dirs]
    return dseq, dhf


@functools.lru_cache(maxsize=None)
def reference(case, grad="both"):
    """fp64 reference of a case (cached: computed once, shared, never modified)"""
    inp = make_inputs(case)
    dseq, dhf = _grads(inp, grad, case.dirs)
    kw = dict(gi=inp["gi"]) if case.precision else dict(x_tm=inp["x"], w_ih=inp["w_ih"], b_ih=inp["b_ih"],
                                                         gi=inp["gi"])
    return rnn_seq_ref.run(case.kind, case.dirs, case.H, case.lengths, inp["w_hh"], inp["b_hh"],
                           dseq=dseq, dh_final=dhf, **kw)


class Buffers:
    """NaN-poisoned buffers with NaN guards around them."""

    def __init__(self, dev):
        self.dev, self.flat = dev, []

    def new(self, *shape):
        n = 1
        for s in shape:
            n *= s
        flat = torch.full((n + 2 * GUARD,), NAN, device=self.dev)
        self.flat.append((flat, n))
        return flat[GUARD:GUARD + n].view(*shape)

    def guards_intact(self):
        return all(bool(f[:GUARD].isnan().all()) and bool(f[GUARD + n:].isnan().all()) for f, n in self.flat)


def alive_mask(case):
    """[L, B, 1] bool: t < len[b]"""
    ln = torch.tensor(case.lengths)
    return (torch.arange(case.L).view(-1, 1) < ln.view(1, -1)).unsqueeze(-1)


def drive(lib, dev, case, *, save=True, seq_mode="contig", grad="both", dseq_mode="contig",
          wgrad="one", alias_db=False, ldx_pad=0, want_dx=True, clean_saved=False, generation=2):
    """One pass fwd -> bwd -> wgrad of `lib` (tests/hostsim.HostSim or the HIP library) over `case`
    on NaN-poisoned buffers.  Asserts the poison contract (exact zeros past each length in out_tm,
    seq, dgi, dgh; guards still NaN) and returns the tensors as CPU copies.

    seq_mode: contig | strided (a [:, :L, :dirs*H] slice of a [B, L+3, dirs*H+8] buffer) | none
    grad: both | dseq | dhf | dhf0 ([t, None]) | dhf1 ([None, t]) | None (forward only)
    dseq_mode: contig | unaligned (slice of a longer padded buffer, data pointer 4 bytes off 16)
    wgrad: one (all directions in one call) | two (dirs = 1 calls with first_dir 0 and 1) | None
    clean_saved: zero gates / aux past the lengths before the backward (default: left NaN)
    generation: 1 = vlnce_rnn_seq_fwd / _bwd on pre-zeroed buffers with transposed weights"""
    kind, H, dirs, B, L, E = case.kind, case.H, case.dirs, case.B, case.L, case.E
    GH = (4 if kind == 0 else 3) * H
    inp = make_inputs(case)
    to = lambda t: t.to(dev).contiguous()  # noqa: E731
    gi, w_hh, b_hh = [to(t) for t in inp["gi"]], [to(t) for t in inp["w_hh"]], [to(t) for t in inp["b_hh"]]
    lens = torch.tensor(case.lengths, dtype=torch.int32).to(dev)
    alive = alive_mask(case)
    dead = ~alive.expand(L, B, 1)
    buf = Buffers(dev)
    res = {}

    out_tm = [buf.new(L, B, H) for _ in range(dirs)]
    hfin = [buf.new(B, H) for _ in range(dirs)]
    gates = [buf.new(L, B, GH) for _ in range(dirs)] if save else None
    aux = [buf.new(L, B, H) for _ in range(dirs)] if save else None
    seq = seq_full = None
    if generation == 1:
        for t in out_tm:
            t.zero_()
        lib.rnn_seq_fwd(kind, dirs, gi, w_hh, b_hh, lens, out_tm, hfin, gates, aux, B, L, H)
    else:
        st = sb = 0
        if seq_mode == "contig":
            seq = seq_full = buf.new(B, L, dirs * H)
        elif seq_mode == "strided":
            seq_full = buf.new(B, L + 3, dirs * H + 8)
            seq = seq_full[:, :L, :dirs * H]
        if seq is not None:
            sb, st = seq.stride(0), seq.stride(1)
        lib.rnn_seq_fwd2(kind, dirs, gi, w_hh, b_hh, lens, out_tm, seq, st, sb, hfin, gates, aux, B, L, H)
    res["out_tm"] = [t.cpu() for t in out_tm]
    res["h_final"] = [t.cpu() for t in hfin]
    for d in range(dirs):
        assert bool((res["out_tm"][d][dead.expand(L, B, H)] == 0).all()), f"{case.id}: out_tm[{d}] tail not zero"
    if seq is not None:
        res["seq"] = seq.cpu()
        dead_seq = dead.expand(L, B, dirs * H).transpose(0, 1)
        assert bool((res["seq"][dead_seq] == 0).all()), f"{case.id}: seq tail not zero"
        if seq_mode == "strided":   # the slice's own guard region: rows L..L+2 and columns dirs*H..+7
            full = seq_full.cpu()
            assert bool(full[:, L:, :].isnan().all()) and bool(full[:, :, dirs * H:].isnan().all()), \
                f"{case.id}: seq wrote outside its strided view"
    if save:
        # unspecified past the lengths: compared (and required finite) at live positions only
        res["gates"] = [torch.where(alive, t.cpu(), torch.zeros(())) for t in gates]
        res["aux"] = [torch.where(alive, t.cpu(), torch.zeros(())) for t in aux]
    assert buf.guards_intact(), f"{case.id}: forward wrote into a guard region"

    if grad is not None:
        assert save
        dseq_c, dhf_c = _grads(inp, grad, dirs)
        dhf = [to(t) if t is not None else None for t in dhf_c] if dhf_c is not None else None
        dseq = None
        st = sb = 0
        if dseq_c is not None:
            if dseq_mode == "contig":
                dseq = to(dseq_c)
            else:
                W = dirs * H + 5
                big = torch.randn(B * (L + 2) * W + 4, generator=_gen("pad", case.id)).to(dev)
                dseq = big[1:1 + B * (L + 2) * W].view(B, L + 2, W)[:, :L, :dirs * H]
                dseq.copy_(dseq_c)
                assert dev == "cpu" or dseq.data_ptr() % 16 != 0
            sb, st = dseq.stride(0), dseq.stride(1)
        if clean_saved:
            for t in gates + aux:
                t.masked_fill_(dead.to(dev), 0.0)
        dgi = [buf.new(L, B, GH) for _ in range(dirs)]
        dgh = [buf.new(L, B, GH) for _ in range(dirs)] if kind == 1 else None
        if generation == 1:
            for t in dgi + (dgh or []):
                t.zero_()
            dout = None
            if dseq is not None:
                dout = [dseq.transpose(0, 1)[:, :, d * H:(d + 1) * H].contiguous() for d in range(dirs)]
            lib.rnn_seq_bwd(kind, dirs, [w.t().contiguous() for w in w_hh], lens, out_tm, gates, aux, dout,
                            dhf, dgi, dgh, B, L, H)
        else:
            ws = buf.new(dirs, L, B, H) if dseq is not None else None
            lib.rnn_seq_bwd2(kind, dirs, w_hh, lens, out_tm, gates, aux, dseq, st, sb, ws, dhf, dgi, dgh,
                             B, L, H)
        res["dgi"] = [t.cpu() for t in dgi]
        if kind == 1:
            res["dgh"] = [t.cpu() for t in dgh]
        for name in ("dgi", "dgh")[:1 + kind]:
            for d in range(dirs):
                assert bool((res[name][d][dead.expand(L, B, GH)] == 0).all()), \
                    f"{case.id}: {name}[{d}] tail not zero"
        assert buf.guards_intact(), f"{case.id}: backward wrote into a guard region"

        if wgrad is not None and generation == 2:
            ldx = E + ldx_pad
            xp = torch.randn(L * B, ldx, generator=_gen("xpad", case.id))
            xp[:, :E] = inp["x"]
            xp = xp.to(dev)
            w_ih = [to(t) for t in inp["w_ih"]]
            dw_ih = [buf.new(GH, E) for _ in range(dirs)]
            dw_hh = [buf.new(GH, H) for _ in range(dirs)]
            db_hh = [buf.new(GH) for _ in range(dirs)]
            db_ih = db_hh if alias_db else [buf.new(GH) for _ in range(dirs)]
            if wgrad == "one":
                dx = buf.new(L * B, E) if want_dx else None
                lib.rnn_seq_wgrad(kind, dirs, dgi, dgh, out_tm, xp, ldx, E, w_ih, dw_ih, dw_hh, db_ih, db_hh,
                                  dx, B, L, H)
                if want_dx:
                    res["dx"] = dx.cpu()
            else:
                dxs = [buf.new(L * B, E) if want_dx else None for _ in range(dirs)]
                for d in range(dirs):
                    one = slice(d, d + 1)
                    lib.rnn_seq_wgrad(kind, 1, dgi[one], dgh[one] if dgh else None, out_tm[one], xp, ldx, E,
                                      w_ih[one], dw_ih[one], dw_hh[one], db_ih[one], db_hh[one], dxs[d],
                                      B, L, H, first_dir=d)
                if want_dx:
                    res["dx_parts"] = [t.cpu() for t in dxs]
            for name, ts in (("dw_ih", dw_ih), ("dw_hh", dw_hh), ("db_ih", db_ih), ("db_hh", db_hh)):
                res[name] = [t.cpu() for t in ts]
            assert buf.guards_intact(), f"{case.id}: wgrad wrote into a guard region"
    if dev != "cpu":
        torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def simulated(case, **opts):
    """hostsim's fp32 result of the same call sequence on the same inputs (cached, shared)"""
    return drive(SIM, "cpu", case, **opts)


def err(x, x64):
    """max|X - X64| / max(max|X64|, 1e-30); non-finite X -> inf"""
    x, x64 = x.detach().double(), x64.detach().double()
    assert x.shape == x64.shape, (x.shape, x64.shape)
    if not bool(torch.isfinite(x).all()):
        return float("inf")
    return (x - x64).abs().max().item() / max(x64.abs().max().item(), 1e-30)


def pairs(res, ref, names):
    """(label, tensor, reference tensor) of every named tensor, per direction"""
    for name in names:
        got, want = res[name], ref[name]
        if isinstance(got, list):
            for d, (g, w) in enumerate(zip(got, want)):
                yield f"{name}[{d}]", name, g, w
        else:
            yield name, name, got, want.view(got.shape)


# ------------------------------------------------------------------ 1. reference vs torch's packed RNNs
@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("kind", [0, 1], ids=KINDS)
def test_reference_matches_torch_packed_rnn(kind, dirs, H):
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

    B, L, E = 6, 7, 5
    g = _gen("torch", kind, dirs, H)
    lengths = torch.randint(1, L + 1, (B,), generator=g)
    lengths[2] = L
    lengths[4] = 1
    mod = (torch.nn.LSTM if kind == 0 else torch.nn.GRU)(E, H, bidirectional=dirs == 2).double()
    for p in mod.parameters():
        p.data.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.3)
    x = torch.randn(L, B, E, generator=g, dtype=torch.float64, requires_grad=True)
    dseq = torch.randn(B, L, dirs * H, generator=g, dtype=torch.float64)
    dhf = [torch.randn(B, H, generator=g, dtype=torch.float64) for _ in range(dirs)]
    packed = pack_padded_sequence(x, lengths, enforce_sorted=False)
    y, hn = mod(packed)
    y, _ = pad_packed_sequence(y, total_length=L)          # [L, B, dirs*H]
    if kind == 0:
        hn = hn[0]
    ((y.transpose(0, 1) * dseq).sum() + sum((hn[d] * dhf[d]).sum() for d in range(dirs))).backward()

    sfx = ["", "_reverse"][:dirs]
    par = lambda n: [getattr(mod, f"{n}_l0{s}") for s in sfx]  # noqa: E731
    ref = rnn_seq_ref.run(kind, dirs, H, lengths, par("weight_hh"), par("bias_hh"), x_tm=x.view(L * B, E),
                          w_ih=par("weight_ih"), b_ih=par("bias_ih"), dseq=dseq, dh_final=dhf)
    checks = [("seq", ref["seq"], y.transpose(0, 1)), ("dx", ref["dx"], x.grad.view(L * B, E))]
    for d in range(dirs):
        checks += [(f"h_final[{d}]", ref["h_final"][d], hn[d]),
                   (f"out_tm[{d}]", ref["out_tm"][d], y[:, :, d * H:(d + 1) * H])]
        for name, attr in (("dw_ih", "weight_ih"), ("db_ih", "bias_ih"), ("dw_hh", "weight_hh"),
                           ("db_hh", "bias_hh")):
            checks.append((f"{name}[{d}]", ref[name][d], par(attr)[d].grad))
    for what, a, b in checks:
        e = err(a, b)
        print(f"{what}: err={e:.3e}")
        assert e <= 1e-12, (what, e)
    # the saved quantities are consistent with the outputs (the kernels' layout)
    for d in range(dirs):
        gt, ax, out = ref["gates"][d], ref["aux"][d], ref["out_tm"][d]
        if kind == 0:
            assert err(gt[..., 3 * H:] * torch.tanh(ax), out) <= 1e-12
        else:   # dgh of the n gate is dgi's n gate times r
            assert err(ref["dgh"][d][..., 2 * H:], ref["dgi"][d][..., 2 * H:] * gt[..., :H]) <= 1e-12
            assert err(ref["dgh"][d][..., :2 * H], ref["dgi"][d][..., :2 * H]) <= 1e-12


# ------------------------------------------------------------------ 2. length 0
@pytest.mark.parametrize("kind", [0, 1], ids=KINDS)
def test_reference_length_zero_row_is_zeros_and_leaves_neighbours_alone(kind):
    """Contract 0 <= len <= L.  A row of length 0 is never alive: its outputs, final state, saved
    quantities and every gradient row are zeros, and the other rows get exactly what they get in the
    same batch without that row."""
    H, dirs, B, L, E, z = 64, 2, 5, 4, 3, 2
    G = 4 if kind == 0 else 3
    g = _gen("zero", kind)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) * 0.4  # noqa: E731
    lengths = [3, 4, 0, 1, 2]
    x, dseq = n(L, B, E), n(B, L, dirs * H)
    w_ih, b_ih = [n(G * H, E) for _ in range(dirs)], [n(G * H) for _ in range(dirs)]
    w_hh, b_hh = [n(G * H, H) for _ in range(dirs)], [n(G * H) for _ in range(dirs)]
    dhf = [n(B, H) for _ in range(dirs)]
    full = rnn_seq_ref.run(kind, dirs, H, lengths, w_hh, b_hh, x_tm=x.reshape(L * B, E), w_ih=w_ih, b_ih=b_ih,
                           dseq=dseq, dh_final=dhf)
    keep = [b for b in range(B) if b != z]
    less = rnn_seq_ref.run(kind, dirs, H, [lengths[b] for b in keep], w_hh, b_hh,
                           x_tm=x[:, keep].reshape(L * (B - 1), E), w_ih=w_ih, b_ih=b_ih,
                           dseq=dseq[keep], dh_final=[t[keep] for t in dhf])
    assert bool((full["seq"][z] == 0).all()) and bool((full["dx"].view(L, B, E)[:, z] == 0).all())
    assert torch.equal(full["seq"][keep], less["seq"])
    assert err(full["dx"].view(L, B, E)[:, keep], less["dx"].view(L, B - 1, E)) <= 1e-14
    for d in range(dirs):
        assert bool((full["h_final"][d][z] == 0).all())
        for name in ("out_tm", "gates", "aux", "dgi"):
            assert bool((full[name][d][:, z] == 0).all()), name
            assert err(full[name][d][:, keep], less[name][d]) <= 1e-14, name
        assert torch.equal(full["h_final"][d][keep], less["h_final"][d])
        for name in ("dw_ih", "db_ih", "dw_hh", "db_hh"):   # sums over rows: order of summation only
            assert err(full[name][d], less[name][d]) <= 1e-13, name
    with pytest.raises(AssertionError):     # len > L is outside the contract
        rnn_seq_ref.run(kind, dirs, H, [L + 1] * B, w_hh, b_hh, x_tm=x.reshape(L * B, E), w_ih=w_ih, b_ih=b_ih)


# ------------------------------------------------------------------ 3. the GPU file's case lists
def test_gpu_case_lists_cover_what_they_must():
    chain = gpu_cases("chain")
    every = [c for grp in GROUPS for c in gpu_cases(grp)]
    assert len({c.id for c in every}) == len(every), "duplicate case id"
    for c in every:
        assert 1 <= c.L <= 12 and 1 <= c.B <= 33 and 1 <= c.E <= 24, c.id
        assert len(c.lengths) == c.B and all(0 <= n <= c.L for n in c.lengths), c.id   # NEVER len > L
        assert any(n > 0 for n in c.lengths), f"{c.id}: no active row"
        assert instance(c.kind, c.H) in c.id
        full = set(FWD_NAMES) | {"dgi"} | ({"dgh"} if c.kind == 1 else set())
        if not c.precision:
            full |= {"dw_ih", "db_ih", "dw_hh", "db_hh", "dx"}
        assert set(compared(c)) == full, f"{c.id}: leaves out a compared tensor"
    for grp in GROUPS:     # all eight kernel instances (forward and backward run in every case)
        assert {(c.kind, c.H) for c in gpu_cases(grp)} == set(_KH), grp
    assert {(c.kind, c.H, c.dirs) for c in chain} == {(k, H, d) for (k, H) in _KH for d in (1, 2)}
    for (k, H) in _KH:
        mine = [c for c in chain if (c.kind, c.H) == (k, H)]
        assert {c.B for c in mine} == {1, 16, 17, 33}
        assert {c.L for c in mine} == {1, 2, 9}
        assert {c.pattern for c in mine} == set(PATTERNS)
    for c in every:
        ln, L = c.lengths, c.L
        if c.pattern == "full":
            assert set(ln) == {L}
        elif c.pattern == "ones":
            assert set(ln) == {1}
        elif c.pattern == "rand_full":
            assert L in ln and min(ln) >= 1
        elif c.pattern == "rand_zero":
            assert ln.count(0) == 1
        elif c.pattern == "zero_tile":
            assert set(ln[:16]) == {0} and max(ln[16:]) == L and min(ln[16:]) >= 1
        elif c.pattern == "short_tile":
            assert 1 <= max(ln[:16]) < L and max(ln[16:]) == L
    assert all(c.L == 1 for c in gpu_cases("l1"))
    assert all(c.L == 2 and c.B == 16 and set(c.lengths) == {2} for c in gpu_cases("precision"))
    assert all(c.dirs == 2 and 0 in c.lengths and c.B > 16 for c in gpu_cases("variant"))


# ------------------------------------------------------------------ 4. hostsim pinned to the reference
def fp32_floor(case):
    """What fp32 arithmetic may lose against fp64 on a case, relative to a tensor's maximum: the
    worst-case bound n * 2^-24 of one dot product, n the longest one in the chain -- 4H gate
    gradients per row in BPTT, L*B rows in the parameter gradients -- taken once for each of them."""
    return (4 * case.H + case.L * case.B) * 2.0 ** -24


def _hostsim_within_floor(case, **opts):
    ref = reference(case, opts.get("grad", "both"))
    sim = simulated(case, **opts)
    names = [n for n in compared(case) if n in sim]
    assert "dgi" in names and (case.precision or "dx" in names or opts.get("wgrad") == "two")
    worst = 0.0
    for label, _, got, want in pairs(sim, ref, names):
        e = err(got, want)
        worst = max(worst, e)
        assert e <= fp32_floor(case), f"{case.id} {label}: hostsim err {e:.3e} > {fp32_floor(case):.3e}"
    return worst


@pytest.mark.parametrize("case", [c for grp in GROUPS for c in gpu_cases(grp)], ids=lambda c: c.id)
def test_hostsim_rnn_seq_within_fp32_floor_of_reference(case):
    """rnn_seq_fwd2 / _bwd2 / _wgrad of the simulator (which run its rnn_seq_fwd / _bwd) on the GPU
    file's cases, poisoned buffers and all."""
    kw = dict(wgrad=None) if case.precision else {}
    print(f"{case.id}: worst err {_hostsim_within_floor(case, **kw):.3e} floor {fp32_floor(case):.3e}")


@pytest.mark.parametrize("case", gpu_cases("variant"), ids=lambda c: c.id)
def test_hostsim_rnn_seq_argument_arms(case):
    """the simulator through the argument arms the GPU file drives"""
    base = simulated(case)
    for opts in (dict(grad="dseq"), dict(grad="dhf"), dict(grad="dhf0"), dict(grad="dhf1"),
                 dict(seq_mode="strided"), dict(dseq_mode="unaligned"), dict(ldx_pad=3), dict(wgrad="two")):
        _hostsim_within_floor(case, **opts)
    one = simulated(case, generation=1, wgrad=None)
    for label, _, got, want in pairs(one, base, ["out_tm", "h_final", "gates", "aux", "dgi"]
                                     + (["dgh"] if case.kind == 1 else [])):
        assert torch.equal(got, want), f"{case.id}: first generation differs in {label}"
    two = simulated(case, wgrad="two")
    assert err(two["dx_parts"][0] + two["dx_parts"][1], base["dx"]) <= 2.0 ** -22
