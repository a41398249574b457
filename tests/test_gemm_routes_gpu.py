"""Every route of vlnce_gemm by name, and against the fp64 product with its full epilogue.

Behind vlnce_gemm sit six loader pairs of igemm_kernel, three tiles, two split-K rules, a zero-fill, a
second bias / activation pass and two epilogues (include/vlnce_hip.h: vlnce_gemm_last_kernel).  ROUTES
below lists every (loader pair, tile, split or not) the entry point can reach, with the smallest call
that lands on it; per row, and per cell of the operand / epilogue matrix, the tests assert
  * the route that ran (HipLib.gemm_last_kernel(), directly after the launch, on the calling thread)
    against tests/gemm_dispatch.py, the dispatch written out a second time,
  * the relative rms error against the fp64 product of the same operands: < 1e-6, the project's
    bound (tests/test_conv_routes_gpu.py),
  * the largest rms error over aligned 32 x 32 output blocks, relative to the reference's global rms:
    at most 3 x the same figure of the fp32 CPU contract (tests/hostsim.py) on the same operands,
  * the guard band: C lies in a larger NaN-filled allocation (ldc > N columns, rows past M, the
    floats in front of a 4-byte-aligned C) that must come back bit for bit; the padding of A, B and
    the residual is NaN as well, so a loader that reads past K, M or N poisons the output.
tests/test_gemm_routes_host.py shows, without a GPU, that the two statistics fail on planted defects
of the kinds these kernels could have."""
import collections
import functools

import pytest
import torch

import gemm_dispatch as gd
import test_conv_routes_gpu as cr
from gemm_dispatch import Call
from test_kernels_gpu import DEV, SIM, rnd
from vlnce_amd import _lib, ops
from vlnce_amd._lib import GemmKernel

pytestmark = pytest.mark.gpu

RMS_BOUND, BLOCK_FACTOR = 1e-6, 3.0
GUARD_ROWS = 3
T64, T128x64, T128 = (64, 64), (128, 64), (128, 128)


@pytest.fixture(scope="module")
def hip():
    return _lib.get_lib()


# ------------------------------------------------------------------ the route table
Row = collections.namedtuple("Row", "name call opts want")
ROUTES, FOLDS, EDGES = [], [], []


def _row(table, name, want, M, N, K, ta=0, tb=0, opts=None, **kw):
    """ldc = N + 4: guard columns that keep ldc % 4; `want` = (a, b, tile, split factor)"""
    table.append(Row(name, Call(M, N, K, ta, tb, ldc=N + 4, **kw), opts or {}, want))


# A_BUF / B_BUF: K % 32 == 0, everything 16-byte aligned.  70 x 52: two row tiles of 64 (the second
# with 6 rows), one of 128 rows with 58 of them empty, 12 empty columns
_row(ROUTES, "buf-plain", ("buf", "buf", T64, 1), 70, 52, 64)                      # KT = 2: no split
_row(ROUTES, "buf-split8", ("buf", "buf", T64, 8), 70, 52, 512)                    # 2 tiles, KT = 16
_row(ROUTES, "buf-tile128x128", ("buf", "buf", T128, 1), 70, 52, 64, opts=dict(igemm_tile=1))
_row(ROUTES, "buf-tile128x64", ("buf", "buf", T128x64, 1), 70, 52, 64, opts=dict(igemm_tile=2))
_row(ROUTES, "buf-tile64x64", ("buf", "buf", T64, 1), 70, 52, 64, opts=dict(igemm_tile=3))
# A_IM2COL_V4 / B_NK_V4: K % 4 == 0 but not % 32 (ragged last K-tile), or option "igemm_nobuf"
_row(ROUTES, "v4-plain", ("v4", "nk_v4", T64, 1), 70, 52, 36)
_row(ROUTES, "v4-split6", ("v4", "nk_v4", T64, 6), 70, 52, 388)                    # KT = 13
_row(ROUTES, "v4-nobuf", ("v4", "nk_v4", T64, 1), 70, 52, 64, opts=dict(igemm_nobuf=1))
_row(ROUTES, "v4-nobuf-split8", ("v4", "nk_v4", T64, 8), 70, 52, 512, opts=dict(igemm_nobuf=1))
_row(ROUTES, "v4-tile128x128", ("v4", "nk_v4", T128, 1), 70, 52, 36, opts=dict(igemm_tile=1))
_row(ROUTES, "v4-tile128x64", ("v4", "nk_v4", T128x64, 1), 70, 52, 36, opts=dict(igemm_tile=2))
# A_IM2COL_S / B_NK_S (always 64 x 64), reached five ways
_row(ROUTES, "s-K50", ("s", "nk_s", T64, 1), 70, 52, 50)
_row(ROUTES, "s-K323-split5", ("s", "nk_s", T64, 5), 70, 52, 323)                  # KT = 11
_row(ROUTES, "s-lda37", ("s", "nk_s", T64, 1), 70, 52, 36, lda=37)
_row(ROUTES, "s-lda389-split6", ("s", "nk_s", T64, 6), 70, 52, 388, lda=389)
_row(ROUTES, "s-ldb37", ("s", "nk_s", T64, 1), 70, 52, 36, ldb=37)
_row(ROUTES, "s-A+1float", ("s", "nk_s", T64, 1), 70, 52, 36, a_align=4)
_row(ROUTES, "s-A+1float-split6", ("s", "nk_s", T64, 6), 70, 52, 388, a_align=4)
_row(ROUTES, "s-B+1float", ("s", "nk_s", T64, 1), 70, 52, 36, b_align=4)
_row(ROUTES, "s-B+1float-split6", ("s", "nk_s", T64, 6), 70, 52, 388, b_align=4)
# ... / B_KN (transB): the B loader's 16-byte form (N % 4 == 0, ldb % 4 == 0) and its scalar form (N = 50)
for _n in (52, 50):
    _row(ROUTES, f"v4-kn-N{_n}", ("v4", "kn", T64, 1), 70, _n, 64, 0, 1)
    _row(ROUTES, f"v4-kn-N{_n}-split8", ("v4", "kn", T64, 8), 70, _n, 512, 0, 1)
    _row(ROUTES, f"s-kn-N{_n}", ("s", "kn", T64, 1), 70, _n, 50, 0, 1)
    _row(ROUTES, f"s-kn-N{_n}-split5", ("s", "kn", T64, 5), 70, _n, 323, 0, 1)
_row(ROUTES, "v4-kn-tile128x128", ("v4", "kn", T128, 1), 70, 52, 64, 0, 1, opts=dict(igemm_tile=1))
_row(ROUTES, "v4-kn-tile128x64", ("v4", "kn", T128x64, 1), 70, 52, 64, 0, 1, opts=dict(igemm_tile=2))
# A_TRANS / B_KN (transA): the A loader's 16-byte form (M % 4 == 0, lda % 4 == 0) and its scalar form
for _m in (72, 70):
    _row(ROUTES, f"trans-M{_m}", ("trans", "kn", T64, 1), _m, 52, 64, 1, 1)
    _row(ROUTES, f"trans-M{_m}-split8", ("trans", "kn", T64, 8), _m, 52, 512, 1, 1)
_row(ROUTES, "trans-tile128x128", ("trans", "kn", T128, 1), 70, 52, 64, 1, 1, opts=dict(igemm_tile=1))
_row(ROUTES, "trans-tile128x64", ("trans", "kn", T128x64, 1), 70, 52, 64, 1, 1, opts=dict(igemm_tile=2))
# transA's long-reduction rule: KT >= 32 and 128 <= tiles < 1024 -- 8 x 16 tiles, KT = 32: the
# smallest such shape (1 GFLOP, the largest call of this file)
_row(ROUTES, "trans-long-M512-split8", ("trans", "kn", T64, 8), 512, 1024, 1024, 1, 1)
_row(ROUTES, "trans-long-M510-split8", ("trans", "kn", T64, 8), 510, 1024, 1024, 1, 1)
# row folding: the "image" is 1024 wide and ceil(M / 1024) high, its last row nearly empty
for _m in (1025, 1030):
    _row(FOLDS, f"fold-buf-M{_m}", ("buf", "buf", T64, 1), _m, 52, 64)
    _row(FOLDS, f"fold-v4-M{_m}", ("v4", "nk_v4", T64, 1), _m, 52, 36)
# one step either side of the constants of choose_splitk and choose_tile (no option set), so that a
# changed constant moves a row: the table above sits on "at least two K-tiles per range" alone
_row(EDGES, "edge-KT7", ("buf", "buf", T64, 1), 70, 52, 224)                      # KT < 8: no split
_row(EDGES, "edge-KT8-split4", ("buf", "buf", T64, 4), 70, 52, 256)
_row(EDGES, "edge-127tiles-split3", ("buf", "buf", T64, 3), 64 * 127, 52, 256)    # ceil(256 / 127)
_row(EDGES, "edge-128tiles", ("buf", "buf", T64, 1), 64 * 128, 52, 256)           # tiles >= 128: no split
_row(EDGES, "edge-256wgs-split11", ("buf", "buf", T64, 11), 70, 768, 1024)        # 24 tiles: ceil(256 / 24)
_row(EDGES, "edge-cap-split64", ("buf", "buf", T64, 64), 70, 52, 8192)            # KT / 2 = 128: at most 64
_row(EDGES, "edge-trans-KT31", ("trans", "kn", T64, 1), 512, 1024, 992, 1, 1)     # long rule needs KT >= 32
_row(EDGES, "edge-trans-120tiles-split3", ("trans", "kn", T64, 3), 512, 960, 1024, 1, 1)   # ... and 128 tiles
_row(EDGES, "edge-512tiles-128x128", ("buf", "buf", T128, 1), 2048, 4096, 32)     # 16 x 32 tiles of 128 x 128
_row(EDGES, "edge-496tiles-128x64", ("buf", "buf", T128x64, 1), 2048, 3968, 32)   # 16 x 31, 16 x 62 of 128 x 64
_row(EDGES, "edge-512tiles-128x64", ("buf", "buf", T128x64, 1), 2048, 2048, 32)   # 16 x 32 of 128 x 64
_row(EDGES, "edge-496tiles-64x64", ("buf", "buf", T64, 1), 2048, 1984, 32)
_row(EDGES, "edge-N64-64x64", ("v4", "kn", T64, 1), 64 * 520, 64, 32, 0, 1)       # N <= 64: 64 x 64 whatever M
# (not separated, as every such shape is above 1 GFLOP: the long rule's 1024 workgroups from its "at
# least four K-tiles per range", and its upper end of 1024 tiles)


def want_kernel(row):
    """a table row's (a, b, tile, split) as the full record of a call without epilogue operands"""
    a, b, tile, split = row.want
    return GemmKernel(a, b, tile, split, split > 1, False)


# ------------------------------------------------------------------ operands, references, statistics
def _store(mat, ld, off, extra_rows=0):
    """a [rows, cols] matrix at row stride ld, `off` floats into a flat NaN-filled buffer"""
    rows, cols = mat.shape
    assert ld >= cols
    buf = torch.full((off + (rows + extra_rows) * ld,), float("nan"))
    buf[off:].as_strided((rows, cols), (ld, 1)).copy_(mat)
    return buf


def _off(align):
    return {16: 0, 4: 1}[align]


@functools.lru_cache(maxsize=None)
def operands(c):
    """CPU buffers of one call as the kernel sees them (strides, offsets, NaN padding), the fp64
    reference of the whole call and the fp32 CPU contract's result on the same buffers"""
    A = rnd(c.M, c.K, seed=61) * c.K ** -0.5
    B = rnd(c.K, c.N, seed=62)
    t = dict(A=_store(A.t() if c.transA else A, c.lda, _off(c.a_align)),
             B=_store(B if c.transB else B.t(), c.ldb, _off(c.b_align)))
    v = A.double() @ B.double()
    if c.scale:
        s = rnd(c.N, seed=63).abs() + 0.5
        t["scale"] = _store(s[None], c.N, _off(c.scale_align))
        v = v * s.double()
    if c.shift:
        b = rnd(c.N, seed=64)
        t["shift"] = _store(b[None], c.N, _off(c.shift_align))
        v = v + b.double()
    if c.residual:
        r = rnd(c.M, c.N, seed=65)
        t["residual"] = _store(r, c.ldr, _off(c.r_align))
        v = v + r.double()
    v = {0: lambda x: x, 1: torch.relu, 2: torch.sigmoid, 3: torch.tanh}[c.act](v)
    C0 = rnd(c.M, c.N, seed=66) if c.accumulate else torch.full((c.M, c.N), float("nan"))
    if c.accumulate:
        v = v + C0.double()
    t["C"] = _store(C0, c.ldc, _off(c.c_align), GUARD_ROWS)
    sim = {k: b.clone() for k, b in t.items()}
    SIM.gemm(*_args(c, sim), **_epilogue(c, sim))
    return dict(t=t, ref=v, sim=_c_region(c, sim["C"]).clone())


def _view(c, t, name):
    if name not in t:
        return None
    return t[name][_off(getattr(c, {"A": "a_align", "B": "b_align", "C": "c_align", "residual": "r_align",
                                     "scale": "scale_align", "shift": "shift_align"}[name])):]


def _args(c, t):
    return (_view(c, t, "A"), c.lda, c.transA, _view(c, t, "B"), c.ldb, c.transB, _view(c, t, "C"), c.ldc,
            c.M, c.N, c.K)


def _epilogue(c, t):
    return dict(scale=_view(c, t, "scale"), shift=_view(c, t, "shift"), residual=_view(c, t, "residual"),
                ldr=c.ldr, act=c.act, accumulate=c.accumulate)


def _c_region(c, buf):
    return buf[_off(c.c_align):].as_strided((c.M, c.N), (c.ldc, 1))


def bounds_broken(y, ref, sim):
    """the two statistics of a result against the fp64 reference and the fp32 CPU contract ->
    (names of the bounds it breaks, rms, worst block, the contract's worst block)"""
    rms, blk = cr.err_stats(y, ref)
    _, blk32 = cr.err_stats(sim, ref)
    broken = []
    if not rms < RMS_BOUND:          # (NaN breaks both)
        broken.append("rms")
    if not blk <= BLOCK_FACTOR * blk32:
        broken.append("block")
    return broken, rms, blk, blk32


FIGURES = []   # (name, route, rms, worst block, fp32 contract's worst block) of every checked launch


def launch(hip, c, opts=None):
    """one vlnce_gemm of `c` under `opts`; asserts the route against the mirror and the guard band;
    returns (C [M, N] on the CPU, the record, the operands dict)"""
    opts = opts or {}
    op = operands(c)
    g = {k: b.to(DEV) for k, b in op["t"].items()}
    with hip.options(**opts):
        hip.gemm(*_args(c, g), **_epilogue(c, g))
        rec = hip.gemm_last_kernel()
    torch.cuda.synchronize()
    assert rec == gd.expected(c, **opts), (c, opts, "ran on", rec)
    out = g["C"].cpu()
    guard = torch.ones(out.numel(), dtype=torch.bool)
    _c_region(c, guard).fill_(False)
    assert int(guard.sum()) == out.numel() - c.M * c.N >= GUARD_ROWS * c.ldc
    same = out.view(torch.int32)[guard] == op["t"]["C"].view(torch.int32)[guard]
    assert bool(same.all()), (c, opts, "guard band written at flat offsets",
                              torch.nonzero(guard)[~same][:8].flatten().tolist())
    return _c_region(c, out).clone(), rec, op


def check(name, hip, c, opts=None):
    y, rec, op = launch(hip, c, opts)
    broken, rms, blk, blk32 = bounds_broken(y, op["ref"], op["sim"])
    FIGURES.append((name, rec, rms, blk, blk32))
    print(f"{name:28s} {rec.a}/{rec.b} {rec.tile[0]}x{rec.tile[1]} split {rec.splitk:2d} zero {int(rec.zero)} "
          f"pass2 {int(rec.pass2)}  rms {rms:.2e}  block {blk:.2e}  fp32 CPU block {blk32:.2e}")
    # measured on the MI355X (profiles/gemm_routes_errors.txt): unsplit launches rms 0.6e-7 .. 5.6e-7 --
    # one k-ordered chain per output: 1.4e-7 at K = 64, 2.9e-7 at K = 512, 5.6e-7 at K = 992 -- with the
    # worst block at most 2.37 x the fp32 CPU contract's (K = 992; 1.96 x at K = 512, 1.2 x at K <= 64);
    # split launches rms 0.7e-7 .. 3.3e-7, worst block at most 1.37 x (K = 1024 in three ranges)
    assert not broken, (name, c, opts, rec, broken, rms, blk, blk32)
    return rec


# ------------------------------------------------------------------ one launch per table row
# (that the table lists every reachable instantiation, and that the mirror puts each row where the
# table says, needs no GPU: tests/test_gemm_routes_host.py)
@pytest.mark.parametrize("row", ROUTES + FOLDS + EDGES, ids=[r.name for r in ROUTES + FOLDS + EDGES])
def test_gemm_route_against_fp64(hip, row):
    rec = check(row.name, hip, row.call, row.opts)
    assert rec == want_kernel(row), (row, rec)


# ------------------------------------------------------------------ operand and epilogue matrix
BASES = [("buf", Call(70, 52, 64, ldc=56)), ("scalar", Call(70, 52, 50, ldc=56)),
         ("split", Call(70, 52, 512, ldc=56))]


def cells(base):
    """(name, call) per cell: the base route's call with one epilogue / storage form each"""
    out = [(f"act{a}+shift", base._replace(shift=True, act=a)) for a in range(4)]
    out += [("scale+shift", base._replace(scale=True, shift=True)),
            ("scale+shift+tanh", base._replace(scale=True, shift=True, act=3)),
            ("residual-ldr=ldc", base._replace(residual=True, ldr=base.ldc, act=1)),
            ("residual-ldr=N", base._replace(residual=True, ldr=base.N)),               # still 16-byte rows
            ("residual-ldr=N+1", base._replace(residual=True, ldr=base.N + 1)),         # scalar epilogue
            ("residual+1float", base._replace(residual=True, ldr=base.ldc, r_align=4)),  # scalar epilogue
            ("accumulate", base._replace(accumulate=1)),
            ("accumulate+shift", base._replace(accumulate=1, shift=True)),
            ("accumulate+relu+shift", base._replace(accumulate=1, act=1, shift=True)),
            ("ldc=N+1", base._replace(ldc=base.N + 1, shift=True, act=1)),               # scalar epilogue
            ("C+1float", base._replace(c_align=4, shift=True, act=1)),                   # scalar epilogue
            ("C+1float-accumulate", base._replace(c_align=4, accumulate=1))]
    return out


MATRIX = [(f"{bn}-{cn}", c) for bn, b in BASES for cn, c in cells(b)]


@pytest.mark.parametrize("name,c", MATRIX, ids=[n for n, _ in MATRIX])
def test_gemm_epilogue_matrix_against_fp64(hip, name, c):
    check(name, hip, c)


def test_gemm_refusals_launch_nothing(hip):
    """the calls vlnce_gemm refuses: an error, C untouched (also where the shape would have split and
    zero-filled), the record left as it was.  The bias-alignment contract of include/vlnce_hip.h: scale
    and shift must be 16-byte aligned on every route."""
    ok = Call(70, 52, 64, ldc=56)
    launch(hip, ok)
    before = hip.gemm_last_kernel()
    refused = [Call(70, 52, 64, ldc=56, shift=True, shift_align=4),
               Call(70, 52, 512, ldc=56, shift=True, act=1, shift_align=4),          # would split
               Call(70, 52, 50, ldc=56, scale=True, shift=True, scale_align=4),      # scalar loaders
               Call(70, 52, 512, 0, 1, ldc=56, b_align=4),                           # B_KN, would split
               Call(72, 52, 512, 1, 1, ldc=56, a_align=4),
               Call(72, 52, 64, 1, 0, lda=72, ldc=56)]                               # transA without transB
    for c in refused:
        with pytest.raises(gd.Refused):
            gd.expected(c)
        op = operands(c)
        g = {k: b.to(DEV) for k, b in op["t"].items()}
        with pytest.raises(RuntimeError, match="vlnce_gemm failed"):
            hip.gemm(*_args(c, g), **_epilogue(c, g))
        torch.cuda.synchronize()
        assert hip.gemm_last_kernel() == before, c
        assert torch.equal(g["C"].cpu().view(torch.int32), op["t"]["C"].view(torch.int32)), c
    # the same bias 16-byte aligned runs
    check("refusal-counterpart", hip, refused[1]._replace(shift_align=16))


# ------------------------------------------------------------------ split-K: order of the atomic adds
def test_split_k_runs_each_meet_the_bounds(hip):
    """the K ranges are added atomically in an order that varies: no bit identity; each of two runs
    meets the bounds, and C += A B on a known C comes back as that matrix plus the product"""
    for name, c in (("buf-split8", Call(70, 52, 512, ldc=56)), ("v4-kn-split8", Call(70, 50, 512, 0, 1, ldc=54)),
                    ("trans-split8", Call(70, 52, 512, 1, 1, ldc=56))):
        for run in (1, 2):
            rec = check(f"{name}-run{run}", hip, c)
            assert rec.splitk == 8 and rec.zero
        rec = check(f"{name}-accumulate", hip, c._replace(accumulate=1))
        assert rec.splitk == 8 and not rec.zero and not rec.pass2


# ------------------------------------------------------------------ the callers' routing (ops.py)
class GemmCalls:
    """wraps HipLib.gemm: the record is read inside the call, on the thread that made it (autograd's
    backward runs on another one), with what the mirror says of the same arguments and copies of the
    operands for an fp64 product (the record is read before the copies: a copy launches nothing of
    vlnce_gemm's, the record is host state)"""

    def __init__(self, hip, monkeypatch):
        self.calls = []
        inner = hip.gemm

        def gemm(A, lda, transA, B, ldb, transB, Cm, ldc, M, N, K, scale=None, shift=None, residual=None,
                 ldr=0, act=0, accumulate=0):
            def al(t):
                return 16 if t.data_ptr() % 16 == 0 else 4
            c = Call(M, N, K, transA, transB, lda, ldb, ldc, al(A), al(B), al(Cm), scale is not None,
                     shift is not None, residual is not None, ldr or ldc, 16 if residual is None else al(residual),
                     accumulate, act)
            a = A.as_strided((K, M) if transA else (M, K), (lda, 1)).cpu()
            b = B.as_strided((K, N) if transB else (N, K), (ldb, 1)).cpu()
            a, b = (a.t() if transA else a), (b if transB else b.t())
            c0 = Cm.as_strided((M, N), (ldc, 1)).cpu() if accumulate else None
            inner(A, lda, transA, B, ldb, transB, Cm, ldc, M, N, K, scale=scale, shift=shift,
                  residual=residual, ldr=ldr, act=act, accumulate=accumulate)
            self.calls.append(dict(call=c, rec=hip.gemm_last_kernel(), want=gd.expected(c), a=a, b=b, c0=c0,
                                   out=Cm.as_strided((M, N), (ldc, 1)).cpu()))

        monkeypatch.setattr(hip, "gemm", gemm)

    def take(self):
        got, self.calls = self.calls, []
        for g in got:
            assert g["rec"] == g["want"], (g["call"], g["rec"], g["want"])
        return got


def _fp64_ok(name, got, ref, ref32):
    broken, rms, blk, blk32 = bounds_broken(got, ref, ref32)
    print(f"{name:28s} rms {rms:.2e}  block {blk:.2e}  fp32 CPU block {blk32:.2e}")
    FIGURES.append((name, None, rms, blk, blk32))
    assert not broken, (name, broken, rms, blk, blk32)


def test_linear_at_64_rows_long_reduction(hip, monkeypatch):
    """ops.linear at one row per environment with K > 2048: forward on the general GEMM (split-K +
    second pass), the whole backward on the skinny kernel (no vlnce_gemm at all)"""
    calls = GemmCalls(hip, monkeypatch)
    M, K, N = 64, 2112, 256
    x, w, b, gy = rnd(M, K, seed=71), rnd(N, K, seed=72, scale=K ** -0.5), rnd(N, seed=73), rnd(M, N, seed=74)
    xd, wd, bd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    y = ops.linear(xd, wd, bd, act=ops.ACT_RELU)
    (fwd,) = calls.take()
    assert fwd["rec"] == GemmKernel("buf", "buf", T64, 33, True, True), fwd["rec"]
    dx, dw, db = torch.autograd.grad(y, (xd, wd, bd), gy.to(DEV))
    torch.cuda.synchronize()
    assert calls.take() == []
    pre = x.double() @ w.double().t() + b.double()
    _fp64_ok("linear64-forward", y, torch.relu(pre), torch.relu(x @ w.t() + b))
    # (the knife edge of the ReLU: the backward kernel takes act'(y) from the y the forward stored)
    dz32 = gy * (y.detach().cpu() > 0)
    _fp64_ok("linear64-dx", dx, dz32.double() @ w.double(), dz32 @ w)
    _fp64_ok("linear64-dw", dw, dz32.double().t() @ x.double(), dz32.t() @ x)


def test_linear_past_the_skinny_kernels(hip, monkeypatch):
    """ops.linear at M = 200: forward A_BUF, dX on B_KN, dW on A_TRANS; and dx_from = c0: C a column
    window of dx, accumulate = 1, the leading columns zero"""
    calls = GemmCalls(hip, monkeypatch)
    M, K, N, c0 = 200, 96, 80, 32
    x, w, b, gy = rnd(M, K, seed=75), rnd(N, K, seed=76, scale=K ** -0.5), rnd(N, seed=77), rnd(M, N, seed=78)
    xd, wd, bd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    y = ops.linear(xd, wd, bd)
    (fwd,) = calls.take()
    assert fwd["rec"] == GemmKernel("buf", "buf", T64, 1, False, False)
    _fp64_ok("linear200-forward", y, x.double() @ w.double().t() + b.double(), x @ w.t() + b)
    dx, dw, db = torch.autograd.grad(y, (xd, wd, bd), gy.to(DEV))
    torch.cuda.synchronize()
    gx, gw = calls.take()
    assert gx["rec"] == GemmKernel("v4", "kn", T64, 1, False, False), gx["rec"]
    assert gw["rec"] == GemmKernel("trans", "kn", T64, 1, False, False), gw["rec"]
    _fp64_ok("linear200-dx", dx, gy.double() @ w.double(), gy @ w)
    _fp64_ok("linear200-dw", dw, gy.double().t() @ x.double(), gy.t() @ x)
    # dx_from: only the trailing columns' gradient
    y = ops.linear(xd, wd, bd, dx_from=c0)
    calls.take()
    (dx,) = torch.autograd.grad(y, (xd,), gy.to(DEV))
    torch.cuda.synchronize()
    (gx,) = [g for g in calls.take() if g["call"].accumulate]
    assert gx["call"] == Call(M, K - c0, N, 0, 1, lda=N, ldb=K, ldc=K, accumulate=1), gx["call"]
    assert gx["rec"] == GemmKernel("v4", "kn", T64, 1, False, False), gx["rec"]
    assert float(dx[:, :c0].abs().max()) == 0.0
    _fp64_ok("linear200-dx_from", dx[:, c0:], gy.double() @ w.double()[:, c0:], gy @ w[:, c0:])


def test_rollout_fallback_recurrent_dgrad(hip, monkeypatch):
    """the step-by-step fallback of ops.MaskedRNNSeqFn (a GRU at N = 5, H = 512, the one-launch rollout
    and the fused step switched off): dh += dgates W_hh is split with accumulate -- no zero-fill --
    and comes back as the C it found plus the product"""
    monkeypatch.setattr(hip, "gru_rollout_supported", lambda N, H: False)
    monkeypatch.setattr(hip, "rnn_step_supported", lambda N, H, lstm: False)
    calls = GemmCalls(hip, monkeypatch)
    T, N, H = 2, 5, 512
    gi = rnd(T * N, 3 * H, seed=81).to(DEV).requires_grad_()
    h0 = rnd(N, H, seed=82).to(DEV).requires_grad_()
    w_hh = rnd(3 * H, H, seed=83, scale=H ** -0.5).to(DEV).requires_grad_()
    b_hh = rnd(3 * H, seed=84).to(DEV).requires_grad_()
    mask = torch.ones(T * N, dtype=torch.uint8, device=DEV)
    y, hT, _ = ops.MaskedRNNSeqFn.apply(False, gi, h0, None, mask, w_hh, b_hh)
    fwd = calls.take()
    assert [g["rec"] for g in fwd] == [GemmKernel("buf", "buf", T64, 8, True, True)] * T, fwd[0]["rec"]
    torch.autograd.grad(y, (gi, h0, w_hh), rnd(T * N, H, seed=85).to(DEV))
    torch.cuda.synchronize()
    bwd = calls.take()
    steps = [g for g in bwd if g["call"].accumulate]
    assert len(steps) == T
    for i, g in enumerate(steps):
        assert g["call"] == Call(N, H, 3 * H, 0, 1, accumulate=1), g["call"]
        assert g["rec"] == GemmKernel("v4", "kn", T64, 24, False, False), g["rec"]
        ref = g["c0"].double() + g["a"].double() @ g["b"].double()
        ref32 = g["c0"] + g["a"] @ g["b"]
        _fp64_ok(f"rollout-dh-step{i}", g["out"], ref, ref32)
    (dw,) = [g for g in bwd if g["call"].transA]
    assert dw["rec"].a == "trans" and dw["rec"].splitk == 1, dw["rec"]
