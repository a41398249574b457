"""The dispatch of vlnce_gemm written out a second time, in Python, from reading vlnce_gemm,
choose_splitk, choose_tile and dispatch_tiles / dispatch_small (csrc/igemm.hip), buf_ok (igemm_shared.h): which
igemm_kernel instance a call must land on and what runs around it, as the GemmKernel tuple that
HipLib.gemm_last_kernel() decodes.  The GPU tests compare the two after every launch, so a changed
split threshold, a changed eligibility rule of the buffer loaders or a changed alignment test fails a
test instead of moving a case to another kernel unnoticed.

Unlike the convolution table (tests/conv_dispatch.py) nothing here depends on the CU count: the
split and tile rules use the shape alone (choose_tile wants 512 tiles, choose_splitk 256 / 1024
workgroups, both constants), so the table holds on any device.

Not a test module and not part of the product."""
import collections

from vlnce_amd._lib import GemmKernel

BK = 32
DEFAULTS = dict(igemm_tile=0, igemm_nobuf=0, igemm_no_splitk=0)
TILES = {1: (128, 128), 2: (128, 64), 3: (64, 64)}      # option "igemm_tile"'s numbering
INT_MAX = 0x7FFFFFFF


class Refused(Exception):
    """vlnce_gemm returns an error for this call and launches nothing"""


_Call = collections.namedtuple(
    "Call", "M N K transA transB lda ldb ldc a_align b_align c_align scale shift residual ldr r_align "
            "accumulate act scale_align shift_align")


class Call(_Call):
    """one vlnce_gemm: the shape, the storage of the operands (row strides in floats, alignment of the
    base pointers in bytes: 16 or 4) and which epilogue operands it carries.  Strides default to the
    contiguous ones of the stored matrices: A [M,K] ([K,M] with transA), B [N,K] ([K,N] with transB)."""
    __slots__ = ()

    def __new__(cls, M, N, K, transA=0, transB=0, lda=None, ldb=None, ldc=None, a_align=16, b_align=16,
                c_align=16, scale=False, shift=False, residual=False, ldr=None, r_align=16, accumulate=0,
                act=0, scale_align=16, shift_align=16):
        lda = (M if transA else K) if lda is None else lda
        ldb = (N if transB else K) if ldb is None else ldb
        ldc = N if ldc is None else ldc
        ldr = ldc if ldr is None else ldr
        return super().__new__(cls, M, N, K, int(transA), int(transB), lda, ldb, ldc, a_align, b_align,
                               c_align, bool(scale), bool(shift), bool(residual), ldr, r_align,
                               int(accumulate), int(act), scale_align, shift_align)


def _cdiv(a, b):
    return -(-a // b)


def choose_splitk(M, N, K, long_reduction_form, no_splitk=0):
    """choose_splitk: the ordinary rule (fewer than 128 tiles of 64 x 64, at least 8 K-tiles: towards 256
    workgroups, at least two K-tiles each, at most 64 ranges) and transA's rule for a long reduction
    (KT >= 32 and 128 <= tiles < 1024: towards 1024 workgroups, at least four K-tiles each)"""
    if no_splitk:
        return 1
    tiles = _cdiv(M, 64) * _cdiv(N, 64)
    KT = _cdiv(K, BK)
    if long_reduction_form and KT >= 32 and 128 <= tiles < 1024:
        s = min(_cdiv(1024, tiles), KT // 4)
        return 1 if s < 2 else s
    if tiles >= 128 or KT < 8:
        return 1
    s = min(_cdiv(256, tiles), KT // 2, 64)
    return 1 if s < 2 else s


def choose_tile(M, N, force=0):
    """choose_tile: a forced tile, else the biggest that still gives 512 workgroups; 64 x 64 whenever
    M <= 64 or N <= 64"""
    if force in TILES:
        return TILES[force]
    for bm, bn in ((128, 128), (128, 64)):
        if N > 64 and M > 64 and _cdiv(M, bm) * _cdiv(N, bn) >= 512:
            return (bm, bn)
    return (64, 64)


def buf_ok(c, nobuf=0):
    """buf_ok for the 1 x 1 'convolution' a GEMM is (Cin = K, one tap, no padding)"""
    a_bytes = ((c.M - 1) * c.lda + c.K) * 4
    b_bytes = ((c.N - 1) * c.ldb + c.K) * 4
    return (not nobuf and c.K % 32 == 0 and c.lda % 4 == 0 and c.ldb % 4 == 0
            and a_bytes < INT_MAX and b_bytes < INT_MAX)


def plain(c):
    """may the reduction be split: no scale, no residual, and not C += act(...)"""
    return not c.scale and not c.residual and not (c.accumulate and c.act)


def epilogue_is_vectorised(c):
    """igemm_kernel's vec_out (an unsplit launch): 16-byte stores of four columns.  The record does not
    tell the two epilogues apart; the tests use this to see that they cover both."""
    return (c.N % 4 == 0 and c.ldc % 4 == 0 and c.c_align == 16
            and (not c.residual or (c.ldr % 4 == 0 and c.r_align == 16)))


def expected(c, **options):
    """the GemmKernel the call must land on; raises Refused where vlnce_gemm returns an error"""
    o = dict(DEFAULTS, **options)
    if c.M <= 0 or c.N <= 0 or c.K <= 0:
        raise Refused("bad shape")
    if (c.scale and c.scale_align != 16) or (c.shift and c.shift_align != 16):
        raise Refused("scale / shift must be 16-byte aligned")
    if c.transA and not c.transB:
        raise Refused("transA requires transB")
    if c.transB and c.b_align != 16:
        raise Refused("B must be 16-byte aligned")
    if c.transA and c.a_align != 16:
        raise Refused("operands must be 16-byte aligned")
    if c.M >= 32767 * 1024:
        raise Refused("M too large")
    split = choose_splitk(c.M, c.N, c.K, bool(c.transA), o["igemm_no_splitk"]) if plain(c) else 1
    zero = split > 1 and not c.accumulate
    pass2 = split > 1 and (c.shift or c.act != 0)
    tile = (64, 64) if split > 1 else choose_tile(c.M, c.N, o["igemm_tile"])
    if c.transA:
        return GemmKernel("trans", "kn", tile, split, zero, pass2)
    av4 = c.K % 4 == 0 and c.lda % 4 == 0 and c.a_align == 16
    if c.transB:
        if av4:
            return GemmKernel("v4", "kn", tile, split, zero, pass2)
        return GemmKernel("s", "kn", (64, 64), split, zero, pass2)
    bv4 = c.K % 4 == 0 and c.ldb % 4 == 0 and c.b_align == 16
    if av4 and bv4 and buf_ok(c, o["igemm_nobuf"]):
        return GemmKernel("buf", "buf", tile, split, zero, pass2)
    if av4 and bv4:
        return GemmKernel("v4", "nk_v4", tile, split, zero, pass2)
    return GemmKernel("s", "nk_s", (64, 64), split, zero, pass2)


def reachable():
    """every (A loader, B loader, tile, split or not) vlnce_gemm instantiates and can reach: the pairs
    with a 16-byte A loader take dispatch_tiles (three tiles) when the reduction is not split, every
    split launch and both scalar-A pairs take dispatch_small (64 x 64)"""
    out = set()
    for a, b in (("buf", "buf"), ("v4", "nk_v4"), ("v4", "kn"), ("trans", "kn")):
        out |= {(a, b, t, False) for t in TILES.values()}
        out.add((a, b, (64, 64), True))
    for a, b in (("s", "nk_s"), ("s", "kn")):
        out |= {(a, b, (64, 64), False), (a, b, (64, 64), True)}
    return out
