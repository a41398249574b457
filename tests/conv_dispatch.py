"""The convolution dispatch of vlnce_conv2d_fwd written out a second time, in Python, from reading
vlnce_conv2d_fwd / choose_splitk (igemm.hip), p3_try_launch_ (conv_p3.hip), m3_try_launch (conv_m3.hip)
and x3_plan (conv_x3.hip): which kernel INSTANCE a launch must land on, as the ConvKernel tuple that
HipLib.conv2d_last_kernel() decodes.  The GPU tests compare the two after every launch, so a changed
eligibility rule, a forced tile that silently does not fit or an instance nothing reaches any more
fails a test instead of moving a case to another kernel unnoticed.

The rules depend on the CU count and the LDS a workgroup may ask for; the defaults are the MI355X's
(256 CUs, 160 KB).  Not a test module and not part of the product."""
from vlnce_amd._lib import ConvKernel

CUS, LDS_MAX = 256, 163840
U3_MAX_CIN, P3_MAX_ROWS, BK = 4096, 384, 32
PLANE_ROW = {1: 208, 2: 144}          # Planes<MATH>::ROW (igemm_shared.h)
DEFAULTS = dict(conv_math=2, p3=2, p3_tile=0, s3=1, u3=1, u3_waves=8, x3_tile=0, m3=1,
                igemm_no_splitk=0, igemm_nobuf=0)
P3_TILES = ((128, 256), (64, 256), (256, 128), (128, 128), (256, 64), (128, 64))
X3_TILES = ((128, 128), (64, 128), (128, 64), (64, 64))


def _cdiv(a, b):
    return -(-a // b)


def _eff(tiles, cus):
    return tiles / (_cdiv(tiles, cus) * cus)


class Launch:
    """one vlnce_conv2d_fwd: the geometry and which optional operands it carries.  Contiguous
    operands (ldx = Cin, ldy = ldr = Cout), 16-byte aligned, as every test here passes them."""

    def __init__(self, N, H, W, Cin, Cout, k, stride, pad, *, prologue=False, dual=None, residual=False,
                 scale=False, shift=None, act=0, stats=False, bn=False):
        self.N, self.H, self.W, self.Cin, self.Cout = N, H, W, Cin, Cout
        self.k, self.stride, self.pad = k, stride, pad
        self.Ho = (H + 2 * pad - k) // stride + 1
        self.Wo = (W + 2 * pad - k) // stride + 1
        self.M, self.K = N * self.Ho * self.Wo, k * k * Cin
        self.prologue = bool(prologue or dual)
        self.dual = dual            # None | "identity" | "bn"
        self.residual, self.scale = bool(residual), bool(scale)
        self.shift = self.scale if shift is None else bool(shift)
        self.act, self.stats, self.bn = act, bool(stats), bool(bn)
        self.stat_rows = 32 if (self.Ho * self.Wo) % 32 == 0 else 16

    @classmethod
    def of_case(cls, case, stats=False):
        """a row of CONV_CASES / P3_CASES as test_conv2d_fwd launches it (its first launch: no
        statistics; `stats`: the second one, ops.conv2d_nhwc(want_stats=True) of the bare operands)"""
        name, N, H, W, Cin, Cout, k, s, p, ex = case
        if stats:
            return cls(N, H, W, Cin, Cout, k, s, p, stats=True)
        return cls(N, H, W, Cin, Cout, k, s, p, prologue=ex.get("prologue"), dual=ex.get("dual"),
                   residual=ex.get("residual"), scale=ex.get("scale"), act=1 if ex.get("relu") else 0)


def _f32(kernel, a=0):
    return ConvKernel("f32", kernel, 0, a, 0, 0)


def _splitk(L, o):
    """choose_splitk() behind the conditions of vlnce_conv2d_fwd (accumulate = 0, ldc = N)"""
    if not ((L.scale and L.shift) or (not L.scale and not L.residual)) or o["igemm_no_splitk"]:
        return 1
    tiles, KT = _cdiv(L.M, 64) * _cdiv(L.Cout, 64), _cdiv(L.K, BK)
    if tiles >= 128 or KT < 8:
        return 1
    s = min(_cdiv(256, tiles), KT // 2, 64)
    return 1 if s < 2 else s


def _m3(L, o, fmt, cus):
    mode = o["m3"]
    if not mode or L.Cin % 32 or L.Cout % 32 or L.dual or L.Cin > 2048:
        return None
    if L.residual and (L.stats or L.bn):
        return None
    KS, M, N = L.K // 16, L.M, L.Cout
    if mode == 1 and (M * N > 4 * 1024 * 1024 + 1 or 2.0 * M * N * L.K > 2.6e9 or L.K > 4608):
        return None
    wide = N % 64 == 0

    def m3(nt, ksplit, rb):
        return ConvKernel("m3", "conv_m3", fmt, nt, ksplit, rb)
    if _cdiv(M, 128) * (N // (64 if wide else 32)) >= cus or KS < 8:
        return m3(2 if wide else 1, 1, 4)
    if mode == 3 and wide:
        return m3(2, 4, 2)
    nt2 = wide and _cdiv(M, 32) * (N // 64) >= cus
    if KS >= 128 and not nt2 and _cdiv(M, 32) * (N // (64 if nt2 else 32)) <= cus:
        return m3(1, 8, 1)
    return m3(2 if nt2 else 1, 4, 1)


def p3_rows(L, bm, dense):
    """p3_rows_for(): patch rows of the BM-pixel tiles, rounded up to whole 32-row passes"""
    if not dense:
        return bm
    Hp, Wp, howo = L.H + 2 * L.pad, L.W + 2 * L.pad, L.Ho * L.Wo

    def u0(m):
        img, rem = divmod(m, howo)
        ho = rem // L.Wo
        return (img * Hp + ho) * Wp + (rem - ho * L.Wo)
    rows, m0 = 0, 0
    while m0 < L.M:
        if m0 > 0 and m0 % howo == 0:
            break
        mlast = min(m0 + bm, L.M) - 1
        rows = max(rows, u0(mlast) - u0(m0) + (L.k - 1) * Wp + L.k)
        m0 += bm
    return (rows + 31) // 32 * 32


def p3_tile_fits(L, fmt, tile):
    """does tile 1..6 of conv_p3_kernel fit the LDS (and the producers' row groups) for this launch"""
    dense = not (L.k == 1 and L.pad == 0)
    bm, bn = P3_TILES[tile - 1]
    rows = p3_rows(L, bm, dense)
    need = 2 * rows * PLANE_ROW[fmt] + (3 * L.Cin * 4 if dense else 2 * bn * 192) + 16
    return need <= LDS_MAX and not (dense and rows > P3_MAX_ROWS)


def p3_eligible(L):
    """what p3_try_launch_ asks of every launch before it looks at the kernel options"""
    one = L.k == 1 and L.pad == 0
    if L.Cin % 32 or L.Cout % 32 or (L.residual and (L.stats or L.bn)):
        return False
    if not one and L.stride != 1:
        return False
    return not (L.dual and not (one and L.stride == 1))


def s3_eligible(L):
    """the documented conv_s3 rule (without the CU-fill condition of option "s3" = 1)"""
    return (p3_eligible(L) and L.k == 1 and L.pad == 0 and not L.dual and not L.residual
            and L.stride == 1 and L.Cin in (64, 128) and L.Cout % 256 == 0 and L.Cout // 256 <= 8
            and (not L.stats or L.stat_rows == 32) and L.act in (0, 1))


def _p3(L, o, fmt, cus):
    if not o["p3"] or not p3_eligible(L):
        return None
    one = L.k == 1 and L.pad == 0
    dense = not one
    M, N = L.M, L.Cout
    if s3_eligible(L) and o["s3"] and (o["s3"] == 2 or _cdiv(M, 64) * (N // 256) >= 4 * cus):
        return ConvKernel("p3", "conv_s3", fmt, L.Cin, 0, 0)
    u3 = o["u3"]
    if one and u3 and N >= 256 and L.Cin <= U3_MAX_CIN:
        def eff(bm):
            return _eff(_cdiv(M, bm) * _cdiv(N, 256), cus)
        bm = 64 if u3 == 2 else 128
        if u3 == 1 and eff(128) < 0.8 and L.K >= 512 and eff(64) >= 0.8:
            bm = 64
        if eff(bm) >= 0.8 or u3 >= 2:
            kind = 0 if not L.dual else (2 if L.dual == "bn" else 1)
            waves = 4 if o["u3_waves"] == 4 else 8
            return ConvKernel("p3", "conv_u3", fmt, 64 if waves == 4 else bm, kind, waves)
    if (o["p3"] == 2 and one) or (o["p3"] == 3 and dense):
        return None
    force = o["p3_tile"]
    forced = 1 <= force <= 6
    bn = 64 if N <= 64 else 128 if N <= 128 else 256
    if one and bn == 64 and not forced:
        return None
    pick, best = 0, 0.0
    for ci, (cbm, cbn) in enumerate(P3_TILES):
        if (ci != force - 1) if forced else (cbn > bn):
            continue
        if not p3_tile_fits(L, fmt, ci + 1):
            continue
        e = _eff(_cdiv(M, cbm) * _cdiv(N, cbn), cus)
        if e > best:
            best, pick = e, ci + 1
        if e >= 0.8:
            break
    if not pick or (best < 0.4 and not forced):
        return None
    return ConvKernel("p3", "conv_p3", fmt, pick, "dual" if L.dual else "dense" if dense else "gather", 0)


def _x3(L, o, fmt, cus):
    if L.Cin % 32 or (L.residual and (L.stats or L.bn)):
        return None
    force = o["x3_tile"]

    def x3(tile):
        return ConvKernel("x3", "conv_x3", fmt, tile, 1 if L.dual else 0, 0)
    if 1 <= force <= 4:
        return x3(force)
    pick, best = 0, 0.0
    for ci, (bm, bn) in enumerate(X3_TILES):
        if bn == 128 and L.Cout <= 64:
            continue
        e = _eff(_cdiv(L.M, bm) * _cdiv(L.Cout, bn), cus)
        if e >= 0.8:
            return x3(ci + 1)
        if e > best:
            best, pick = e, ci + 1
    return x3(pick) if best >= 0.4 else None


def reaches_plane_kernels(L, **opts):
    """does the launch get as far as the plane kernels' routers (conv_m3 aside): operands the buffer
    loaders cover, and no split-K first"""
    o = dict(DEFAULTS, **opts)
    ok = L.Cin % 32 == 0 and L.k * L.k <= 32 and not o["igemm_nobuf"]
    return ok and (bool(L.dual) or _splitk(L, o) == 1)


def expected(L, fmt=None, cus=CUS, **opts):
    """the ConvKernel a launch `L` must run on under the dispatch options `opts` (the others at their
    defaults) in plane format `fmt` (default: option "conv_math")"""
    o = dict(DEFAULTS, **opts)
    planes = o["conv_math"] != 0
    fmt = fmt or (2 if o["conv_math"] == 2 else 1)
    v4 = L.Cin % 4 == 0
    buf_ok = not o["igemm_nobuf"] and L.Cin % 32 == 0 and L.k * L.k <= 32
    if L.dual:
        hit = planes and (_p3(L, o, fmt, cus) or _x3(L, o, fmt, cus))
        return hit or _f32("dual")
    if v4 and buf_ok:
        hit = planes and _m3(L, o, fmt, cus)
        if hit:
            return hit
        sk = _splitk(L, o)
        if sk > 1:
            return _f32("splitk", sk)
        hit = planes and (_p3(L, o, fmt, cus) or _x3(L, o, fmt, cus))
        return hit or _f32("buf")
    if v4:
        return _f32("v4")
    if L.k == 7 and L.Cin in (3, 1):
        return _f32("stem3" if L.Cin == 3 else "stem1")
    return _f32("s")
