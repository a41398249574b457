"""GPU tier: vlnce_bn_bwd / vlnce_gn_bwd called WITH the `pow2` output (csrc/bwd.hip: the maxima
reductions, tops_partial, the bound pass, block 0 of the apply kernels) against an fp64 restatement
of the formulas in include/vlnce_hip.h:

* dx, dgamma, dbeta, dres to 2e-4 of the output scale (the tolerance of test_bn_bwd / test_gn_bwd),
  and bit-identical to the same call without `pow2` -- the scale is an extra output;
* pow2[0] = P copies of one exact power of two 2^k, pow2[1] its exact inverse;
* max|dx| * 2^k <= 2^14 (what the fp16 planes of the data-gradient convolution and of
  wgrad_x6<.., MATH_F16X3> rely on), and 2^k is the one the documented bound gives:
    BN  max_c |gamma rstd| (max|g| + |dbeta|/M + max|x - mean| |rstd dgamma|/M)
    GN  max_{n,c} |rstd| (max|g| |gamma| + |s1|/cnt + max|x - mean| |rstd s2|/cnt),  cnt = HW * C/groups
  with g = dy [y > 0], the maxima per channel (GN: per sample and channel) -- so a maximum lost in a
  tail loop or a partial chunk shows as a 2^k one binade too large even where dx still fits.

Shapes: quads of channels that span two groups (cpg = 3), odd N*groups (the 16-byte alignment of
the workspace segments), one- and two-pixel last chunks (HW = 129, 130), one strip / several strips
of channel quads, one slice / several slices of rows."""
import functools
import math

import pytest
import torch

from vlnce_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-4     # of the output scale: test_bn_bwd / test_gn_bwd


@pytest.fixture(scope="module")
def hip():
    return _lib.get_lib()


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(hash((shape, seed)) & 0x7FFFFFFF)
    return torch.randn(*shape, generator=g)


def close(got, ref, what):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    print(f"{what}: max|d|={err:.3e} scale={scale:.3e}")
    assert err <= TOL * scale, f"{what}: max|d|={err:.3e} scale={scale:.3e}"


def check_pow2(pow2, bound, dx_ref, what):
    """shape of the scale, safety, and the documented rule; returns 2^k"""
    up, down = pow2[0].cpu().double(), pow2[1].cpu().double()
    assert bool((up == up[0]).all()) and bool((down == down[0]).all()), what
    u, d = float(up[0]), float(down[0])
    assert math.frexp(u)[0] == 0.5 and u * d == 1.0, (what, u, d)     # an exact power of two, its inverse
    top = float(dx_ref.abs().max())
    if bound > 0:
        e = math.frexp(bound)[1]
        want = 2.0 ** (14 - e)
    else:
        want = 1.0
    print(f"{what}: P={pow2.size(1)} 2^k=2^{math.frexp(u)[1] - 1} bound={bound:.6e} "
          f"rule 2^{math.frexp(want)[1] - 1} max|dx|*2^k={top * u:.1f}")
    assert top * u <= 2.0 ** 14, (what, top, u)
    if u != want:
        # the kernel sums in fp32 and multiplies its bound by 1.0001: next to a power of two it may
        # land in the neighbouring binade
        m = math.frexp(bound)[0] if bound > 0 else 0.0
        near = bound > 0 and (m >= 1.0 / (1.0 + 1e-3) or m <= 0.5 * (1.0 + 1e-3))
        assert near and u in (want * 0.5, want * 2.0), (what, u, want, bound)
    return u


def dev(t):
    return {k: (v.to(DEV) if v is not None else None) for k, v in t.items()}


# ------------------------------------------------------------------ BatchNorm
@functools.lru_cache(maxsize=None)
def bn_inputs(M, Cc, relu):
    x = rnd(M, Cc, seed=1) * 2 + 0.5
    mean = x.mean(0)
    rstd = torch.rsqrt(x.var(0, unbiased=False) + 1e-5)
    gamma = rnd(Cc, seed=2).abs() + 0.5
    y = (x - mean) * rstd * gamma + rnd(Cc, seed=3)
    if relu:
        y = torch.relu(y)
    return dict(dy=rnd(M, Cc, seed=4), y=y, x=x, mean=mean, rstd=rstd, gamma=gamma)


def bn_reference(t, relu, batch):
    """fp64, from the fp32 operands the kernel is given: (dx, dgamma, dbeta, dres, bound)"""
    d = {k: v.double() for k, v in t.items()}
    M = d["dy"].shape[0]
    g = d["dy"] * (d["y"] > 0) if relu else d["dy"]
    xc = d["x"] - d["mean"]
    xh = xc * d["rstd"]
    db, dg = g.sum(0), (g * xh).sum(0)
    k = d["gamma"] * d["rstd"]
    dx = k * (g - db / M - xh * dg / M) if batch else k * g
    b = g.abs().amax(0)
    if batch:
        b = b + db.abs() / M + xc.abs().amax(0) * (d["rstd"] * dg).abs() / M
    return dx, dg, db, g, float((k.abs() * b).max())


def bn_run(hip, t, relu, batch, res, P):
    M, Cc = t["dy"].shape
    g = dev(t)
    out = dict(dx=torch.zeros(M, Cc, device=DEV), dres=torch.zeros(M, Cc, device=DEV) if res else None,
               dgamma=torch.zeros(Cc, device=DEV), dbeta=torch.zeros(Cc, device=DEV))
    pow2 = torch.zeros(2, P, device=DEV) if P else None
    ws = torch.empty(max(hip.bn_bwd_workspace_floats(M, Cc), 1), device=DEV)
    hip.bn_bwd(g["dy"], g["y"], g["x"], g["mean"], g["rstd"], g["gamma"], M, Cc, relu, batch,
               out["dx"], out["dres"], out["dgamma"], out["dbeta"], ws, pow2)
    torch.cuda.synchronize()
    return out, pow2


def bn_check(hip, t, relu, batch, res, what, Ps=(7, 300)):
    dx, dg, db, g, bound = bn_reference(t, relu, batch)
    ref = dict(dx=dx, dgamma=dg, dbeta=db, dres=g)
    keys = ("dx", "dgamma", "dbeta") + (("dres",) if res else ())
    plain, _ = bn_run(hip, t, relu, batch, res, 0)
    ups = []
    for P in Ps:    # the fill loop of 256 threads: a tail, and more than one pass
        out, pow2 = bn_run(hip, t, relu, batch, res, P)
        for k in keys:
            close(out[k], ref[k], f"{what}/P={P}/{k}")
            assert torch.equal(out[k], plain[k]), f"{what}/P={P}/{k}: pow2 changed the result"
        ups.append(check_pow2(pow2, bound, dx, what))
    assert len(set(ups)) == 1, (what, ups)
    return ups[0]


@pytest.mark.parametrize("M,Cc", [(37, 4), (300, 8), (1031, 48), (4099, 256)])
@pytest.mark.parametrize("relu,batch,res", [(1, 1, 1), (1, 1, 0), (0, 0, 1), (0, 1, 0)])
def test_bn_bwd_pow2(hip, M, Cc, relu, batch, res):
    bn_check(hip, bn_inputs(M, Cc, relu), relu, batch, res, f"bn {M}x{Cc} relu={relu} batch={batch}")


@pytest.mark.parametrize("where", ["first_row", "last_row", "last_row_last_channel"])
def test_bn_bwd_pow2_outlier(hip, where):
    """one element of dy 1e4 times the rest: the maximum the scale hangs on sits in the first row,
    in the last row (the tail loop of the last row slice) or in the last channel of the last row"""
    M, Cc = 1031, 48
    row, c = {"first_row": (0, 5), "last_row": (M - 1, 5), "last_row_last_channel": (M - 1, Cc - 1)}[where]
    t = {k: v.clone() for k, v in bn_inputs(M, Cc, 1).items()}
    t["dy"][row, c] *= 1e4
    t["y"][row, c] = t["y"][row, c].clamp(min=1.0)      # the outlier survives the ReLU mask
    bn_check(hip, t, 1, 1, 0, f"bn outlier {where}")


@pytest.mark.parametrize("scale", [3e-7, 5e3, 0.0])
def test_bn_bwd_pow2_scales(hip, scale):
    t = dict(bn_inputs(1031, 48, 1))
    t["dy"] = t["dy"] * scale
    up = bn_check(hip, t, 1, 1, 0, f"bn dy x{scale:g}")
    if scale == 0.0:
        assert up == 1.0


# ------------------------------------------------------------------ GroupNorm
@functools.lru_cache(maxsize=None)
def gn_inputs(N, HW, Cc, groups, relu):
    cpg = Cc // groups
    x = rnd(N, HW, Cc, seed=1) * 2 + 0.3
    xg = x.view(N, HW, groups, cpg)
    mean = xg.mean((1, 3)).contiguous()
    rstd = torch.rsqrt(xg.var((1, 3), unbiased=False) + 1e-5).contiguous()
    gamma = rnd(Cc, seed=2).abs() + 0.5
    y = ((xg - mean.view(N, 1, groups, 1)) * rstd.view(N, 1, groups, 1)).reshape(N, HW, Cc) * gamma \
        + rnd(Cc, seed=3)
    if relu:
        y = torch.relu(y)
    return dict(dy=rnd(N, HW, Cc, seed=4), y=y.contiguous(), x=x, mean=mean, rstd=rstd, gamma=gamma)


def gn_reference(t, groups, relu):
    """fp64: (dx, dgamma, dbeta, dres, bound) -- dx = rstd (g gamma - s1/cnt - xhat s2/cnt), s1 / s2
    the sums of g gamma and g gamma xhat over a (sample, group); the bound is the per-sample form
    above gn_bwd_finalize_kernel, maximised over samples"""
    d = {k: v.double() for k, v in t.items()}
    N, HW, Cc = d["dy"].shape
    cpg = Cc // groups
    v5 = lambda a: a.view(N, HW, groups, cpg)
    g = v5(d["dy"] * (d["y"] > 0) if relu else d["dy"])
    mean, rstd = d["mean"].view(N, 1, groups, 1), d["rstd"].view(N, 1, groups, 1)
    ga = d["gamma"].view(1, 1, groups, cpg)
    xc = v5(d["x"]) - mean
    xh = xc * rstd
    cnt = HW * cpg
    s1 = (g * ga).sum((1, 3), keepdim=True)
    s2 = (g * ga * xh).sum((1, 3), keepdim=True)
    dx = rstd * (g * ga - s1 / cnt - xh * s2 / cnt)
    per = rstd.abs() * (g.abs().amax(1, keepdim=True) * ga.abs() + s1.abs() / cnt
                        + xc.abs().amax(1, keepdim=True) * (rstd * s2).abs() / cnt)
    return (dx.reshape(N, HW, Cc), (g * xh).sum((0, 1)).reshape(Cc), g.sum((0, 1)).reshape(Cc),
            g.reshape(N, HW, Cc), float(per.max()))


def gn_run(hip, t, groups, relu, res, P):
    N, HW, Cc = t["dy"].shape
    g = dev(t)
    out = dict(dx=torch.zeros(N, HW, Cc, device=DEV),
               dres=torch.zeros(N, HW, Cc, device=DEV) if res else None,
               dgamma=torch.zeros(Cc, device=DEV), dbeta=torch.zeros(Cc, device=DEV))
    pow2 = torch.zeros(2, P, device=DEV) if P else None
    ws = torch.empty(hip.gn_bwd_workspace_floats(N, HW, Cc, groups), device=DEV)
    hip.gn_bwd(g["dy"], g["y"], g["x"], g["mean"], g["rstd"], g["gamma"], N, HW, Cc, groups, relu,
               out["dx"], out["dres"], out["dgamma"], out["dbeta"], ws, pow2)
    torch.cuda.synchronize()
    return out, pow2


def gn_check(hip, t, groups, relu, res, what, Ps=(7, 300)):
    dx, dg, db, g, bound = gn_reference(t, groups, relu)
    ref = dict(dx=dx, dgamma=dg, dbeta=db, dres=g)
    keys = ("dx", "dgamma", "dbeta") + (("dres",) if res else ())
    plain, _ = gn_run(hip, t, groups, relu, res, 0)
    ups = []
    for P in Ps:
        out, pow2 = gn_run(hip, t, groups, relu, res, P)
        for k in keys:
            close(out[k], ref[k], f"{what}/P={P}/{k}")
            assert torch.equal(out[k], plain[k]), f"{what}/P={P}/{k}: pow2 changed the result"
        ups.append(check_pow2(pow2, bound, dx, what))
    assert len(set(ups)) == 1, (what, ups)
    return ups[0]


GN_SHAPES = [
    (3, 50, 12, 3),       # N*groups = 9: odd
    (1, 130, 8, 1),       # N*groups = 1: odd; a two-pixel last chunk
    (3, 129, 12, 4),      # cpg = 3: a channel quad spans two groups; a one-pixel last chunk
    (5, 16, 256, 128),
    (2, 300, 64, 16),
]


@pytest.mark.parametrize("N,HW,Cc,groups", GN_SHAPES)
@pytest.mark.parametrize("relu,res", [(1, 1), (0, 0)])
def test_gn_bwd_pow2(hip, N, HW, Cc, groups, relu, res):
    gn_check(hip, gn_inputs(N, HW, Cc, groups, relu), groups, relu, res,
             f"gn {N}x{HW}x{Cc}/{groups} relu={relu}")


@pytest.mark.parametrize("where", ["first_row", "last_row", "last_row_last_channel"])
def test_gn_bwd_pow2_outlier(hip, where):
    """as test_bn_bwd_pow2_outlier: the last row is the one-pixel last chunk of the last sample"""
    N, HW, Cc, groups = 3, 129, 12, 4
    n, p, c = {"first_row": (0, 0, 5), "last_row": (N - 1, HW - 1, 5),
               "last_row_last_channel": (N - 1, HW - 1, Cc - 1)}[where]
    t = {k: v.clone() for k, v in gn_inputs(N, HW, Cc, groups, 1).items()}
    t["dy"][n, p, c] *= 1e4
    t["y"][n, p, c] = t["y"][n, p, c].clamp(min=1.0)
    gn_check(hip, t, groups, 1, 0, f"gn outlier {where}")


@pytest.mark.parametrize("scale", [3e-7, 5e3, 0.0])
def test_gn_bwd_pow2_scales(hip, scale):
    t = dict(gn_inputs(2, 300, 64, 16, 1))
    t["dy"] = t["dy"] * scale
    up = gn_check(hip, t, 16, 1, 0, f"gn dy x{scale:g}")
    if scale == 0.0:
        assert up == 1.0


def test_gn_bwd_workspace_layout(hip):
    """[N,chunks,C,2] partial sums | [N,groups,2] group sums, padded to a multiple of 4 floats so that
    the next segment starts on a 16-byte boundary | [N,chunks,C,2] partial maxima | [N] bounds |
    [N,C,2] per-sample shares of dbeta / dgamma"""
    N, HW, Cc, groups = 3, 50, 12, 3
    chunks = 1                                  # ceil(50 / 128)
    per_cc = N * chunks * Cc * 2                # 72
    s12 = (N * groups * 2 + 3) // 4 * 4         # 18 -> 20
    shares = N * Cc * 2                         # 72
    assert hip.gn_bwd_workspace_floats(N, HW, Cc, groups) == per_cc + s12 + per_cc + N + shares == 239
    # even N*groups: nothing to pad
    assert hip.gn_bwd_workspace_floats(2, 300, 64, 16) == 2 * (2 * 3 * 64 * 2) + 2 * 16 * 2 + 2 + 2 * 64 * 2


# ------------------------------------------------------------------ argument checks
def test_pow2_argument_checks(hip):
    """refused before any kernel that would write the scale: a dx off 16-byte alignment (BN: the
    scalar kernels have no maxima pass), C % 4 != 0 (GN)"""
    M, Cc = 64, 8
    t = dev(bn_inputs(M, Cc, 1))
    buf = torch.zeros(M * Cc + 4, device=DEV)
    ws = torch.empty(hip.bn_bwd_workspace_floats(M, Cc), device=DEV)
    dg, db, pow2 = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV), torch.zeros(2, 7, device=DEV)
    with pytest.raises(RuntimeError):
        hip.bn_bwd(t["dy"], t["y"], t["x"], t["mean"], t["rstd"], t["gamma"], M, Cc, 1, 1,
                   buf[1:1 + M * Cc].view(M, Cc), None, dg, db, ws, pow2)
    N, HW, Cc, groups = 2, 20, 6, 3
    t = dev(gn_inputs(N, HW, Cc, groups, 1))
    ws = torch.empty(hip.gn_bwd_workspace_floats(N, HW, Cc, groups), device=DEV)
    dg, db = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    with pytest.raises(RuntimeError):
        hip.gn_bwd(t["dy"], t["y"], t["x"], t["mean"], t["rstd"], t["gamma"], N, HW, Cc, groups, 1,
                   torch.zeros(N, HW, Cc, device=DEV), None, dg, db, ws, pow2)
    torch.cuda.synchronize()
    assert bool((pow2 == 0).all())      # neither call wrote the scale
