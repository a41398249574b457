"""Every convolution kernel INSTANCE by name, and against an fp64 convolution.

vlnce_conv2d_last_path() names a family; behind each family sit template instances with their own
product schedule, scaling and epilogue (include/vlnce_hip.h: vlnce_conv2d_last_kernel).  INSTANCES
below lists every instance the four dispatchers can launch, with the smallest launch that lands on
it; per instance and plane format the tests assert
  * the instance that ran (HipLib.conv2d_last_kernel(), directly after the launch),
  * the relative rms error against F.conv2d in fp64 of the same operands: < 1e-6, the project's bound
    (a bf16-plane kernel that drops one of its six plane products sits at 2.3e-6 .. 2.8e-6, an
    fp16-plane kernel without a cross product at 2e-4; correct ones at 1e-7 .. 5e-7),
  * the largest rms error over aligned 32 x 32 output blocks, relative to the reference's global
    rms: at most 3 x the same figure of the fp32 CPU contract (tests/hostsim.py) on the same
    operands -- a defect limited to a ragged tail tile or one column block does not average out,
  * format 2's range contract: an activation beyond fp16's range gives non-finite outputs exactly
    where it is read, never a wrong finite value.
The same statistics for the weight gradient, the stem from frames, the large-linear route and the
data gradient of conv_backward."""
import collections
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import conv_dispatch as cd
import test_kernels_gpu as tk
from test_kernels_gpu import CONV_CASES, DEV, P3_CASES, SIM, rnd
from vlnce_amd import _lib, ops
from vlnce_amd._lib import ConvKernel, WgradKernel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    return _lib.get_lib()


def need_full_device():
    if not tk.full_device():
        pytest.skip(f"the instance a launch lands on depends on the CU count: the table is written for "
                    f"{cd.CUS} CUs, this device has "
                    f"{torch.cuda.get_device_properties(0).multi_processor_count}")


# ------------------------------------------------------------------ B1: the instance table
# shapes: (N, H, W, Cin, Cout, k, stride, pad); every one gives >= 4096 outputs with 64 <= K <= 2304
DENSE = (4, 32, 32, 64, 128, 3, 1, 1)     # M = 4096, K = 576: 128 tiles of 64 x 64 (no split-K)
ONE = (3, 20, 12, 192, 256, 1, 1, 0)      # M = 720 (ragged in every tile height), K = 192
ONE_S3A = (3, 20, 12, 64, 256, 1, 1, 0)
ONE_S3B = (3, 20, 12, 128, 512, 1, 1, 0)
OFF = dict(m3=0)

Inst = collections.namedtuple("Inst", "kernel shape opts dual")
INSTANCES = []


def _add(kernel, shape, opts, dual=None):
    INSTANCES.append(Inst(kernel, shape, opts, dual))


# family P3, conv_p3_kernel: six tiles x {dense (KxK), gather (1x1), dual (1x1, two inputs)}.  The
# 1x1 forms run only under option "p3" = 1 / 3 (default 2: KxK layers only).
for _t in range(1, 7):
    _add(ConvKernel("p3", "conv_p3", 0, _t, "dense", 0), DENSE, dict(OFF, p3_tile=_t))
    _add(ConvKernel("p3", "conv_p3", 0, _t, "gather", 0), ONE, dict(OFF, p3=1, u3=0, s3=0, p3_tile=_t))
    _add(ConvKernel("p3", "conv_p3", 0, _t, "dual", 0), ONE, dict(OFF, p3=1, u3=0, s3=0, p3_tile=_t), "bn")
# family P3, conv_u3_kernel: rows 64 / 128 x kind 0 / 1 / 2 at 8 waves; 4 waves always with 64 rows
for _kind, _dual in enumerate((None, "identity", "bn")):
    _add(ConvKernel("p3", "conv_u3", 0, 64, _kind, 8), ONE, dict(OFF, u3=2), _dual)
    _add(ConvKernel("p3", "conv_u3", 0, 128, _kind, 8), ONE, dict(OFF, u3=3), _dual)
    _add(ConvKernel("p3", "conv_u3", 0, 64, _kind, 4), ONE, dict(OFF, u3=3, u3_waves=4), _dual)
# family P3, conv_s3_kernel: Cin 64 / 128
_add(ConvKernel("p3", "conv_s3", 0, 64, 0, 0), ONE_S3A, dict(OFF, s3=2))
_add(ConvKernel("p3", "conv_s3", 0, 128, 0, 0), ONE_S3B, dict(OFF, s3=2))
# family M3: launch_m3<NT, KSPLIT, RB>
_add(ConvKernel("m3", "conv_m3", 0, 2, 1, 4), (2, 16, 16, 64, 256, 1, 1, 0), dict(m3=2))   # K < 128
_add(ConvKernel("m3", "conv_m3", 0, 1, 1, 4), (2, 8, 8, 64, 96, 1, 1, 0), dict(m3=2))      # K < 128, N % 64 != 0
_add(ConvKernel("m3", "conv_m3", 0, 2, 4, 2), (2, 16, 16, 64, 64, 3, 1, 1), dict(m3=3))
_add(ConvKernel("m3", "conv_m3", 0, 1, 8, 1), (2, 8, 8, 256, 64, 3, 1, 1), dict(m3=2))     # K = 2304: 144 slabs
_add(ConvKernel("m3", "conv_m3", 0, 2, 4, 1), (2, 32, 32, 128, 256, 1, 1, 0), dict(m3=2))  # 256 workgroups of 32 x 64
_add(ConvKernel("m3", "conv_m3", 0, 1, 4, 1), (2, 16, 16, 64, 64, 3, 1, 1), dict(m3=2))
# family X3: four tiles, without / with the two-input prologue
for _t in range(1, 5):
    _add(ConvKernel("x3", "conv_x3", 0, _t, 0, 0), DENSE, dict(OFF, p3=0, x3_tile=_t))
    _add(ConvKernel("x3", "conv_x3", 0, _t, 1, 0), ONE, dict(OFF, p3=0, x3_tile=_t), "bn")
# family F32 (igemm_kernel; no planes: format 0)
F32 = dict(conv_math=0)
_add(ConvKernel("f32", "buf", 0, 0, 0, 0), ONE, F32)
_add(ConvKernel("f32", "dual", 0, 0, 0, 0), ONE, F32, "bn")
_add(ConvKernel("f32", "splitk", 0, 36, 0, 0), (2, 8, 8, 256, 64, 3, 1, 1), F32)   # 2 tiles, 72 K-tiles
_add(ConvKernel("f32", "v4", 0, 0, 0, 0), (3, 7, 9, 36, 48, 3, 1, 1), F32)
_add(ConvKernel("f32", "s", 0, 0, 0, 0), (2, 12, 12, 10, 64, 3, 1, 1), F32)         # Cin % 4 != 0, not a stem
_add(ConvKernel("f32", "stem3", 0, 0, 0, 0), (2, 64, 64, 3, 64, 7, 2, 3), F32)
_add(ConvKernel("f32", "stem1", 0, 0, 0, 0), (2, 32, 32, 1, 32, 7, 2, 3), F32)      # K = 49: the kernel's only K
# Not told apart by vlnce_conv2d_last_kernel, hence not listed: the tile of igemm_kernel (128 x 128 /
# 128 x 64 / 64 x 64, option "igemm_tile"; CONV_CASES big_128x128 / big_128x64 under conv_math = 0) and
# conv_u3_kernel's LINEAR = 0 form (stride 2: p3_1x1_s2 under test_conv_u3_forced).


def _launches(inst):
    """(instance, plane format) pairs to run: both formats for a plane kernel, 0 for igemm_kernel"""
    return [0] if inst.kernel.family == "f32" else [1, 2]


def _id(inst, fmt=None):
    k = inst.kernel
    s = "-".join(str(v) for v in (k.kernel, k.a, k.b, k.c))
    s += "-fourwaves" if k.c == 4 and k.kernel == "conv_u3" else ""
    return s if fmt is None else s + ("-fp32", "-bf16x6", "-f16x3")[fmt]


def _launch_of(inst, prologue=True):
    return cd.Launch(*inst.shape, prologue=prologue, dual=inst.dual)


def test_instance_table_lists_every_instance():
    """the table against the template instances the dispatch code can reach (p3_try_launch_ /
    dispatch_p3, u3_launch_, s3_launch, m3_try_launch, dispatch_x3_, vlnce_conv2d_fwd), and against
    tests/conv_dispatch.py: each (shape, options) pair lands where the table says."""
    want = {ConvKernel("p3", "conv_p3", 0, t, m, 0) for t in range(1, 7) for m in ("dense", "gather", "dual")}
    want |= {ConvKernel("p3", "conv_u3", 0, r, k, 8) for r in (64, 128) for k in (0, 1, 2)}
    want |= {ConvKernel("p3", "conv_u3", 0, 64, k, 4) for k in (0, 1, 2)}
    want |= {ConvKernel("p3", "conv_s3", 0, c, 0, 0) for c in (64, 128)}
    want |= {ConvKernel("m3", "conv_m3", 0, *a) for a in ((2, 1, 4), (1, 1, 4), (2, 4, 2), (1, 8, 1),
                                                         (2, 4, 1), (1, 4, 1))}
    want |= {ConvKernel("x3", "conv_x3", 0, t, d, 0) for t in range(1, 5) for d in (0, 1)}
    want |= {ConvKernel("f32", k, 0, 0, 0, 0) for k in ("buf", "v4", "s", "stem3", "stem1", "dual")}
    have = {i.kernel._replace(a=0) if i.kernel.kernel == "splitk" else i.kernel for i in INSTANCES}
    assert have == want | {ConvKernel("f32", "splitk", 0, 0, 0, 0)}
    for inst in INSTANCES:
        for fmt in _launches(inst):
            for prologue in (True, False) if not inst.dual else (True,):
                got = cd.expected(_launch_of(inst, prologue), **dict(inst.opts, conv_math=fmt))
                assert got == inst.kernel._replace(fmt=fmt), (inst, fmt, got)
        N, H, W, Cin, Cout, k, s, p = inst.shape
        L = _launch_of(inst)
        assert L.M * Cout >= 4096 and (64 <= L.K <= 2304 or inst.kernel.kernel == "stem1"), inst


# ------------------------------------------------------------------ operands, references, statistics
HOT = 1.0e5      # beyond fp16's range (65504)


@functools.lru_cache(maxsize=None)
def operands(shape, signed, prologue, dual, hot=None):
    """CPU operands of one launch + its fp64 reference + the fp32 CPU contract's result.
    hot: None | "direct" (one input element is 1e5) | "prologue" (it is 1e3 and its channel's
    in_scale 100: beyond fp16's range only after the prologue).  Returns a dict; `hit` marks the
    outputs whose receptive field holds the hot element."""
    N, H, W, Cin, Cout, k, s, p = shape
    x = rnd(N, H, W, Cin, seed=31)
    x = x if signed else x.abs()
    w = rnd(Cout, k, k, Cin, seed=32, scale=(Cin * k * k) ** -0.5)
    w = torch.where(w == 0, torch.full_like(w, 1e-3), w)
    t = dict(x=x, w=w)
    if prologue or dual:
        t["in_scale"] = rnd(Cin, seed=33).abs() + 0.5
        t["in_shift"] = rnd(Cin, seed=34) * 0.3
        t["in_center"] = rnd(Cin, seed=35) * 0.5
    if dual:
        t["x2"] = rnd(N, H, W, Cin, seed=36)
        if dual == "bn":
            t["in2_scale"] = rnd(Cin, seed=37).abs() + 0.5
            t["in2_shift"] = rnd(Cin, seed=38) * 0.3
            t["in2_center"] = rnd(Cin, seed=39) * 0.5
    hit = None
    if hot:
        n0, h0, w0, c0 = N - 1, H // 2, W // 2 + 1, Cin - 3
        x = t["x"] = x.clone()
        if "in_scale" in t:
            t["in_scale"] = t["in_scale"].clone()
            t["in_scale"][c0] = 100.0 if hot == "prologue" else 1.0
            x[n0, h0, w0, c0] = 1.0e3 if hot == "prologue" else HOT
        else:
            assert hot == "direct"
            x[n0, h0, w0, c0] = HOT
        ind = torch.zeros(N, 1, H, W)
        ind[n0, 0, h0, w0] = 1.0
        hit = F.conv2d(ind, torch.ones(1, 1, k, k), stride=s, padding=p) > 0     # [N, 1, Ho, Wo]
        hit = hit.permute(0, 2, 3, 1).expand(-1, -1, -1, Cout).reshape(-1, Cout)
    g = ops.conv_geometry(x, w, s, p)
    # fp64: the prologue in fp64 on the fp32 operands, then the convolution
    xin = x.double()
    if "in_scale" in t:
        xin = (xin - t["in_center"].double()) * t["in_scale"].double() + t["in_shift"].double()
        if dual:
            x2 = t["x2"].double()
            if dual == "bn":
                x2 = (x2 - t["in2_center"].double()) * t["in2_scale"].double() + t["in2_shift"].double()
            xin = xin + x2
        xin = torch.relu(xin)
    ref = F.conv2d(xin.permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), stride=s, padding=p)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, Cout)
    y32 = torch.zeros(N, g["Ho"], g["Wo"], Cout)
    SIM.conv2d_fwd(y=y32, g=g, in_relu=int("in_scale" in t), ldr=Cout, **t)
    return dict(t=t, g=g, ref=ref, sim=y32.reshape(-1, Cout).double(), hit=hit,
                relu=int("in_scale" in t))


def err_stats(y, ref, keep=None):
    """(rms error / rms of ref, largest rms error over the aligned 32 x 32 blocks of the [rows,
    columns] output, ragged edge blocks included, / rms of ref); `keep`: the outputs that count"""
    y, ref = y.detach().cpu().double().reshape(ref.shape), ref.double()
    k = torch.ones_like(ref) if keep is None else keep.double()
    d2 = torch.where(k > 0, (y - ref) ** 2, torch.zeros_like(ref))
    glob = (ref ** 2 * k).sum() / k.sum()

    def blocks(v):   # block sums ([1, 1, rows, cols] -> per 32 x 32 block), zero padding
        R, Cc = v.shape
        v = F.pad(v, (0, -Cc % 32, 0, -R % 32))
        return v.reshape(v.size(0) // 32, 32, v.size(1) // 32, 32).sum((1, 3))
    cnt = blocks(k)
    worst = (blocks(d2) / cnt.clamp(min=1.0))[cnt > 0].max()
    return math.sqrt(d2.sum() / k.sum() / glob), math.sqrt(worst / glob)


def run_instance(hip, inst, fmt, signed, prologue, hot=None):
    """one launch of the instance's shape under its options in plane format `fmt`; asserts the
    instance that ran; returns (gpu output [M, Cout], operands dict)"""
    op = operands(inst.shape, signed, bool(prologue or inst.dual), inst.dual, hot)
    t = {k: v.to(DEV) for k, v in op["t"].items()}
    N, H, W, Cin, Cout, k, s, p = inst.shape
    y = torch.full((N, op["g"]["Ho"], op["g"]["Wo"], Cout), float("nan"), device=DEV)
    pf = fmt or 1
    hip.conv2d_fwd(y=y, g=op["g"], in_relu=op["relu"], ldr=Cout,
                   w_split=ops.split_weights(t["w"], pf), w_frag=ops.pack_weights(t["w"], pf),
                   options=dict(inst.opts, conv_math=fmt), **t)
    got = hip.conv2d_last_kernel()
    path = hip.conv2d_last_path()
    torch.cuda.synchronize()
    assert got == inst.kernel._replace(fmt=fmt), (inst.shape, inst.opts, "ran on", got)
    assert path == ("f32", "x3", "p3", "m3").index(got.family), (inst.shape, inst.opts, path, got)
    return y.reshape(-1, Cout), op


B3 = [(i, f) for i in INSTANCES for f in _launches(i)]


# ------------------------------------------------------------------ B3: precision per instance
@pytest.mark.parametrize("inst,fmt", B3, ids=[_id(i, f) for i, f in B3])
def test_conv_instance_against_fp64(hip, inst, fmt):
    """each instance x plane format: signed and non-negative activations, with and without the
    prologue (scale / shift / centre / ReLU; the two-input instances always have one)."""
    need_full_device()
    seen = []
    for signed in (True, False):
        for prologue in ((True,) if inst.dual else (False, True)):
            y, op = run_instance(hip, inst, fmt, signed, prologue)
            rms, blk = err_stats(y, op["ref"])
            _, blk32 = err_stats(op["sim"], op["ref"])
            seen.append((signed, prologue, f"{rms:.2e}", f"{blk:.2e}", f"{blk32:.2e}"))
            print(_id(inst, fmt), seen[-1])
            # measured on the MI355X, over the four runs of every instance (rms; worst block; worst
            # block of the fp32 CPU convolution; largest ratio of the two):
            #   conv_p3 bf16x6  2.0e-7 .. 3.7e-7   2.3e-7 .. 4.4e-7   2.1e-7 .. 5.1e-7   1.18
            #   conv_p3 f16x3   1.7e-7 .. 2.8e-7   1.8e-7 .. 3.3e-7   2.1e-7 .. 5.1e-7   0.97
            #   conv_u3 bf16x6  2.0e-7 .. 2.1e-7   2.3e-7 .. 2.4e-7   2.1e-7 .. 2.9e-7   1.11
            #   conv_u3 f16x3   1.7e-7 .. 1.8e-7   1.8e-7 .. 2.0e-7   2.1e-7 .. 2.9e-7   0.97
            #   conv_s3 bf16x6  1.1e-7 .. 1.7e-7   1.2e-7 .. 2.1e-7   1.4e-7 .. 2.5e-7   1.13
            #   conv_s3 f16x3   1.1e-7 .. 1.5e-7   1.2e-7 .. 1.8e-7   1.4e-7 .. 2.5e-7   1.01
            #   conv_m3 bf16x6  0.8e-7 .. 2.6e-7   0.9e-7 .. 2.7e-7   1.2e-7 .. 8.8e-7   1.05
            #   conv_m3 f16x3   1.0e-7 .. 2.2e-7   1.1e-7 .. 2.2e-7   1.2e-7 .. 8.8e-7   1.03
            #   conv_x3 bf16x6  2.0e-7 .. 3.6e-7   2.3e-7 .. 4.1e-7   2.1e-7 .. 5.1e-7   1.11
            #   conv_x3 f16x3   1.7e-7 .. 2.7e-7   2.0e-7 .. 3.2e-7   2.1e-7 .. 5.1e-7   0.97
            #   igemm_kernel    1.1e-7 .. 3.1e-7   1.3e-7 .. 3.4e-7   1.1e-7 .. 8.8e-7   1.15 (stem1; split-K 0.27)
            assert rms < 1e-6, (_id(inst, fmt), seen)
            assert blk <= 3.0 * blk32, (_id(inst, fmt), seen)


# ------------------------------------------------------------------ B5: range contract of format 2
PLANE = [i for i in INSTANCES if i.kernel.family != "f32"]


@pytest.mark.parametrize("inst", PLANE, ids=[_id(i) for i in PLANE])
def test_conv_instance_fp16_range_contract(hip, inst):
    """include/vlnce_hip.h, format 2: |activation| >= 65504 gives inf / NaN, never a wrong finite
    value -- one input element of 1e5, given directly and (where the instance has a prologue) reached
    only through in_scale: every output that reads it is non-finite, every other output as close to
    fp64 as without it; in format 1 the same launch is finite and right everywhere."""
    need_full_device()
    for hot in ("direct", "prologue"):
        prologue = hot == "prologue"
        y, op = run_instance(hip, inst, 2, True, prologue, hot)
        hit = op["hit"]
        assert int(hit.sum()) >= inst.shape[4]
        bad = torch.isfinite(y.cpu()) & hit
        assert not bool(bad.any()), (_id(inst), hot, "finite outputs that read the 1e5:", int(bad.sum()))
        rms, blk = err_stats(y, op["ref"], ~hit)
        _, blk32 = err_stats(op["sim"], op["ref"], ~hit)
        print(_id(inst), hot, f"f16x3 rms {rms:.2e} block {blk:.2e} fp32 {blk32:.2e}")
        assert rms < 1e-6 and blk <= 3.0 * blk32, (_id(inst), hot, rms, blk, blk32)
        y1, _ = run_instance(hip, inst, 1, True, prologue, hot)
        assert bool(torch.isfinite(y1).all()), (_id(inst), hot)
        rms, blk = err_stats(y1, op["ref"])
        _, blk32 = err_stats(op["sim"], op["ref"])
        print(_id(inst), hot, f"bf16x6 rms {rms:.2e} block {blk:.2e} fp32 {blk32:.2e}")
        # measured on the MI355X over all plane instances: f16x3 (the outputs that do not read the
        # 1e5) rms 0.8e-7 .. 2.7e-7, worst block at most 1.88 x the fp32 CPU convolution's; bf16x6
        # rms 0.4e-7 .. 2.2e-7, at most 1.63 x
        assert rms < 1e-6 and blk <= 3.0 * blk32, (_id(inst), hot, rms, blk, blk32)


# ------------------------------------------------------------------ forced kernels the suite did not reach
def test_conv_u3_four_waves_forced(hip):
    """conv_u3_kernel with one wave per SIMD (option "u3_waves" = 4: 64 x 256 tiles whatever "u3"
    says) over the conv cases: prologue, statistics, stride 2, both two-input kinds, ragged M."""
    def expect(L):
        if not (cd.p3_eligible(L) and L.k == 1 and L.pad == 0 and L.Cout >= 256
                and L.Cin <= cd.U3_MAX_CIN and cd.reaches_plane_kernels(L)):
            return None
        if cd.expected(L, m3=0, u3=0).kernel == "conv_s3":
            return None
        return ("conv_u3", 64, {None: 0, "identity": 1, "bn": 2}[L.dual], 4)
    for fmt in (2, 1):
        tk._conv_cases_under(hip, CONV_CASES + P3_CASES, want_path=2, expect=expect, min_expected=12,
                             u3=3, u3_waves=4, conv_math=fmt)


# ------------------------------------------------------------------ B4: weight gradient
WG_CASES = [
    # name,             N,  H,  W, Cin, Cout, k, s, p, (TM, split) of wgrad_x6_kernel
    ("tm64_s1_split",  16, 32, 32,  64,  64, 3, 1, 1, (64, True)),     # 16384 pixels
    ("tm128_s1_split",  2, 16, 16,  64, 128, 1, 1, 0, (128, True)),    # 512 pixels: two slices
    ("tm128_s2",        4, 16, 16,  64, 128, 3, 2, 1, (128, False)),   # 256 pixels
    ("tm64_s2",         5, 15, 17,  32,  64, 3, 2, 1, (64, False)),    # 360 pixels, chunks straddle images
]


def wgrad_f32_split(Cout, K, M):
    """vlnce_conv2d_wgrad's fp32 kernel, 64 x 64 tiles: is the reduction split"""
    tiles = -(-Cout // 64) * -(-K // 64)
    return min(-(-1024 // tiles), -(-M // 32) // 4, 512) >= 2


@functools.lru_cache(maxsize=None)
def wgrad_operands(case, size):
    name, N, H, W, Cin, Cout, k, s, p, _ = case
    x = rnd(N, H, W, Cin, seed=41)
    g = ops.conv_geometry(x, torch.empty(Cout, k, k, Cin), s, p)
    dy = rnd(N, g["Ho"], g["Wo"], Cout, seed=42) * size
    ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2).contiguous(), (Cout, Cin, k, k),
                                      dy.double().permute(0, 3, 1, 2).contiguous(), stride=s, padding=p)
    ref = ref.permute(0, 2, 3, 1).reshape(Cout, -1)
    dw32 = torch.zeros(Cout, k, k, Cin)
    SIM.conv2d_wgrad(x, dy, dw32, g)
    return x, dy, g, ref, dw32.reshape(Cout, -1).double()


@pytest.mark.parametrize("size", [1.0, 1e-7], ids=["dy1", "dy1e-7"])
@pytest.mark.parametrize("case", WG_CASES, ids=[c[0] for c in WG_CASES])
def test_wgrad_against_fp64(hip, case, size):
    """vlnce_conv2d_wgrad on wgrad_x6_kernel with bf16 planes, with fp16 planes + dy's power of two,
    and on the fp32 kernel: both row tiles, stride 1 and 2, with and without the split reduction,
    dy of size 1 and 1e-7, against conv2d_weight in fp64.  The reduction runs over up to 16384
    pixels and is added atomically, so the bound is the fp32 CPU contract's own error on the same
    operands x 3, for the whole-output rms and for the worst 32 x 32 block."""
    need_full_device()
    name, N, H, W, Cin, Cout, k, s, p, (tm, split) = case
    x, dy, g, ref, dw32 = wgrad_operands(case, size)
    rms32, blk32 = err_stats(dw32, ref)
    up = 2.0 ** (14 - math.frexp(float(dy.abs().max()))[1])
    pow2 = torch.stack([torch.full((8,), up), torch.full((8,), 1.0 / up)]).to(DEV)
    xd, dyd = x.to(DEV), dy.to(DEV)
    M = N * g["Ho"] * g["Wo"]
    runs = [("bf16x6", None, {}, WgradKernel(1, tm, split)),
            ("f16x3", pow2, {}, WgradKernel(2, tm, split)),
            ("fp32", None, dict(wgrad_tile=1), WgradKernel(0, 64, wgrad_f32_split(Cout, k * k * Cin, M)))]
    for what, p2, opts, kern in runs:
        dw = torch.full((Cout, k, k, Cin), float("nan"), device=DEV)
        with hip.options(**opts):
            hip.conv2d_wgrad(xd, dyd, dw, g, p2)
            got = hip.conv2d_wgrad_last_kernel()
        torch.cuda.synchronize()
        assert got == kern, (name, what, got)
        rms, blk = err_stats(dw, ref)
        print(name, size, what, f"rms {rms:.2e} (fp32 CPU {rms32:.2e}) block {blk:.2e} (fp32 CPU {blk32:.2e})")
        # measured on the MI355X (rms, fp32 CPU rms; dy of size 1 and 1e-7 agree to 2 %):
        #   tm64_s1_split   bf16x6 3.0e-7  f16x3 2.5e-7  fp32 kernel 2.9e-7   CPU 8.0e-7 (worst block 8.6e-7)
        #   tm128_s1_split  bf16x6 2.4e-7  f16x3 1.9e-7  fp32 kernel 2.1e-7   CPU 2.8e-7
        #   tm128_s2        bf16x6 2.3e-7  f16x3 1.9e-7  fp32 kernel 2.0e-7   CPU 2.8e-7
        #   tm64_s2         bf16x6 2.7e-7  f16x3 2.2e-7  fp32 kernel 1.9e-7   CPU 2.3e-7
        # worst block / the CPU's worst block: at most 1.17 (tm64_s2, bf16x6)
        assert rms <= 3.0 * rms32 and blk <= 3.0 * blk32, (name, size, what, rms, rms32, blk, blk32)


def test_wgrad_fp32_kernel_128_tiles(hip):
    """the fp32 kernel's 128 x 128 tile (option "wgrad_tile" = 128, a layer wgrad_x6 does not cover)"""
    N, H, W, Cin, Cout, k = 3, 7, 9, 36, 128, 3
    x, dy = rnd(N, H, W, Cin, seed=43), rnd(N, H, W, Cout, seed=44)
    g = ops.conv_geometry(x, torch.empty(Cout, k, k, Cin), 1, 1)
    ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2).contiguous(), (Cout, Cin, k, k),
                                      dy.double().permute(0, 3, 1, 2).contiguous(), padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(Cout, -1)
    dw32 = torch.zeros(Cout, k, k, Cin)
    SIM.conv2d_wgrad(x, dy, dw32, g)
    dw = torch.full((Cout, k, k, Cin), float("nan"), device=DEV)
    with hip.options(wgrad_tile=128):
        hip.conv2d_wgrad(x.to(DEV), dy.to(DEV), dw, g)
        assert hip.conv2d_wgrad_last_kernel() == WgradKernel(0, 128, False)
    rms, blk = err_stats(dw, ref)
    rms32, blk32 = err_stats(dw32, ref)
    print(f"wgrad fp32 128: rms {rms:.2e} ({rms32:.2e}) block {blk:.2e} ({blk32:.2e})")
    assert rms <= 3.0 * rms32 and blk <= 3.0 * blk32, (rms, rms32, blk, blk32)


# ------------------------------------------------------------------ B3: the other routes to the plane kernels
@pytest.mark.parametrize("fmt", [2, 1], ids=["f16x3", "bf16x6"])
def test_stem7_against_fp64(hip, fmt):
    """vlnce_stem7_fwd from uint8 frames (K = 147), raw output, against fp64 of the true filters"""
    N, H, W, Cout = 2, 50, 38, 64
    x = torch.randint(0, 256, (N, H, W, 3), generator=torch.Generator().manual_seed(51)).to(torch.uint8)
    w = rnd(Cout, 7, 7, 3, seed=52) * 147 ** -0.5
    isc = torch.tensor([1 / 58.4, 1 / 57.1, 1 / 57.4])
    ish = torch.tensor([-2.12, -2.04, -1.80])
    xin = x.double() * isc.double() + ish.double()
    ref = F.conv2d(xin.permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), stride=2, padding=3)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, Cout)
    y32 = F.conv2d((x.float() * isc + ish).permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), stride=2, padding=3)
    y32 = y32.permute(0, 2, 3, 1).reshape(-1, Cout)
    fr = ops.frames(x.to(DEV))
    y = ops.stem7(fr, ops.stem7_pack_weights(w.to(DEV), fmt), Cout, isc.to(DEV), ish.to(DEV), w_format=fmt)
    rms, blk = err_stats(y, ref)
    _, blk32 = err_stats(y32, ref)
    print(f"stem7 fmt {fmt}: rms {rms:.2e} block {blk:.2e} fp32 CPU block {blk32:.2e}")
    # measured on the MI355X: f16x3 rms 1.6e-7, worst block 1.8e-7; bf16x6 1.9e-7, 2.1e-7; fp32 CPU block 2.5e-7
    assert rms < 1e-6 and blk <= 3.0 * blk32, (rms, blk, blk32)


def test_large_linear_against_fp64(hip):
    """ops.linear at >= 1024 rows and >= 1 GFLOP: forward through vlnce_conv2d_fwd in the default
    plane format, the input gradient in format 1"""
    M, K, N = 2048, 512, 512
    x, w, b, gy = rnd(M, K, seed=53), rnd(N, K, seed=54, scale=K ** -0.5), rnd(N, seed=55), rnd(M, N, seed=56)
    xd, wd, bd = x.to(DEV).requires_grad_(), w.to(DEV), b.to(DEV)
    y = ops.linear(xd, wd, bd)
    assert hip.conv2d_last_kernel().family != "f32"
    (dx,) = torch.autograd.grad(y, xd, gy.to(DEV))
    # (autograd's worker thread made that launch and the record is per thread: the same launch from here)
    dx2 = torch.empty_like(dx)
    assert ops._planes_gemm(gy.to(DEV), N, wd.t().contiguous(), dx2, w_format=ops.PLANES_BF16X6)
    k = hip.conv2d_last_kernel()
    assert k.family != "f32" and k.fmt == 1, k
    ref = x.double() @ w.double().t() + b.double()
    rms, blk = err_stats(y, ref)
    _, blk32 = err_stats(x @ w.t() + b, ref)
    print(f"linear fwd: rms {rms:.2e} block {blk:.2e} fp32 CPU block {blk32:.2e}")
    assert rms < 1e-6 and blk <= 3.0 * blk32, (rms, blk, blk32)
    ref = gy.double() @ w.double()
    _, blk32 = err_stats(gy @ w, ref)
    for got in (dx, dx2):
        rms, blk = err_stats(got, ref)
        print(f"linear dx: rms {rms:.2e} block {blk:.2e} fp32 CPU block {blk32:.2e}")
        assert rms < 1e-6 and blk <= 3.0 * blk32, (rms, blk, blk32)


@pytest.mark.parametrize("size", [1.0, 1e-7], ids=["dy1", "dy1e-7"])
@pytest.mark.parametrize("form", ["bf16x6", "f16x3_pow2"])
def test_conv_backward_data_gradient_against_fp64(hip, form, size):
    """conv_backward's data gradient (the forward kernels on the flipped, transposed filters): bf16
    planes, and fp16 planes with dy's power of two in the prologue / epilogue; dy of size 1 and 1e-7"""
    from vlnce_amd.encoders import trunk_backward as tb
    N, H, W, Cin, Cout, k = 2, 16, 16, 64, 128, 3
    x, w = rnd(N, H, W, Cin, seed=57), rnd(Cout, k, k, Cin, seed=58, scale=(Cin * 9) ** -0.5)
    dy = rnd(N, H, W, Cout, seed=59) * size
    ref = torch.nn.grad.conv2d_input((N, Cin, H, W), w.double().permute(0, 3, 1, 2),
                                     dy.double().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    d32 = torch.nn.grad.conv2d_input((N, Cin, H, W), w.permute(0, 3, 1, 2).contiguous(),
                                     dy.permute(0, 3, 1, 2).contiguous(), padding=1).permute(0, 2, 3, 1)
    pow2 = None
    if form == "f16x3_pow2":
        up = 2.0 ** (14 - math.frexp(float(dy.abs().max()))[1])
        pow2 = torch.stack([torch.full((128,), up), torch.full((128,), 1.0 / up)]).to(DEV)
    dx, _ = tb.conv_backward(x.to(DEV), w.to(DEV), dy.to(DEV), 1, 1, True, pow2=pow2)
    kern = hip.conv2d_last_kernel()
    assert kern.family != "f32" and kern.fmt == (2 if pow2 is not None else 1), kern
    ref = ref.reshape(-1, Cin)
    rms, blk = err_stats(dx, ref)
    _, blk32 = err_stats(d32.reshape(-1, Cin), ref)
    print(f"dgrad {form} dy {size:g} on {kern}: rms {rms:.2e} block {blk:.2e} fp32 CPU block {blk32:.2e}")
    # measured on the MI355X (conv_m3<1,4,1>): bf16x6 rms 2.5e-7, worst block 2.7e-7; f16x3 + power of
    # two 2.0e-7, 2.1e-7; fp32 CPU block 2.4e-7; the same at both sizes of dy
    assert rms < 1e-6 and blk <= 3.0 * blk32, (rms, blk, blk32)
