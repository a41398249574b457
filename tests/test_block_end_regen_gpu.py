"""The block end of ResNet-50 layers 1-2 that regenerates conv3's output instead of reading it back.

Two launches replace conv3 (raw output stored) + the dual block end (raw output read):
  * conv_s3_kernel's statistics-only instance (vlnce_epilogue.stats_only): bn3's batch statistics
    from a pass over conv3's INPUT, nothing stored;
  * conv_r3_kernel (vlnce_prologue.regen): conv3's tile computed again in registers, bn3 + skip +
    ReLU, the block output stored to side_out and multiplied into the next block's first 1x1.
Checked here, on the smallest shapes that reach every path of the two kernels (option "s3_wgs" caps
the workgroups, so that 1 064 rows are 17 tiles over 4 workgroups: four or five tiles each, the last
one ragged, 1 064 % 64 = 40; and one 40-row launch, M < 64.  Tile moments (stat_partial) exist per 32
rows of a sample only when the sample's pixel count is a multiple of 32, so the cases with that
statistics target have 1 056 and 32 rows: a ragged last tile of 32 rows):
  1. statistics-only against storing launch: identical tile moments, column sums equal up to the
     order of the fp64 atomic adds, both within 1e-6 of an fp64 convolution;
  2. the regenerating block end against the old pair with the same normalisation vectors handed
     in: side_out bit for bit, the second product and both outputs within 1e-6 rms of fp64;
  3. the RGB trunk, new route against old (option "r3"), eagerly, while capturing and in replays.
"""
import pytest
import torch

import test_kernels_gpu as tk
from test_kernels_gpu import DEV, rnd
from vlnce_amd import _lib, ops
from vlnce_amd._lib import ConvKernel

pytestmark = pytest.mark.gpu

BOUND = 1e-6          # the project's relative rms bound against fp64 (tests/test_conv_routes_gpu.py)
WGS = 4               # workgroups of the capped launches
M_TILES = 64 * 4 * WGS + 40   # 17 tiles: every workgroup runs >= 4, the last tile has 40 rows
M_SMALL = 40
SHAPES = [(64, 256, 64), (64, 256, 128), (128, 512, 128), (128, 512, 256)]   # (K1, N1, N2)


def rows_for(M, target):
    """the launch's rows: tile moments need a multiple of 32"""
    return M if target == "acc" else M - 8


@pytest.fixture(scope="module")
def hip():
    return _lib.get_lib()


def rel_rms(a, ref):
    a, ref = a.double(), ref.double()
    return float(((a - ref).pow(2).mean() / ref.pow(2).mean().clamp_min(1e-300)).sqrt())


def signed_scale(n, seed):
    """|scale| in [0.5, ...) with every third channel negative"""
    s = rnd(n, seed=seed).abs() + 0.5
    s[::3] = -s[::3]
    return s


@pytest.fixture(scope="module")
def operands():
    """device operands of one (K1, N1, N2, M) problem + the fp64 references, computed once"""
    cache = {}

    def get(K1, N1, N2, M):
        key = (K1, N1, N2, M)
        if key in cache:
            return cache[key]
        t = dict(
            raw2=rnd(1, M, 1, K1, seed=1),
            s2=signed_scale(K1, 2), t2=rnd(K1, seed=3) * 0.3, c2=rnd(K1, seed=4) * 0.5,
            w3=rnd(N1, 1, 1, K1, seed=5, scale=K1 ** -0.5),
            s3=signed_scale(N1, 6), t3=rnd(N1, seed=7) * 0.3, c3=rnd(N1, seed=8) * 0.5,
            skip=rnd(1, M, 1, N1, seed=9),
            sk_s=signed_scale(N1, 10), sk_t=rnd(N1, seed=11) * 0.3, sk_c=rnd(N1, seed=12) * 0.5,
            wn=rnd(N2, 1, 1, N1, seed=13, scale=N1 ** -0.5))
        t = {k: v.to(DEV).contiguous() for k, v in t.items()}
        d = {k: v.double() for k, v in t.items()}
        ref = {}
        for center in (True, False):
            a = torch.relu((d["raw2"].reshape(M, K1) - (d["c2"] if center else 0)) * d["s2"] + d["t2"])
            raw3 = a @ d["w3"].reshape(N1, K1).t()
            ref["raw3", center] = raw3
            for skip in ("identity", "bn"):
                sk = d["skip"].reshape(M, N1)
                if skip == "bn":
                    sk = (sk - (d["sk_c"] if center else 0)) * d["sk_s"] + d["sk_t"]
                y = torch.relu((raw3 - (d["c3"] if center else 0)) * d["s3"] + d["t3"] + sk)
                ref["y", center, skip] = y
                ref["out", center, skip] = y @ d["wn"].reshape(N2, N1).t()
        cache[key] = (t, ref)
        return cache[key]

    return get


def moments_of_sums(hip, acc, M, C):
    """(mean, biased variance) per channel from vlnce_bn_sums.acc; leaves acc zero"""
    scale = torch.empty(C, device=DEV)
    mean, rstd = torch.empty_like(scale), torch.empty_like(scale)
    hip.bn_finalize_sums(acc, M, None, None, 0.0, 0.1, None, None, scale, mean, rstd_out=rstd)
    return mean.double(), rstd.double().pow(-2)


def moments_of_partials(partial, M, rows):
    """the same from tile moments [tiles, C, 2] = {sum, M2 about the tile mean}"""
    p = partial.double()
    n = torch.full((p.size(0),), float(rows), device=p.device, dtype=torch.float64)
    n[-1] = M - rows * (p.size(0) - 1)
    S = p[:, :, 0].sum(0)
    Q = (p[:, :, 1] + p[:, :, 0] ** 2 / n[:, None]).sum(0)
    mean = S / M
    return mean, (Q - S * mean) / M


def check_moments(got, ref_rows, what):
    """channel means and variances against an fp64 output [M, C]: relative rms over the channels"""
    mean, var = got
    assert rel_rms(mean, ref_rows.mean(0)) < BOUND, (what, "mean", rel_rms(mean, ref_rows.mean(0)))
    assert rel_rms(var, ref_rows.var(0, unbiased=False)) < BOUND, (what, "var")


# ------------------------------------------------------------------ 1. the statistics-only launch
@pytest.mark.parametrize("fmt", [1, 2], ids=["bf16x6", "f16x3"])
@pytest.mark.parametrize("center", [True, False], ids=["center", "nocenter"])
@pytest.mark.parametrize("K1,N1,M", [(64, 256, M_TILES), (128, 512, M_TILES), (64, 256, M_SMALL),
                                     (128, 512, M_SMALL)])
def test_stats_only_launch_matches_the_storing_launch(hip, operands, K1, N1, M, center, fmt):
    N2 = 64 if K1 == 64 else 128   # (unused here: the operands are shared with the block-end tests)
    t, ref = operands(K1, N1, N2, M)
    pro = dict(in_scale=t["s2"], in_shift=t["t2"], in_center=t["c2"] if center else None, in_relu=True)
    want = ref["raw3", center]
    # N1 = 512 has two column tiles: 2 x WGS workgroups keep four row walkers
    with hip.options(conv_math=fmt, m3=0, s3=2, s3_wgs=WGS * (N1 // 256)):
        w = t["w3"]
        # ---- column sums (vlnce_bn_sums)
        acc = torch.zeros((ops.BN_SHARDS, N1, 2), device=DEV, dtype=torch.float64)
        y = ops.conv2d_bn_sums(t["raw2"], w, 1, 0, acc, **pro)
        assert hip.conv2d_last_kernel() == ConvKernel("p3", "conv_s3", fmt, K1, 0, 0)
        stored = moments_of_sums(hip, acc, M, N1)
        assert float(acc.abs().max()) == 0.0
        e = ops.conv2d_bn_sums(t["raw2"], w, 1, 0, acc, stats_only=True, **pro)
        assert hip.conv2d_last_kernel() == ConvKernel("p3", "conv_s3", fmt, K1, 1, 0)
        assert e.shape == (1, M, 1, 0)
        only = moments_of_sums(hip, acc, M, N1)
        assert rel_rms(y.reshape(M, N1), want) < BOUND
        check_moments(stored, want, "storing launch")
        check_moments(only, want, "statistics-only launch")
        # the two launches add the same per-wave fp64 terms in a different order: the difference is
        # fp64 rounding, held here to a relative 1e-6 of the channel's scale sqrt(mean^2 + var)
        scale = (stored[0] ** 2 + stored[1]).sqrt()
        assert float(((only[0] - stored[0]).abs() / scale).max()) < 1e-6
        assert float(((only[1] - stored[1]).abs() / stored[1]).max()) < 1e-6
        # ---- tile moments (stat_partial): one wave writes each, no atomics -> bit for bit
        Mp = rows_for(M, "partial")
        t, ref = operands(K1, N1, N2, Mp)
        want = ref["raw3", center]
        pro = dict(pro, in_scale=t["s2"], in_shift=t["t2"], in_center=t["c2"] if center else None)
        w = t["w3"]
        y2, (partial, tiles_m, rows) = ops.conv2d_nhwc(t["raw2"], w, 1, 0, want_stats=True, **pro)
        assert hip.conv2d_last_kernel() == ConvKernel("p3", "conv_s3", fmt, K1, 0, 0) and rows == 32
        assert rel_rms(y2.reshape(Mp, N1), want) < BOUND
        p2 = torch.full_like(partial, float("nan"))
        g = ops.conv_geometry(t["raw2"], w, 1, 0)
        hip.conv2d_fwd(t["raw2"], w, None, g, **dict(pro, in_relu=1), ldr=N1, stat_partial=p2,
                       w_split=ops.split_weights(w, fmt), w_frag=ops.pack_weights(w, fmt), w_format=fmt,
                       stats_only=True)
        assert hip.conv2d_last_kernel() == ConvKernel("p3", "conv_s3", fmt, K1, 1, 0)
        assert torch.equal(p2, partial)
        check_moments(moments_of_partials(p2, Mp, rows), want, "statistics-only tile moments")


def test_stats_only_launch_rejects_what_it_cannot_do(hip, operands):
    t, _ = operands(64, 256, 64, M_SMALL)
    w = t["w3"]
    g = ops.conv_geometry(t["raw2"], w, 1, 0)
    acc = torch.zeros((ops.BN_SHARDS, 256, 2), device=DEV, dtype=torch.float64)
    ws = torch.empty(max(hip.conv2d_bn_workspace_bytes(g), 16), device=DEV, dtype=torch.uint8)
    kw = dict(ldr=256, w_split=ops.split_weights(w), w_frag=ops.pack_weights(w), stats_only=True)
    y = torch.empty(1, M_SMALL, 1, 256, device=DEV)
    with pytest.raises(RuntimeError, match="takes no output"):
        hip.conv2d_fwd(t["raw2"], w, y, g, bn=(acc, ws), **kw)
    with pytest.raises(RuntimeError, match="needs bn or stat_partial"):
        hip.conv2d_fwd(t["raw2"], w, None, g, **kw)
    wide = rnd(256, 1, 1, 256, seed=3).to(DEV)          # Cin = 256: not a short-K expansion
    xw = rnd(1, M_SMALL, 1, 256, seed=4).to(DEV)
    with pytest.raises(RuntimeError, match="no statistics-only kernel"):
        hip.conv2d_fwd(xw, wide, None, ops.conv_geometry(xw, wide, 1, 0), bn=(acc, ws), ldr=256,
                       w_split=ops.split_weights(wide), w_frag=ops.pack_weights(wide), stats_only=True)
    assert float(acc.abs().max()) == 0.0


# ------------------------------------------------------------------ 2. the regenerating block end
def _cases():
    out = []
    for K1, N1, N2 in SHAPES:
        for fmt in (1, 2):
            for skip in ("identity", "bn"):
                # both values of `center` and both statistics targets for every shape and format
                center = (skip == "identity") == (fmt == 2)
                target = "acc" if (skip == "identity") else "partial"
                out.append(pytest.param(K1, N1, N2, M_TILES, fmt, skip, center, target,
                                        id=f"{K1}-{N1}-{N2}-{'bf16x6' if fmt == 1 else 'f16x3'}-{skip}-"
                                           f"{'center' if center else 'nocenter'}-{target}"))
        out.append(pytest.param(K1, N1, N2, M_SMALL, 2, "identity", True, "acc",
                                id=f"{K1}-{N1}-{N2}-f16x3-identity-center-acc-m40"))
        out.append(pytest.param(K1, N1, N2, M_SMALL, 1, "bn", False, "partial",
                                id=f"{K1}-{N1}-{N2}-bf16x6-bn-nocenter-partial-m40"))
    return out


@pytest.mark.parametrize("K1,N1,N2,M,fmt,skip,center,target", _cases())
def test_regenerating_block_end_matches_the_old_pair(hip, operands, K1, N1, N2, M, fmt, skip, center,
                                                     target):
    M = rows_for(M, target)
    t, ref = operands(K1, N1, N2, M)
    pro2 = dict(in_scale=t["s2"], in_shift=t["t2"], in_center=t["c2"] if center else None, in_relu=True)
    pro3 = dict(in_scale=t["s3"], in_shift=t["t3"], in_center=t["c3"] if center else None, in_relu=True,
                x2=t["skip"])
    if skip == "bn":
        pro3.update(in2_scale=t["sk_s"], in2_shift=t["sk_t"], in2_center=t["sk_c"] if center else None)

    def block_end(x, **more):
        side = torch.full_like(t["skip"], float("nan"))
        if target == "acc":
            acc = torch.zeros((ops.BN_SHARDS, N2, 2), device=DEV, dtype=torch.float64)
            out = ops.conv2d_bn_sums(x, t["wn"], 1, 0, acc, side_out=side, **pro3, **more)
            kern = hip.conv2d_last_kernel()
            return out, side, moments_of_sums(hip, acc, M, N2), kern
        out, (partial, _, rows) = ops.conv2d_nhwc(x, t["wn"], 1, 0, want_stats=True, side_out=side, **pro3,
                                                  **more)
        return out, side, moments_of_partials(partial, M, rows), hip.conv2d_last_kernel()

    # the old pair: conv_s3_kernel stores raw3, the dual block end reads it -- on conv_u3_kernel
    # (Cout >= 256) or conv_x3_kernel, the two the flagship's block ends run on
    with hip.options(conv_math=fmt, m3=0, s3=2, u3=2, x3_tile=4):
        raw3 = ops.conv2d_nhwc(t["raw2"], t["w3"], 1, 0, **pro2)
        assert hip.conv2d_last_kernel().kernel == "conv_s3"
        out_old, side_old, mom_old, kern = block_end(raw3)
        assert kern.kernel == ("conv_u3" if N2 >= 256 else "conv_x3"), kern
    with hip.options(conv_math=fmt, s3_wgs=WGS):
        out_new, side_new, mom_new, kern = block_end(
            t["raw2"], regen=dict(w=t["w3"], in_scale=pro2["in_scale"], in_shift=pro2["in_shift"],
                                  in_center=pro2["in_center"], in_relu=True))
        assert kern == ConvKernel("p3", "conv_r3", fmt, K1, N2 // 32, 2 if skip == "bn" else 1)
    y64, out64 = ref["y", center, skip], ref["out", center, skip]
    figures = dict(side_new=rel_rms(side_new.reshape(M, N1), y64), side_old=rel_rms(side_old.reshape(M, N1), y64),
                   out_new=rel_rms(out_new.reshape(M, N2), out64), out_old=rel_rms(out_old.reshape(M, N2), out64),
                   new_vs_old=rel_rms(out_new, out_old),
                   side_differs=int((side_new != side_old).sum()))
    print(figures)
    # the regenerated values are the values the old route stored and read back: same MFMA sequence,
    # same epilogue operation order -> the block output is the same bits
    assert torch.equal(side_new, side_old), figures
    assert figures["side_new"] < BOUND and figures["out_new"] < BOUND, figures
    assert figures["out_old"] < BOUND, figures
    # same inputs (side_out is identical), two correct fp32 accumulation orders of the second product
    assert figures["new_vs_old"] < BOUND, figures
    check_moments(mom_new, out64, "second product, new route")
    check_moments(mom_old, out64, "second product, old route")


def test_regenerating_launch_rejects_what_it_cannot_do(hip, operands):
    t, _ = operands(64, 256, 64, M_SMALL)
    regen = dict(w=t["w3"], in_scale=t["s2"], in_shift=t["t2"], in_relu=True)
    side = torch.empty_like(t["skip"])
    with pytest.raises(RuntimeError, match="regen needs"):   # no skip / side_out handed in
        g = ops.conv_geometry(t["skip"], t["wn"], 1, 0)
        y = torch.empty(1, M_SMALL, 1, 64, device=DEV)
        hip.conv2d_fwd(None, t["wn"], y, g, in_scale=t["s3"], in_shift=t["t3"], in_relu=1, ldr=64,
                       w_frag=ops.pack_weights(t["wn"]), w_split=ops.split_weights(t["wn"]),
                       regen=dict(x=t["raw2"], w_frag=ops.pack_weights(t["w3"]), in_scale=t["s2"],
                                  in_shift=t["t2"], in_relu=1))
    w96 = rnd(96, 1, 1, 256, seed=21).to(DEV)     # Cout = 96: no instance
    with pytest.raises(RuntimeError, match="no instance"):
        ops.conv2d_nhwc(t["raw2"], w96, 1, 0, in_scale=t["s3"], in_shift=t["t3"], in_relu=True,
                        x2=t["skip"], side_out=side, regen=regen)


# ------------------------------------------------------------------ 3. the trunk
@pytest.mark.parametrize("graphs", ["0", "1"], ids=["eager", "graphs"])
def test_trunk_new_route_equals_old_route(hip, monkeypatch, graphs):
    """ResNet-50 RGB trunk_features, 2 environments x 64 x 64 frames, train-mode statistics: option
    "r3" = 2 (every block end of layers 1-2 regenerated) against "r3" = 0, four passes each -- with
    graphs: eager, capturing, two replays, new frames in every pass -- features per pass and every
    BatchNorm running statistic afterwards at the trunk parity tolerance (1e-5).
    At 512 / 128 rows the default dispatch would give the old route's conv3 and block ends to the
    small-launch kernels (conv_m3, the fp32-MFMA dual kernel), which the flagship's layers 1-2 never
    run on; BOTH arms therefore run under m3 = 0, s3 = 2, x3_tile = 4, so that the old arm is the
    pair the new route replaces -- conv_s3_kernel storing + the dual block end on conv_x3_kernel --
    and every other layer runs on the same kernel in both arms; and under igemm_no_splitk = 1,
    because the split-K kernel that m3 = 0 would otherwise hand the 3x3 layers to adds with fp32
    atomics: two runs of the SAME route then differ by 1.5e-7 behind the first 3x3 layer, and
    train-mode BatchNorm over the 8 pixels of layer 4 at this frame size amplifies that to 5e-5 .. 1e-4
    in the features (measured: both routes against themselves and against each other)."""
    from oracle import thirdparty as tp
    from vlnce_amd.encoders import resnet_encoders as enc

    monkeypatch.setenv("VLNCE_HIP_GRAPHS", graphs)
    g = torch.Generator().manual_seed(5)
    frames = [torch.randint(0, 256, (2, 64, 64, 3), generator=g).float().to(DEV) for _ in range(3)]
    frames = [frames[0], frames[0], frames[1], frames[2]]
    sd, runs, launched = None, {}, {}
    orig = ops.conv2d_bn_sums
    for mode in (0, 2):
        net = enc.TorchVisionResNet(128, resnet_version="resnet50", spatial_output=False,
                                    single_spatial_filter=False)
        sd = sd or tp.synth_state_dict(net)
        net.load_state_dict(sd)
        net.to(DEV).train()
        seen = []

        def counting(*a, **k):
            seen.append(("stats_only" if k.get("stats_only") else "regen" if k.get("regen") else "plain"))
            return orig(*a, **k)

        monkeypatch.setattr(ops, "conv2d_bn_sums", counting)
        with torch.no_grad(), hip.options(r3=mode, m3=0, s3=2, x3_tile=4, igemm_no_splitk=1):
            feats = [net.trunk_features({"rgb": f}).clone() for f in frames]
        monkeypatch.setattr(ops, "conv2d_bn_sums", orig)
        torch.cuda.synchronize()
        runs[mode] = (feats, {k: v.clone() for k, v in net.state_dict().items() if "running_" in k
                              or "num_batches" in k})
        launched[mode] = seen
    # 3 + 4 block ends of layers 1-2 per eager pass took the new route, none under r3 = 0
    passes = 4 if graphs == "0" else 2      # (replays launch nothing from Python)
    assert launched[0].count("regen") == 0 and launched[0].count("stats_only") == 0
    assert launched[2].count("regen") == 7 * passes and launched[2].count("stats_only") == 7 * passes
    for k, (a, b) in enumerate(zip(runs[2][0], runs[0][0])):
        assert bool(torch.isfinite(a).all())
        tk.close(a, b, 1e-5, what=f"features of pass {k}")
    assert runs[0][1].keys() == runs[2][1].keys() and len(runs[0][1]) > 100
    for k in runs[0][1]:
        tk.close(runs[2][1][k], runs[0][1][k], 1e-5, what=k)
