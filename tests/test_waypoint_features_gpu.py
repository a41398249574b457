"""GPU tier: vlnce_waypoint_feature_pick / vlnce_waypoint_feature_rows (csrc/waypoint_features.hip) on
the MI355X, bit for bit against their restatement in plain torch (tests/waypoint_features_ref.py).
F = 6 (no 16-byte path), 2048 (the depth trunk's real row), 4100 (crosses a 4096-element chunk, with a
4-element tail) -- the three as three fields of ONE launch; B in {1, 3}; P in {1, 12}; the source
contiguous, a slice of a larger arena, and with its base advanced by one element (which forces the
element path for every F).  `zero` holds distinct non-zero values; every output sits between guard
bands."""
import pytest
import torch

import waypoint_features_ref as wf
from vlnce_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FS = (6, 2048, 4100)
GUARD = 64
SENTINEL = -77.0


def source(shape, kind, g):
    """an fp32 tensor of `shape` [B, ...] on the device laid out as `kind` says, and its CPU copy"""
    B = shape[0]
    host = torch.randint(1, 1000, shape, generator=g).float()
    if kind == "contiguous":
        dev = host.to(DEV)
    elif kind == "arena-slice":      # row stride three rows
        arena = torch.full((B, 3) + tuple(shape[1:]), SENTINEL, device=DEV)
        arena[:, 1] = host.to(DEV)
        dev = arena[:, 1]
        assert B == 1 or not dev.is_contiguous()
    else:                            # the base one element behind a 16-byte boundary
        flat = torch.full((host.numel() + 1,), SENTINEL, device=DEV)
        flat[1:] = host.to(DEV).reshape(-1)
        dev = flat[1:].view(shape)
        assert dev.data_ptr() % 16 == 4
    assert dev.shape == tuple(shape) and dev[0].is_contiguous()
    return dev, host


def banded(shape):
    """a contiguous output of `shape` with GUARD sentinel elements on either side"""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
    return whole, whole[GUARD:GUARD + n].view(shape)


def bands_untouched(whole):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all())


def zero_rows(F):
    return -(torch.arange(F, dtype=torch.float32) + 1.0)      # distinct, non-zero, unlike any source value


def pano_patterns(B, P):
    values = [0, P - 1, P, P + 3, -1]
    if B == 1:
        return [[v] for v in values]
    return [values[:3], [values[3], values[4], 0], [P, P, P]]


KINDS = ["contiguous", "arena-slice", "offset-base"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", [1, 12])
@pytest.mark.parametrize("B", [1, 3])
def test_feature_pick_bit_for_bit(B, P, kind):
    lib = _lib.get_lib()
    g = torch.Generator().manual_seed(100 * B + P)
    srcs = [source((B, P, F), kind, g) for F in FS]
    zeros = [zero_rows(F) for F in FS]
    for pattern in pano_patterns(B, P):
        pano = torch.tensor(pattern, dtype=torch.int64)
        outs = [banded((B, F)) for F in FS]
        lib.waypoint_feature_pick([(dev, z.to(DEV), dst) for (dev, _), z, (_, dst) in zip(srcs, zeros, outs)],
                                  pano.to(DEV), B, P)
        torch.cuda.synchronize()
        for (_, host), z, (whole, dst), F in zip(srcs, zeros, outs, FS):
            want = wf.feature_pick_ref(host, z, pano)
            assert torch.equal(dst.cpu(), want), (F, pattern)
            assert bands_untouched(whole), (F, pattern)
            for b, p in enumerate(pattern):      # "zeros" and `zero` cannot be confused
                assert bool((dst[b] < 0).all()) == (not 0 <= p < P), (F, pattern, b)


def mask_patterns(B):
    return [[0] * B, [1] * B] + ([[1, 0, 1], [0, 0, 1]] if B > 1 else [])


@pytest.mark.parametrize("mask_dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", [1, 12])
@pytest.mark.parametrize("B", [1, 3])
def test_feature_rows_bit_for_bit(B, P, kind, mask_dtype):
    lib = _lib.get_lib()
    g = torch.Generator().manual_seed(200 * B + P)
    panos = [source((B, P, F), kind, g) for F in FS]
    hists = [source((B, F), kind, g) for F in FS]
    zeros = [zero_rows(F) for F in FS]
    for pattern in mask_patterns(B):
        masks = torch.tensor(pattern).to(mask_dtype)
        if mask_dtype == torch.float32 and any(pattern):
            masks = masks * 0.25                  # any non-zero value is "not done"
        outs = [banded((B, P + 1, F)) for F in FS]
        lib.waypoint_feature_rows([(p, h, z.to(DEV), out) for (p, _), (h, _), z, (_, out)
                                   in zip(panos, hists, zeros, outs)], masks.to(DEV), B, P)
        torch.cuda.synchronize()
        for (_, ph), (_, hh), z, (whole, out), F in zip(panos, hists, zeros, outs, FS):
            want = wf.feature_rows_ref(ph, hh, z, masks)
            assert torch.equal(out.cpu(), want), (F, pattern)
            assert bands_untouched(whole), (F, pattern)
            for b, m in enumerate(pattern):
                assert bool((out[b, P] < 0).all()) == (m == 0), (F, pattern, b)


def test_masks_as_the_storage_and_the_net_hold_them():
    """[B, 1] uint8 (the storage's arena row) and [B, 1] fp32 (what the trainer's batch carries) go
    through the binding as they are; two fields of different F in one launch"""
    lib = _lib.get_lib()
    B, P = 3, 12
    g = torch.Generator().manual_seed(9)
    for masks in (torch.tensor([[1], [0], [1]], dtype=torch.uint8), torch.tensor([[0.0], [1.0], [1.0]])):
        fields, want = [], []
        for F in (2048, 8192):
            p, ph = source((B, P, F), "contiguous", g)
            h, hh = source((B, F), "arena-slice", g)
            z = zero_rows(F)
            whole, out = banded((B, P + 1, F))
            fields.append((p, h, z.to(DEV), out))
            want.append((wf.feature_rows_ref(ph, hh, z, masks), whole, out))
        lib.waypoint_feature_rows(fields, masks.to(DEV).reshape(-1), B, P)
        torch.cuda.synchronize()
        for ref, whole, out in want:
            assert torch.equal(out.cpu(), ref) and bands_untouched(whole)


def test_refused_calls_launch_nothing():
    lib = _lib.get_lib()
    B, P, F = 2, 12, 8
    src = torch.ones(B, P, F, device=DEV)
    zero, hist = torch.ones(F, device=DEV), torch.ones(B, F, device=DEV)
    dst, out = torch.zeros(B, F, device=DEV), torch.zeros(B, P + 1, F, device=DEV)
    pano = torch.zeros(B, device=DEV, dtype=torch.int64)
    masks = torch.ones(B, device=DEV, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="9 fields"):
        lib.waypoint_feature_pick([(src, zero, dst)] * 9, pano, B, P)
    with pytest.raises(RuntimeError, match="9 fields"):
        lib.waypoint_feature_rows([(src, hist, zero, out)] * 9, masks, B, P)
    torch.cuda.synchronize()
    assert float(dst.abs().sum()) == 0.0 and float(out.abs().sum()) == 0.0
