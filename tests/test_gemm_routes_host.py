"""CPU tier of tests/test_gemm_routes_gpu.py: the route table against the dispatch mirror
(tests/gemm_dispatch.py), and the two error statistics against planted defects -- a bound that no
defect can break is decoration.  No GPU, no library call."""
import pytest
import torch

import gemm_dispatch as gd
import test_gemm_routes_gpu as gr
from gemm_dispatch import Call
from vlnce_amd._lib import GemmKernel, decode_gemm_kernel


def test_route_table_lists_every_route():
    """the table against the instantiations vlnce_gemm can reach (gemm_dispatch.reachable(), read off
    dispatch_tiles / dispatch_small and the six branches of the entry point), and against the mirror:
    each (call, options) pair lands where the table says"""
    have = {(r.want[0], r.want[1], r.want[2], r.want[3] > 1) for r in gr.ROUTES}
    assert have == gd.reachable(), (sorted(gd.reachable() - have), sorted(have - gd.reachable()))
    for r in gr.ROUTES + gr.FOLDS + gr.EDGES:
        assert gd.expected(r.call, **r.opts) == gr.want_kernel(r), (r, gd.expected(r.call, **r.opts))
        assert 2.0 * r.call.M * r.call.N * r.call.K <= 1.1e9, r      # nothing above the long-reduction row
        assert r.call.ldc > r.call.N                                   # guard columns
    assert {r.call.M > 1024 and r.call.M % 1024 != 0 for r in gr.FOLDS} == {True}
    rows = gr.ROUTES + gr.FOLDS + gr.EDGES
    assert len({r.name for r in rows}) == len(rows)
    # the default tile choice (no option) reaches all three tiles, the split factor every constant
    assert {gd.expected(r.call).tile for r in gr.EDGES} == set(gd.TILES.values())
    assert {r.want[3] for r in gr.EDGES} >= {1, 3, 4, 11, 64}


def test_matrix_covers_both_epilogues_and_both_split_outcomes():
    T64 = (64, 64)
    for bn, base in gr.BASES:
        assert {gd.epilogue_is_vectorised(c) for _, c in gr.cells(base)} == {True, False}, bn
    recs = {n: gd.expected(c) for n, c in gr.MATRIX}
    assert recs["buf-act0+shift"] == GemmKernel("buf", "buf", T64, 1, False, False)
    assert recs["scalar-act2+shift"] == GemmKernel("s", "nk_s", T64, 1, False, False)
    assert recs["split-act1+shift"] == GemmKernel("buf", "buf", T64, 8, True, True)
    assert recs["split-accumulate"] == GemmKernel("buf", "buf", T64, 8, False, False)       # no zero-fill
    assert recs["split-accumulate+shift"] == GemmKernel("buf", "buf", T64, 8, False, True)
    assert recs["split-accumulate+relu+shift"].splitk == 1                                   # C += act(...)
    assert recs["split-scale+shift"].splitk == 1 and recs["split-residual-ldr=N"].splitk == 1


def test_mirror_rules_at_their_thresholds():
    """choose_splitk / choose_tile / buf_ok one step either side of each constant of igemm.hip"""
    sk = gd.choose_splitk
    assert sk(70, 52, 7 * 32, False) == 1 and sk(70, 52, 7 * 32 + 1, False) == 4            # KT < 8
    assert sk(64 * 127, 64, 512, False) == 3 and sk(64 * 128, 64, 512, False) == 1            # tiles >= 128
    assert sk(64, 64, 64 * 128, False) == 64 and sk(64, 64, 3200, False) == 50                # at most 64, KT / 2
    assert sk(70, 52, 512, False, no_splitk=1) == 1
    assert sk(512, 1024, 1024, True) == 8 and sk(512, 1024, 1024, False) == 1                 # transA's rule
    assert sk(512, 1024, 1023 - 31, True) == 1                                                # KT = 31
    assert sk(512, 1024 - 64, 1024, True) == 3                                                # 120 tiles: ordinary rule
    assert sk(64 * 32, 64 * 32, 1024, True) == 1                                              # 1024 tiles
    assert gd.choose_tile(128 * 16, 128 * 32) == (128, 128)
    assert gd.choose_tile(128 * 16, 128 * 32 - 128) == (128, 64)
    assert gd.choose_tile(64 * 512, 64) == (64, 64) and gd.choose_tile(70, 52, 1) == (128, 128)
    # a_bytes = ((M - 1) lda + K) 4 just below / just past 2^31 - 1: no buffer descriptor beyond
    assert gd.expected(Call(70, 52, 64, lda=7780736)).a == "buf"
    assert gd.expected(Call(70, 52, 64, lda=7780740)).a == "v4"
    assert decode_gemm_kernel(-1) is None
    assert decode_gemm_kernel(0 | 3 << 2 | 2 << 4 | 1 << 6 | 1 << 7 | 24 << 8) == \
        GemmKernel("buf", "kn", (128, 64), 24, True, True)


# ------------------------------------------------------------------ the statistics must be able to fail
def _fp32_product(c):
    """the undamaged fp32 result of a table row's call, its fp64 reference and the CPU contract"""
    op = gr.operands(c)
    A = op["t"]["A"].as_strided((c.M, c.K), (c.lda, 1))
    B = op["t"]["B"].as_strided((c.N, c.K), (c.ldb, 1)).t()
    return A, B, A @ B, op["ref"], op["sim"]


def _row(name):
    (r,) = [r for r in gr.ROUTES if r.name == name]
    assert not r.call.transA and not r.call.transB
    return r.call


def test_undamaged_fp32_products_break_no_bound():
    for name in ("s-K50", "s-K323-split5", "buf-split8"):
        c = _row(name)
        A, B, y, ref, sim = _fp32_product(c)
        assert gr.bounds_broken(y, ref, sim)[0] == []
        # ... nor does the same product added up in eight K ranges, as a split launch does
        step = -(-c.K // 8)
        y8 = sum(A[:, k:k + step] @ B[k:k + step] for k in range(0, c.K, step))
        assert gr.bounds_broken(y8, ref, sim)[0] == [], name


@pytest.mark.parametrize("name", ["s-K50", "s-K323-split5"])
def test_dropped_last_k_in_one_block_breaks_a_bound(name):
    """a loader that loses the last k of a ragged K, in one 32 x 32 block only"""
    c = _row(name)
    A, B, y, ref, sim = _fp32_product(c)
    y = y.clone()
    y[32:64, 0:32] -= A[32:64, c.K - 1:] @ B[c.K - 1:, 0:32]
    broken, rms, blk, blk32 = gr.bounds_broken(y, ref, sim)
    assert "block" in broken and "rms" in broken, (broken, rms, blk, blk32)


def test_missing_split_range_in_one_tile_breaks_a_bound():
    """one K range of eight never added, in the ragged 6-row tail tile only"""
    c = _row("buf-split8")
    A, B, y, ref, sim = _fp32_product(c)
    y = y.clone()
    y[64:, :] -= A[64:, 192:256] @ B[192:256, :]
    broken, rms, blk, blk32 = gr.bounds_broken(y, ref, sim)
    assert "block" in broken and "rms" in broken, (broken, rms, blk, blk32)


def test_shifted_output_column_breaks_a_bound():
    """the last column of the tail tile stored one column to the left (what the guard band cannot see)"""
    c = _row("buf-plain")
    A, B, y, ref, sim = _fp32_product(c)
    y = y.clone()
    y[:, c.N - 2] = y[:, c.N - 1]
    broken, rms, blk, blk32 = gr.bounds_broken(y, ref, sim)
    assert "block" in broken and "rms" in broken, (broken, rms, blk, blk32)


def test_a_defect_of_one_part_in_a_thousand_in_one_block_breaks_the_block_bound():
    """the smallest defect of the table's largest row: one k of 1024 lost in one 32 x 32 block of
    16 x 32 -- three orders of magnitude above both bounds"""
    c = Call(512, 1024, 1024)
    g = torch.Generator().manual_seed(5)
    A, B = torch.randn(c.M, c.K, generator=g) * c.K ** -0.5, torch.randn(c.K, c.N, generator=g)
    ref, sim = A.double() @ B.double(), A @ B
    y = sim.clone()
    y[480:512, 992:1024] -= A[480:512, -1:] @ B[-1:, 992:1024]
    broken, rms, blk, blk32 = gr.bounds_broken(y, ref, sim)
    assert broken == ["rms", "block"] and blk > 1000 * blk32, (broken, rms, blk, blk32)
