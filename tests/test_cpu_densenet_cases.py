"""CPU: the case tables of tests/densenet_cases.py have the edges they claim, and the references the GPU tests lean on are right:
the fp64 "deferred" restatement of the plan's BatchNorm-backward chain equals torch autograd through torch.cat, and every block and
transition of DensePlan at 224 and at 200 falls in a class the tables hold."""
import pytest
import torch

from densenet_cases import (ADAPTIVE_CASES, BLOCK_CASES, BN_SINGLE_STAGE_ROWS, GROWTH, MAXPOOL_CASES, SLICE_CASES, TAP_PAIRS, TRANS_CASES,
                            block_autograd, block_classes, block_deferred, block_eval_chain, block_id, block_inputs, block_param_slices, col_geom,
                            densenet_geometry, eval_buffers, maxpool_input, maxpool_reference, pad64, trans_autograd, trans_chain, trans_id, trans_reference)
from mbconv_cases import EPC
from mmskin import _lib


def _stage(gx):
    return "two-stage" if gx > BN_SINGLE_STAGE_ROWS else "single"


def test_block_rows_have_their_edges():
    by = {block_id(c): c for c in BLOCK_CASES}
    c = by["n2-c64-l3-7x5"]
    cins = [c.C0 + GROWTH * i for i in range(c.L)]
    assert cins == [64, 96, 128] and [pad64(x) for x in cins] == [64, 128, 128]
    rows = c.N * c.H * c.W
    assert rows == 70 and all(rows % t for t in (16, 32, 64, 128))
    c = by["n3-c128-l2-1x1"]
    assert c.N * c.H * c.W == 3
    assert by["n2-c64-l6-14x14"].L == 6
    c = by["n1-c256-l2-3x3"]
    assert c.C0 + GROWTH == 288 and pad64(288) == 320
    assert len(by) == len(BLOCK_CASES) == 4


def test_transition_rows_have_their_edges():
    a, b, c = TRANS_CASES
    assert (a.H % 2, a.W % 2) == (1, 1) and (a.H // 2, a.W // 2) == (3, 3) and a.pitch > a.C // 2
    assert sorted((b.H % 2, b.W % 2)) == [0, 1] and b.pitch > b.C // 2
    assert c.pitch == c.C // 2 and c.H % 2 == 0 and c.W % 2 == 0


def test_slice_rows_reach_each_finalize_branch():
    stages = set()
    for c in SLICE_CASES:
        rl, rbk, gx = col_geom(c.rows, c.C, EPC[c.dtype])
        assert c.c0 + c.C <= c.pitch and c.C % 8 == 0 and c.c0 % 8 == 0
        if "two-stage" in c.edge:
            assert gx > 512 and c.rows % rbk != 0, (c, gx, rbk)
        elif "64 <" in c.edge:
            assert 64 < gx <= 512, (c, gx)
        else:
            assert gx <= 2 and c.rows == 70 and c.rows % rbk != 0
        stages.add((c.dtype, _stage(gx)))
    assert {("fp32", "two-stage"), ("bf16", "two-stage"), ("fp32", "single"), ("bf16", "single")} <= stages
    # the two-stage rows sit just above the threshold of their dtype: one fewer chunk row block and the branch is not taken
    assert col_geom(65536, 32, 4)[2] == 512 and col_geom(131072, 32, 8)[2] == 512


def test_maxpool_rows_plant_equal_maxima_at_every_pair_of_taps():
    assert (1, 64, 7, 5) in MAXPOOL_CASES and (2, 64, 2, 2) in MAXPOOL_CASES and (2, 64, 6, 6) in MAXPOOL_CASES
    assert len(TAP_PAIRS) == 6
    for N, C, H, W in MAXPOOL_CASES:
        y, plants = maxpool_input(N, C, H, W)
        assert float(y.min()) == 0.0 and float((y == 0).float().mean()) > 0.2 and torch.equal(y, y.bfloat16().float())
        pooled, tap = maxpool_reference(y)
        pairs = set()
        for n, c, ph, pw, first in plants:
            win = y[n, c, 2 * ph:2 * ph + 2, 2 * pw:2 * pw + 2].reshape(-1)
            tied = [i for i in range(4) if win[i] == win.max()]
            assert len(tied) >= 2 and tied[0] == first == int(tap[n, c, ph, pw])   # torch takes the first maximum, row-major
            pairs.add(tuple(tied))
        assert set(TAP_PAIRS) <= pairs and (0, 1, 2, 3) in pairs


def test_adaptive_rows_cover_every_bin_regime():
    def bins(n):
        return [(i * n // 7, -(-(i + 1) * n // 7)) for i in range(7)]
    shapes = {(H, W) for _, _, H, W in ADAPTIVE_CASES}
    assert {(2, 2), (3, 3), (7, 7), (10, 10), (9, 12), (14, 14)} <= shapes
    assert all(b - a == 1 for a, b in bins(7)) and all(b - a == 2 for a, b in bins(14))
    assert any(bins(10)[i][1] > bins(10)[i + 1][0] for i in range(6))            # overlapping bins on a map larger than 7
    assert len({b - a for a, b in bins(10)}) > 1                                  # of more than one size
    assert bins(2)[3] == (0, 2)                                                   # bins larger than a pixel's share of the map
    # the kernels are scalar per element: no alignment requirement on C, so one row is a multiple of neither chunk width
    assert any(C % 4 and C % 8 for _, C, _, _ in ADAPTIVE_CASES) and any(C == 24 for _, C, _, _ in ADAPTIVE_CASES)


@pytest.mark.parametrize("case", BLOCK_CASES, ids=block_id)
def test_deferred_restatement_equals_autograd_through_cat(case):
    """fp64: the plan's algebraic rewrite (cB / cC of every consumer summed as coefficients, applied once per channel) against autograd"""
    x, dcat, params = block_inputs(case)
    ref = block_autograd(case, x, dcat, params)
    got = block_deferred(case, x, dcat, params)
    for name in ("cat", "table", "dx", "grads"):
        err = float((got[name] - ref[name]).abs().max() / ref[name].abs().max())
        assert err < 1e-10, (name, err)


def test_eval_restatement_equals_the_eval_reference():
    """fp64: norm2 folded into conv1's weights and epilogue is the eval-mode layer"""
    case = BLOCK_CASES[0]
    x, dcat, params = block_inputs(case)
    bufs = eval_buffers(case)
    ref = block_autograd(case, x, dcat, params, training=False, buffers=bufs)
    got = block_eval_chain(case, x, params, bufs)
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-10


@pytest.mark.parametrize("case", TRANS_CASES, ids=trans_id)
def test_transition_restatement_equals_autograd(case):
    """the restated chain with the batch statistics in fp64 (the GPU test hands the kernel, and the reference, the table rounded to fp32)"""
    r = trans_reference(case)
    ref = trans_autograd(case, r["x"], r["dnext"], r["params"])
    xd = r["x"].double()
    table = torch.cat([xd.mean((0, 2, 3)), xd.var((0, 2, 3), unbiased=False)])
    got = trans_chain(case, r["x"], r["dnext"], r["params"], table)
    for name in ("pooled", "dx", "grads"):
        err = float((got[name] - ref[name]).abs().max() / ref[name].abs().max())
        assert err < 1e-10, (name, err)
    # odd maps: the last row / column is outside every pooling window, so the gradient that reaches the BatchNorm backward is exactly zero
    # there (dx itself is not: batch statistics add cB * x + cC to every pixel) -- the GPU test judges those borders on their own
    if case.H % 2:
        assert float(got["dz"][:, :, -1].abs().max()) == 0.0 and float(got["dz"][:, :, :-1].abs().max()) > 0
    if case.W % 2:
        assert float(got["dz"][:, :, :, -1].abs().max()) == 0.0


def test_every_block_and_transition_of_the_plan_falls_in_a_covered_class():
    have_blocks = set().union(*(block_classes(c.C0, c.L) for c in BLOCK_CASES))
    have_trans = {("odd" if (c.H % 2 or c.W % 2) else "even") for c in TRANS_CASES}
    have_stats = {(c.dtype, _stage(col_geom(c.rows, c.C, EPC[c.dtype])[2])) for c in SLICE_CASES}
    for size, batch in ((224, 256), (200, 256), (224, 2), (200, 2)):
        blocks, trans = densenet_geometry(size)
        for C0, L, H, W in blocks:
            assert block_classes(C0, L) <= have_blocks, (size, C0, L)
            for dtype in ("fp32", "bf16"):   # the block input's statistics: slice_stats over batch * H * W rows
                assert (dtype, _stage(col_geom(batch * H * W, C0, EPC[dtype])[2])) in have_stats, (size, batch, C0, dtype)
        for C, H, W in trans:
            assert ("odd" if H % 2 else "even") in have_trans, (size, C, H)
    assert [b[2] for b in densenet_geometry(224)[0]] == [56, 28, 14, 7] and [b[2] for b in densenet_geometry(200)[0]] == [50, 25, 12, 6]
    assert [t[0] for t in densenet_geometry(224)[1]] == [256, 512, 1280]
    assert any(t[1] % 2 for t in densenet_geometry(200)[1])                      # 25 -> 12: the plan does pool an odd map at 200


def test_param_numel_matches_the_library():
    lib = _lib.load()
    for c in BLOCK_CASES:
        assert lib.mmskin_dense_block_param_numel(c.C0, c.L) == block_param_slices(c.C0, c.L)[1]
