"""-m gpu: the GroupNorm(8, C) + ReLU (+ 2x2 max-pool) kernels of csrc/groupnorm.hip on their own, through mmskin_groupnorm8_relu_*, against
plain torch in fp64 on the CPU.  Cases, inputs and references: tests/groupnorm_cases.py (checked on the CPU by test_cpu_groupnorm_cases.py).

fp32: every tensor is at most 3x as far (relative L2) from fp64 as torch's CPU fp32 is, plus 1e-6; mean and rstd are fp32 in both element
types and keep that bound.  bf16: relative L2 against fp64 at most 1.25x the emulation's (fp32 arithmetic, each stored tensor rounded once)
plus 1e-4.  The argmax bytes and the ReLU mask are compared element by element: exactly in fp32 (the inputs keep every decision MARGIN away
from a rounding), outside the BF16_MARGIN exclusions in bf16."""
import pytest
import torch

import groupnorm_cases as G
from gpu_util import DEV, DT, ws
from mmskin import _lib
from mmskin._lib import call, ptr, stream

pytestmark = pytest.mark.gpu


def run(shape, pool, dtype, y, gamma, beta, gout, groups=G.GROUPS):
    N, C, H, W = shape
    oh, ow = (H // 2, W // 2) if pool else (H, W)
    lib = _lib.load()
    wsp = ws(lib.mmskin_groupnorm8_relu_workspace_bytes(N, C, H, W, groups, pool))
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    o = dict(out=nan(N, C, oh, ow), mean=nan(N, 8), rstd=nan(N, 8), dy=nan(N, C, H, W), dgamma=nan(C), dbeta=nan(C),
             idx=torch.full((N, oh, ow, C), 255, dtype=torch.uint8, device=DEV))
    yd, gd, bd, god = (t.to(DEV) for t in (y, gamma, beta, gout))
    call("mmskin_groupnorm8_relu_forward", ptr(yd), ptr(gd), ptr(bd), ptr(o["out"]), ptr(o["idx"]), ptr(o["mean"]), ptr(o["rstd"]), N, C, H, W,
         groups, pool, G.EPS, DT[dtype], ptr(wsp), stream())
    call("mmskin_groupnorm8_relu_backward", ptr(god), ptr(yd), ptr(gd), ptr(bd), ptr(o["dy"]), ptr(o["dgamma"]), ptr(o["dbeta"]), N, C, H, W,
         groups, pool, G.EPS, DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def check(shape, pool, dtype, conditioning=False, names=("mean", "rstd", "out", "dy", "dgamma", "dbeta")):
    y, gamma, beta, gout = G.inputs(shape, pool, conditioning)
    r64, r32, emu = G.references(shape, pool, conditioning)
    o = run(shape, pool, dtype, y, gamma, beta, gout)
    for k, v in o.items():   # every output element is written
        assert not bool(torch.isnan(v).any()) if v.is_floating_point() else (not pool or int(v.max()) < 4), f"{k}: an element was not written"
    figures = {}
    for k in names:
        hip, cpu, em = G.rel_l2(o[k], r64[k]), G.rel_l2(r32[k], r64[k]), G.rel_l2(emu[k], r64[k])
        figures[k] = (hip, cpu, em)
        print(f"{G.case_id(shape)} pool={pool} {dtype} {k}: hip {hip:.3e} cpu-fp32 {cpu:.3e} emulation {em:.3e}")
    for k, (hip, cpu, em) in figures.items():
        if dtype == "fp32" or k in ("mean", "rstd"):
            assert hip <= 3 * cpu + 1e-6, (k, hip, cpu)
        else:
            assert hip <= 1.25 * em + 1e-4, (k, hip, em)
    # decisions, element by element
    near_zero, near_tie = G.excluded(r64, pool, G.BF16_MARGIN if dtype == "bf16" else 0.0)
    assert float(near_zero.float().mean()) <= G.EXCLUDED_CAP
    if pool:
        assert float(near_tie.float().mean()) <= G.EXCLUDED_CAP
        tap = o["idx"].permute(0, 3, 1, 2).long()
        assert bool(((tap == r64["tap"]) | near_tie).all()), "argmax byte"
    else:   # the ReLU mask of the stored z
        assert bool((((o["out"] > 0) == (r64["pre"] > 0)) | near_zero).all()), "forward ReLU mask"
    # the backward's recomputed mask: where the fp64 gradient at z is zero, dy is the group's mean terms alone, i.e. what dy would be without
    # the element's own gamma * dz * rstd term.  Checked through dy itself: a flipped bit moves the element by |gamma * gout * rstd| = O(1).
    moved = (o["dy"].double() - r64["dy"]).abs() > (0.05 if dtype == "bf16" else 1e-3) * (1 + r64["dy"].abs())
    if pool:
        N, C, H, W = shape
        tie_in = torch.zeros_like(near_zero)
        tie_in[:, :, :2 * (H // 2), :2 * (W // 2)] = near_tie.repeat_interleave(2, 2).repeat_interleave(2, 3)
        near_zero = near_zero | tie_in
    assert not bool((moved & ~near_zero).any()), "backward ReLU mask / gradient routing"
    return o


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("shape", G.SMALL_SHAPES, ids=G.case_id)
def test_groupnorm_relu_pool_against_fp64(shape, pool, dtype):
    o = check(shape, pool, dtype)
    N, C, H, W = shape
    if pool and (H % 2 or W % 2):   # the dropped row / column receives no routed gradient: its dy is the mean terms of its group alone
        y, gamma, beta, gout = G.inputs(shape, pool)
        r64 = G.references(shape, pool)[0]
        edge = torch.zeros(N, C, H, W, dtype=torch.bool)
        edge[:, :, 2 * (H // 2):] = True
        edge[:, :, :, 2 * (W // 2):] = True
        assert G.rel_l2(o["dy"][edge], r64["dy"][edge]) <= (4e-3 if dtype == "bf16" else 1e-4)   # bf16: one rounding, 2^-9


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("pool", [0, 1])
def test_statistics_span_several_workgroups(pool, dtype):
    check(G.LARGE_SHAPE, pool, dtype)


@pytest.mark.parametrize("pool", [0, 1])
def test_conditioning_mean_50_std_1(pool):
    """A single-pass fp32 sum of squares loses the variance here (E[x^2] = 2501 against a variance of 1)."""
    check(G.CONDITIONING_SHAPE, pool, "fp32", conditioning=True, names=("rstd", "dy"))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_launches_are_bitwise_equal(dtype):
    for shape in (G.LARGE_SHAPE, (3, 256, 7, 9)):
        args = G.inputs(shape, 1)
        a, b = run(shape, 1, dtype, *args), run(shape, 1, dtype, *args)
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_refused_arguments_launch_nothing():
    lib = _lib.load()
    t = torch.zeros(1 << 16, device=DEV)
    out = torch.full((1 << 16,), 5.0, device=DEV)
    idx = torch.full((1 << 16,), 9, dtype=torch.uint8, device=DEV)
    big = ws(1 << 22)
    for (N, C, H, W, groups, pool), code in (((1, 96, 4, 4, 8, 0), 3), ((1, 64, 4, 4, 4, 1), 3), ((1, 32, 4, 4, 8, 0), 3), ((1, 64, 1, 4, 8, 1), 1)):
        assert lib.mmskin_groupnorm8_relu_workspace_bytes(N, C, H, W, groups, pool) == -1
        with pytest.raises(_lib.MMSkinError, match=f"error {code}"):
            call("mmskin_groupnorm8_relu_forward", ptr(t), ptr(t), ptr(t), ptr(out), ptr(idx), ptr(out), ptr(out), N, C, H, W, groups, pool,
                 G.EPS, DT["fp32"], ptr(big), stream())
        with pytest.raises(_lib.MMSkinError, match=f"error {code}"):
            call("mmskin_groupnorm8_relu_backward", ptr(t), ptr(t), ptr(t), ptr(t), ptr(out), ptr(out), ptr(out), N, C, H, W, groups, pool,
                 G.EPS, DT["bf16"], ptr(big), stream())
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((idx == 9).all()), "a refused call wrote to an output"
