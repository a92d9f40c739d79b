"""-m gpu: the DynamicCNN trunk's tail -- GroupNorm(8, C) + ReLU (+ 2x2 max-pool) + global average in one kernel pair (csrc/groupnorm.hip,
gn8_relu_gap_apply / gn8_relu_gap_backward) -- through mmskin_groupnorm8_relu_gap_*, against plain torch in fp64 on the CPU and against the
un-fused chain (mmskin_groupnorm8_relu_forward, a mean in torch, mmskin_groupnorm8_relu_backward on the broadcast gradient).

Shapes, y, gamma and beta: tests/groupnorm_cases.py (SMALL_SHAPES with their odd maps, and the conditioning case).  The upstream gradient is
dfeat = g * OH * OW with g bf16-representable, so the gradient at the activation, dfeat / (OH * OW), is the same number on every path.

Bounds: those of tests/test_gpu_groupnorm_ops.py.  fp32, and the fp32 tensors feat / mean / rstd in both element types: relative L2 against
fp64 at most 3x torch CPU fp32's own, plus 1e-6.  bf16 (dy, dgamma, dbeta): at most 1.25x the emulation's (fp32 arithmetic, each stored
tensor rounded once; the only stored tensor here is dy) plus 1e-4.  The fused and un-fused results differ by no more than those bounds.
Decisions (ReLU mask, recomputed argmax) are checked through dy, outside groupnorm_cases' exclusions (none in fp32)."""
import functools

import pytest
import torch

import groupnorm_cases as G
from gpu_util import DEV, DT, ws
from mmskin import _lib
from mmskin._lib import call, ptr, stream

pytestmark = pytest.mark.gpu
NAMES = ("feat", "mean", "rstd", "dy", "dgamma", "dbeta")


def out_hw(shape, pool):
    return (shape[2] // 2, shape[3] // 2) if pool else (shape[2], shape[3])


@functools.lru_cache(maxsize=None)
def gap_inputs(shape, pool, conditioning=False):
    """y, gamma, beta of groupnorm_cases; g [N, C] bf16-representable: the gradient at every element of the (pooled) activation"""
    y, gamma, beta, _ = G.inputs(shape, pool, conditioning)
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(77 + 1000 * C + 10 * H + W + pool)
    g = G.rb(torch.randn(N, C, generator=gen))
    oh, ow = out_hw(shape, pool)
    return y, gamma, beta, g, (g.double() * (oh * ow)).float()     # exact: 8 significant bits times an integer below 2^11


@functools.lru_cache(maxsize=None)
def gap_references(shape, pool, conditioning=False):
    """fp64, CPU fp32 and the bf16 emulation, each with feat = the mean of its un-rounded activation"""
    y, gamma, beta, g, _ = gap_inputs(shape, pool, conditioning)
    oh, ow = out_hw(shape, pool)
    gout = g.double()[:, :, None, None].expand(-1, -1, oh, ow)
    refs = []
    for dtype, store in ((torch.float64, None), (torch.float32, None), (torch.float32, G.rb)):
        r = G.reference(y, gamma, beta, gout, pool, dtype, store=store)
        plain = r if store is None else refs[1]                    # feat is fp32 and never stored in bf16
        r["feat"] = plain["out"].mean(dim=(2, 3))
        refs.append(r)
    return tuple(refs)


def nan(*s):
    return torch.full(s, float("nan"), device=DEV)


def run_fused(shape, pool, dtype, y, gamma, beta, dfeat, groups=G.GROUPS):
    N, C, H, W = shape
    wsp = ws(_lib.load().mmskin_groupnorm8_relu_gap_workspace_bytes(N, C, H, W, groups, pool))
    o = dict(feat=nan(N, C), mean=nan(N, 8), rstd=nan(N, 8), dy=nan(N, C, H, W), dgamma=nan(C), dbeta=nan(C))
    yd, gd, bd, dfd = (t.to(DEV) for t in (y, gamma, beta, dfeat))
    call("mmskin_groupnorm8_relu_gap_forward", ptr(yd), ptr(gd), ptr(bd), ptr(o["feat"]), ptr(o["mean"]), ptr(o["rstd"]), N, C, H, W, groups, pool,
         G.EPS, DT[dtype], ptr(wsp), stream())
    call("mmskin_groupnorm8_relu_gap_backward", ptr(dfd), ptr(yd), ptr(gd), ptr(bd), ptr(o["dy"]), ptr(o["dgamma"]), ptr(o["dbeta"]), N, C, H, W,
         groups, pool, G.EPS, DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def run_unfused(shape, pool, dtype, y, gamma, beta, g):
    N, C, H, W = shape
    oh, ow = out_hw(shape, pool)
    wsp = ws(_lib.load().mmskin_groupnorm8_relu_workspace_bytes(N, C, H, W, G.GROUPS, pool))
    o = dict(out=nan(N, C, oh, ow), mean=nan(N, 8), rstd=nan(N, 8), dy=nan(N, C, H, W), dgamma=nan(C), dbeta=nan(C))
    idx = torch.full((N, oh, ow, C), 255, dtype=torch.uint8, device=DEV)
    yd, gd, bd = (t.to(DEV) for t in (y, gamma, beta))
    god = g[:, :, None, None].expand(-1, -1, oh, ow).contiguous().to(DEV)
    call("mmskin_groupnorm8_relu_forward", ptr(yd), ptr(gd), ptr(bd), ptr(o["out"]), ptr(idx), ptr(o["mean"]), ptr(o["rstd"]), N, C, H, W,
         G.GROUPS, pool, G.EPS, DT[dtype], ptr(wsp), stream())
    call("mmskin_groupnorm8_relu_backward", ptr(god), ptr(yd), ptr(gd), ptr(bd), ptr(o["dy"]), ptr(o["dgamma"]), ptr(o["dbeta"]), N, C, H, W,
         G.GROUPS, pool, G.EPS, DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    o = {k: v.cpu() for k, v in o.items()}
    o["feat"] = o["out"].double().mean(dim=(2, 3))
    return o


def bound(k, dtype, cpu, em):
    return 3 * cpu + 1e-6 if dtype == "fp32" or k in ("feat", "mean", "rstd") else 1.25 * em + 1e-4


def check(shape, pool, dtype, conditioning=False, names=NAMES):
    y, gamma, beta, g, dfeat = gap_inputs(shape, pool, conditioning)
    r64, r32, emu = gap_references(shape, pool, conditioning)
    o = run_fused(shape, pool, dtype, y, gamma, beta, dfeat)
    u = run_unfused(shape, pool, dtype, y, gamma, beta, g)
    for k, v in o.items():   # every output element is written
        assert bool(torch.isfinite(v).all()), f"{k}: an element was not written, or is not finite"
    figures = {}
    for k in names:
        hip, cpu, em, chain = G.rel_l2(o[k], r64[k]), G.rel_l2(r32[k], r64[k]), G.rel_l2(emu[k], r64[k]), G.rel_l2(o[k], u[k])
        figures[k] = (hip, cpu, em, chain)
        print(f"{G.case_id(shape)} pool={pool} {dtype} {k}: hip {hip:.3e} cpu-fp32 {cpu:.3e} emulation {em:.3e} fused-vs-unfused {chain:.3e}")
    for k, (hip, cpu, em, chain) in figures.items():
        assert hip <= bound(k, dtype, cpu, em), (k, hip, cpu, em)
        if k != "feat" or dtype == "fp32":   # the un-fused chain rounds its stored activation to bf16 before the mean; the fused one does not
            assert chain <= bound(k, dtype, cpu, em), (k, "fused vs un-fused", chain, cpu, em)
    # decisions, through dy (the gradient at the activation is g = O(1)): a flipped ReLU bit or a gradient routed to another tap moves the
    # element by |gamma * g * rstd| = O(1)
    near_zero, near_tie = G.excluded(r64, pool, G.BF16_MARGIN if dtype == "bf16" else 0.0)
    assert float(near_zero.float().mean()) <= G.EXCLUDED_CAP
    moved = (o["dy"].double() - r64["dy"]).abs() > (0.05 if dtype == "bf16" else 1e-3) * (1 + r64["dy"].abs())
    if pool:
        assert float(near_tie.float().mean()) <= G.EXCLUDED_CAP
        N, C, H, W = shape
        tie_in = torch.zeros_like(near_zero)
        tie_in[:, :, :2 * (H // 2), :2 * (W // 2)] = near_tie.repeat_interleave(2, 2).repeat_interleave(2, 3)
        near_zero = near_zero | tie_in
    assert not bool((moved & ~near_zero).any()), "backward ReLU mask / recomputed argmax"
    return o


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("shape", G.SMALL_SHAPES, ids=G.case_id)
def test_gap_tail_against_fp64_and_the_unfused_chain(shape, pool, dtype):
    check(shape, pool, dtype)


@pytest.mark.parametrize("pool", [0, 1])
def test_gap_tail_conditioning_mean_50_std_1(pool):
    check(G.CONDITIONING_SHAPE, pool, "fp32", conditioning=True, names=("feat", "rstd", "dy"))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_launches_are_bitwise_equal(dtype):
    for shape in ((3, 64, 32, 32), (3, 256, 7, 9)):
        for pool in (0, 1):
            y, gamma, beta, _, dfeat = gap_inputs(shape, pool)
            a, b = (run_fused(shape, pool, dtype, y, gamma, beta, dfeat) for _ in range(2))
            for k in a:
                assert torch.equal(a[k], b[k]), (shape, pool, k)


def test_refused_arguments_launch_nothing():
    lib = _lib.load()
    t = torch.zeros(1 << 16, device=DEV)
    out = torch.full((1 << 16,), 5.0, device=DEV)
    big = ws(1 << 22)
    for (N, C, H, W, groups, pool), code in (((1, 96, 4, 4, 8, 0), 3), ((1, 64, 4, 4, 4, 1), 3), ((1, 32, 4, 4, 8, 0), 3), ((1, 64, 1, 4, 8, 1), 1)):
        assert lib.mmskin_groupnorm8_relu_gap_workspace_bytes(N, C, H, W, groups, pool) == -1
        with pytest.raises(_lib.MMSkinError, match=f"error {code}"):
            call("mmskin_groupnorm8_relu_gap_forward", ptr(t), ptr(t), ptr(t), ptr(out), ptr(out), ptr(out), N, C, H, W, groups, pool, G.EPS,
                 DT["fp32"], ptr(big), stream())
        with pytest.raises(_lib.MMSkinError, match=f"error {code}"):
            call("mmskin_groupnorm8_relu_gap_backward", ptr(t), ptr(t), ptr(t), ptr(t), ptr(out), ptr(out), ptr(out), N, C, H, W, groups, pool,
                 G.EPS, DT["bf16"], ptr(big), stream())
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()), "a refused call wrote to an output"
