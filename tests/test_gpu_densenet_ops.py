"""-m gpu: DenseNet's plan kernels op by op, through the entry points that run what csrc/densenet.hip runs (mmskin_dense_block_*,
mmskin_dense_transition_*: the plan's own block / transition functions; mmskin_slice_stats: slice_stats + bn_table_finalize), against plain
torch in fp64 on the CPU.  Cases and references: tests/densenet_cases.py (checked on the CPU by tests/test_cpu_densenet_cases.py).

Bounds (the project's existing ones).
  fp32: max |got - want| / rms(want) < 2e-4 for every tensor, < 1e-4 for per-channel sums over pixels (dgamma, dbeta, mean), var and
        running_var < 1e-4.  cat, the table and dx are judged per 32-channel slice, the gradients per layer.
  bf16, single-rounding outputs (the transition's pooled rows given the stored conv output): half a bf16 ulp and relative L2 < 1e-3
        against the bf16-rounded reference (half_ulp_excess / l2_vs_rounded of test_gpu_mbconv_ops.py).
  bf16, chains: relative L2 distance from the fp64 truth at most 1.5 x the distance of the CPU emulation (fp64 arithmetic rounded to bf16
        where the plan stores a T) from the same truth -- the factor of test_gpu_densenet.py -- per tensor, per slice and per layer, no
        median.  Both distances go to the parity report (test_gpu_abn.REPORT)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from densenet_cases import (BLOCK_CASES, GROWTH, SLICE_CASES, TRANS_CASES, block_autograd, block_buffer_slices, block_eval_chain, block_id,
                            block_param_slices, block_reference, eval_buffers, pad64, rb64, slice_id, trans_id, trans_reference)
from gpu_util import DEV, DT, rel_err, ws
from mbconv_cases import rb
from mmskin import _lib
from mmskin._lib import call, ptr, stream
from test_gpu_mbconv_ops import edges, half_ulp_excess, l2_vs_rounded, report

pytestmark = pytest.mark.gpu
FP32, SUMS, FACTOR = 2e-4, 1e-4, 1.5


def l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / (want.norm() + 1e-300))


class Judge:
    """one tensor (or slice) at a time: fp32 -> rel_err under `bound`; bf16 chain -> L2 distance from the truth within FACTOR x the
    emulation's.  Figures are recorded before any assertion; failures are collected so that the report holds every tensor."""

    def __init__(self, dtype, rec):
        self.dtype, self.rec, self.failed = dtype, rec, []

    def fp32(self, what, got, want, bound=FP32):
        self.rec[what] = rel_err(got, want)
        if not self.rec[what] < bound:
            self.failed.append((what, self.rec[what], bound))

    def chain(self, what, got, want, emu, bound=FP32):
        if self.dtype == "fp32":
            return self.fp32(what, got, want, bound)
        d_got, d_emu, fp32_err = l2(got, want), l2(emu, want), rel_err(got, want)
        self.rec[what] = dict(kernel=d_got, emulation=d_emu, ratio=d_got / d_emu if d_emu > 0 else (0.0 if d_got == 0 else float("inf")))
        # a tensor no bf16 store lies behind (statistics of the exact block input, ...) has an emulation distance of zero: it is an fp32
        # result of exact operands and is held to the fp32 bound, which needs no allowance in bf16 either
        if not (d_got <= FACTOR * d_emu or fp32_err < bound):
            self.failed.append((what, d_got, d_emu))

    def finish(self):
        report(**self.rec)
        assert not self.failed, self.failed


def block_run(c, r, dtype, training=True, buffers=None):
    lib = _lib.load()
    ctot = c.C0 + GROWTH * c.L
    nbytes = lib.mmskin_dense_block_workspace_bytes(c.N, c.C0, c.L, c.H, c.W)
    assert nbytes > 0
    wsp = ws(nbytes)
    x, dcat, params = r["x"].to(DEV), r["dcat"].to(DEV), r["params"].to(DEV)
    nbuf = block_buffer_slices(c.C0, c.L)[1]
    if buffers is None:   # fresh BatchNorm2d: running_mean 0, running_var 1
        buffers = torch.zeros(nbuf)
        for d in block_buffer_slices(c.C0, c.L)[0]:
            for k in ("rv1", "rv2"):
                buffers[d[k][0]:d[k][0] + d[k][1][0]] = 1.0
    bufs = buffers.to(DEV)
    cat = torch.full((c.N, ctot, c.H, c.W), float("nan"), device=DEV)
    table = torch.full((2 * ctot,), float("nan"), device=DEV)
    call("mmskin_dense_block_forward", ptr(x), ptr(params), ptr(bufs), ptr(cat), ptr(table), c.N, c.C0, c.L, c.H, c.W, int(training), DT[dtype],
         ptr(wsp), stream())
    if not training:
        torch.cuda.synchronize()
        return cat.cpu()
    dx = torch.full((c.N, c.C0, c.H, c.W), float("nan"), device=DEV)
    grads = torch.full((params.numel(),), float("nan"), device=DEV)
    call("mmskin_dense_block_backward", ptr(dcat), ptr(x), ptr(params), ptr(dx), ptr(grads), c.N, c.C0, c.L, c.H, c.W, DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    return dict(cat=cat.cpu(), table=table.cpu(), buffers=bufs.cpu(), dx=dx.cpu(), grads=grads.cpu())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", BLOCK_CASES, ids=block_id)
def test_dense_block_forward_backward(case, dtype):
    """dense_block_forward / dense_block_backward: slice_stats, bn_table_finalize, bn_coef_from_table, slice_pack, the two convs with their
    statistics epilogues, slice_scatter; slice_pack_deferred, the fused dgrads, bn_bwd_finalize(accumulate_bc), slice_accumulate_scaled and
    slice_affine_inplace -- against autograd through torch.cat in fp64.  Per 32-channel slice and per layer: a wrong slice cannot average out."""
    c = case
    r = block_reference(c)
    ref, emu = r["ref"], r["emu"]
    got = block_run(c, r, dtype)
    ctot = c.C0 + GROWTH * c.L
    j = Judge(dtype, dict(test="dense_block", case=block_id(c), dtype=dtype))
    for c0 in range(0, ctot, GROWTH):
        sl = slice(c0, c0 + GROWTH)
        j.chain(f"cat[{c0}:{c0 + GROWTH}]", got["cat"][:, sl], ref["cat"][:, sl], emu["cat"][:, sl])
        j.chain(f"mean[{c0}:{c0 + GROWTH}]", got["table"][:ctot][sl], ref["table"][:ctot][sl], emu["table"][:ctot][sl], SUMS)
        j.chain(f"var[{c0}:{c0 + GROWTH}]", got["table"][ctot:][sl], ref["table"][ctot:][sl], emu["table"][ctot:][sl], SUMS)
    for c0 in range(0, c.C0, GROWTH):
        sl = slice(c0, c0 + GROWTH)
        j.chain(f"dx[{c0}:{c0 + GROWTH}]", got["dx"][:, sl], ref["dx"][:, sl], emu["dx"][:, sl])
    for i, d in enumerate(block_param_slices(c.C0, c.L)[0]):
        cin = c.C0 + GROWTH * i
        tag = f"layer{i}" + (" (padded)" if pad64(cin) != cin else "")
        for k, (o, s) in d.items():
            n = int(torch.tensor(s).prod())
            j.chain(f"{tag} d{k}", got["grads"][o:o + n], ref["grads"][o:o + n], emu["grads"][o:o + n], SUMS if k[0] in "gb" else FP32)
    # Running statistics.  bn_coef_from_table_kernel and bn_finalize's update read fp32 statistics and do not depend on the element type,
    # so the fp32 run holds every layer's momentum update and count / (count - 1) factor at the fp32 bound.  In bf16 the statistics
    # behind them carry the chain's rounding and are judged above through the table; layer 0's norm1 reads the exact block input, so its
    # running_mean AND running_var (the unbias factor included) are held to the fp32 bound in bf16 as well.
    for i, d in enumerate(block_buffer_slices(c.C0, c.L)[0]):
        for k, (o, s) in d.items():
            if dtype == "fp32" or (i == 0 and k in ("rm1", "rv1")):
                j.fp32(f"layer{i} {k}", got["buffers"][o:o + s[0]], ref["buffers"][o:o + s[0]], SUMS)
    j.finish()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dense_block_eval_forward(dtype):
    """eval mode: running statistics, norm2 folded into conv1's staged weights and epilogue (bn_eval_table, stage_weights' fold)"""
    c = BLOCK_CASES[0]
    r = block_reference(c)
    bufs = eval_buffers(c)
    want = block_autograd(c, r["x"], r["dcat"], r["params"], training=False, buffers=bufs)
    got = block_run(c, r, dtype, training=False, buffers=bufs)
    emu = block_eval_chain(c, r["x"], r["params"], bufs, rb64)
    assert torch.equal(got[:, :c.C0], r["x"]), "the block input is copied through"
    j = Judge(dtype, dict(test="dense_block_eval", case=block_id(c), dtype=dtype))
    for c0 in range(c.C0, c.C0 + GROWTH * c.L, GROWTH):   # per layer: fp32 at the fp32 bound, bf16 within 1.5 x the emulation of the folded chain
        sl = slice(c0, c0 + GROWTH)
        j.chain(f"cat[{c0}:{c0 + GROWTH}]", got[:, sl], want[:, sl], emu[:, sl])
    j.finish()


def trans_run(c, r, dtype):
    lib = _lib.load()
    h, PH, PW = c.C // 2, c.H // 2, c.W // 2
    wsp = ws(lib.mmskin_dense_transition_workspace_bytes(c.N, c.C, c.H, c.W, c.pitch))
    x, dnext, params, table = (r[k].to(DEV) for k in ("x", "dnext", "params", "table"))
    bufs = torch.cat([torch.zeros(c.C), torch.ones(c.C)]).to(DEV)
    dst = torch.full((c.N, c.pitch, PH, PW), -3.0, device=DEV)   # sentinel, bf16-representable
    conv = torch.full((c.N, h, c.H, c.W), float("nan"), device=DEV)
    call("mmskin_dense_transition_forward", ptr(x), ptr(table), ptr(params), ptr(bufs), ptr(dst), ptr(conv), c.N, c.C, c.H, c.W, c.pitch, 1,
         DT[dtype], ptr(wsp), stream())
    dx = torch.full((c.N, c.C, c.H, c.W), float("nan"), device=DEV)
    grads = torch.full((params.numel(),), float("nan"), device=DEV)
    dconv = torch.full((c.N, h, c.H, c.W), float("nan"), device=DEV)
    call("mmskin_dense_transition_backward", ptr(dnext), ptr(x), ptr(table), ptr(params), ptr(dx), ptr(grads), ptr(dconv), c.N, c.C, c.H, c.W,
         c.pitch, DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    return dict(dst=dst.cpu(), conv=conv.cpu(), buffers=bufs.cpu(), dx=dx.cpu(), grads=grads.cpu(), dconv=dconv.cpu())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", TRANS_CASES, ids=trans_id)
def test_dense_transition_forward_backward(case, dtype):
    """dense_transition_forward / _backward: bn_coef_from_table, bn_apply, the 1x1 conv, avgpool2_fwd into a pitched destination;
    avgpool2_bwd (odd maps: the rows / columns outside every window), the fused dgrad and bn_backward_from_sums"""
    c = case
    r = trans_reference(c)
    ref, emu = r["ref"], r["emu"]
    got = trans_run(c, r, dtype)
    h = c.C // 2
    j = Judge(dtype, dict(test="dense_transition", case=trans_id(c), dtype=dtype))
    assert torch.equal(got["dst"][:, h:], torch.full_like(got["dst"][:, h:], -3.0)), "channels >= C/2 of the destination rows were touched"
    pooled = got["dst"][:, :h]
    j.chain("conv", got["conv"], ref["conv"], emu["conv"])
    j.chain("pooled", pooled, ref["pooled"], emu["pooled"])
    # the pool alone, given the conv output the kernel stored: a single rounding
    want = F.avg_pool2d(got["conv"].double(), 2)
    if dtype == "fp32":
        j.fp32("pooled given conv", pooled, want)
    else:
        j.rec["pooled_half_ulp_excess"], j.rec["pooled_l2r"] = half_ulp_excess(pooled, want), l2_vs_rounded(pooled, want)
        if not (j.rec["pooled_half_ulp_excess"] <= 0 and j.rec["pooled_l2r"] < 1e-3):
            j.failed.append(("pooled given conv", j.rec["pooled_half_ulp_excess"], j.rec["pooled_l2r"]))
    # avgpool2_bwd alone: a quarter of the pooled gradient (exact in both element types) at every pixel of a window, and EXACTLY zero
    # on the last row / column of an odd map, which lies outside every window.  (dx itself is not zero there: the BatchNorm backward
    # adds cB * x + cC to every pixel; its borders are judged on their own below.)
    PH, PW = c.H // 2, c.W // 2
    routed = torch.zeros(c.N, h, c.H, c.W, dtype=torch.float64)
    routed[:, :, :2 * PH, :2 * PW] = (0.25 * r["dnext"].double()[:, :h]).repeat_interleave(2, 2).repeat_interleave(2, 3)
    assert torch.equal(got["dconv"].double(), routed), "avgpool2_bwd: a quarter of the pooled gradient per window pixel"
    if c.H % 2:
        assert float(got["dconv"][:, :, -1].abs().max()) == 0.0 and float(got["dconv"][:, :, :-1].abs().max()) > 0
    if c.W % 2:
        assert float(got["dconv"][:, :, :, -1].abs().max()) == 0.0
    j.chain("dx", got["dx"], ref["dx"], emu["dx"])
    for name, sl in edges(c.H, c.W):   # odd maps: the bottom row / right column receive no pooled gradient, only cB * x + cC
        j.chain(f"dx {name}", got["dx"][sl], ref["dx"][sl], emu["dx"][sl])
    C = c.C
    j.chain("dgamma", got["grads"][:C], ref["grads"][:C], emu["grads"][:C], SUMS)
    j.chain("dbeta", got["grads"][C:2 * C], ref["grads"][C:2 * C], emu["grads"][C:2 * C], SUMS)
    j.chain("dw", got["grads"][2 * C:], ref["grads"][2 * C:], emu["grads"][2 * C:])
    j.fp32("running_mean", got["buffers"][:C], ref["buffers"][:C], SUMS)
    j.fp32("running_var", got["buffers"][C:], ref["buffers"][C:], SUMS)
    j.finish()


@pytest.mark.parametrize("case", SLICE_CASES, ids=slice_id)
def test_slice_stats_and_table_finalize(case):
    """slice_stats + bn_table_finalize on a channel slice of a wider matrix; the rows above 65 536 (fp32) / 131 072 (bf16) leave more
    than 512 partial rows, so the interleaved slab goes through partial_reduce first (the two-stage branch)."""
    c = case
    g = torch.Generator().manual_seed(c.rows % 1000 + c.C)
    x = rb(torch.randn(c.rows, c.pitch, generator=g) * 2 + torch.randn(1, c.pitch, generator=g))
    sl = x[:, c.c0:c.c0 + c.C].double()
    mean_ref, var_ref = sl.mean(0), sl.var(0, unbiased=False)
    lib = _lib.load()
    wsp = ws(lib.mmskin_slice_stats_workspace_bytes(c.rows, c.pitch, c.c0, c.C))
    xd = x.to(DEV)
    mean, var = torch.full((c.C,), float("nan"), device=DEV), torch.full((c.C,), float("nan"), device=DEV)
    call("mmskin_slice_stats", ptr(xd), c.rows, c.pitch, c.c0, c.C, ptr(mean), ptr(var), DT[c.dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    rec = dict(test="slice_stats", case=slice_id(c), mean=rel_err(mean, mean_ref), var=rel_err(var, var_ref))
    report(**rec)
    assert rec["mean"] < SUMS and rec["var"] < SUMS, rec   # inputs are exact in both element types: one bound


def test_slice_stats_cases_on_the_two_stage_reduction():
    """MMSKIN_BN_SINGLE_ROWS=1 (read once per process -> fresh interpreter) sends every row of SLICE_CASES that leaves more than one partial
    row through partial_reduce + the table epilogue on the interleaved slab: G = 1 for the 70-row fp32 case (2 partial rows), G = 4 for the
    12 805-row case (101), G = 64 for the two long ones as before."""
    env = dict(os.environ, MMSKIN_BN_SINGLE_ROWS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", "test_slice_stats_and_table_finalize"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_unsupported_arguments_are_refused_before_any_launch():
    lib = _lib.load()
    big = ws(1 << 20)
    t = torch.zeros(1 << 16, device=DEV)
    out = torch.full((1 << 16,), 5.0, device=DEV)
    bad = [
        ("mmskin_slice_stats", (ptr(t), 70, 160, 32, 60, ptr(out), ptr(out), DT["fp32"], ptr(big), stream())),        # C not a multiple of the chunk
        ("mmskin_slice_stats", (ptr(t), 70, 32, 0, 64, ptr(out), ptr(out), DT["fp32"], ptr(big), stream())),          # pitch < C
        ("mmskin_dense_block_forward", (ptr(t), ptr(t), ptr(out), ptr(out), ptr(out), 1, 48, 1, 2, 2, 1, DT["fp32"], ptr(big), stream())),
        ("mmskin_dense_transition_forward", (ptr(t), ptr(t), ptr(t), ptr(out), ptr(out), None, 1, 128, 4, 4, 32, 1, DT["fp32"], ptr(big), stream())),   # pitch < C/2
        ("mmskin_dense_transition_forward", (ptr(t), ptr(t), ptr(t), ptr(out), ptr(out), None, 1, 128, 1, 4, 64, 1, DT["fp32"], ptr(big), stream())),   # H < 2
        ("mmskin_dense_transition_forward", (ptr(t), ptr(t), ptr(t), ptr(out), ptr(out), None, 1, 96, 4, 4, 64, 1, DT["fp32"], ptr(big), stream())),    # C
    ]
    for name, args in bad:
        with pytest.raises(_lib.MMSkinError):
            call(name, *args)
        assert lib.mmskin_last_error()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()), "a refused call wrote to an output"
    assert lib.mmskin_slice_stats_workspace_bytes(70, 32, 0, 64) == -1 and lib.mmskin_dense_transition_workspace_bytes(1, 128, 1, 4, 64) == -1
    assert lib.mmskin_dense_block_workspace_bytes(1, 48, 1, 2, 2) == -1
