"""-m gpu: the MBConv kernels of csrc/ops.hip op by op, through the entry points that launch what csrc/mbconv.hip launches
(mmskin_dwconv2d_*, mmskin_batchnorm_act_*, mmskin_se_*, mmskin_sd_*), against plain torch in fp64 on the CPU.

Until these tests the family was reached only through whole-network runs at 64x64 / 96x96 (every map even-sized) judged by a median over
parameters.  Cases: tests/mbconv_cases.py (checked on the CPU by tests/test_cpu_mbconv_cases.py).

Bounds.  Inputs, weights and upstream gradients are bf16-REPRESENTABLE, so operands are exact in both element types and a depthwise
output sums at most 25 exact products.
  fp32: max |got - want| / rms(want) < 2e-4 (TOL["fp32"] of test_gpu_kernels.py); fp32 sums over many pixels (dw, dgamma, ...) < 1e-4 / 2e-4.
  bf16: every stored element within half a bf16 ulp of the exact value, |got - want| <= |want| * 2^-8 + 1e-5 * rms(want), and relative
        L2 < 1e-3 against the reference rounded to bf16 (the criteria of test_gpu_conv_pipe.py); fp32 outputs as in fp32.
Measured errors are appended to the parity report that the conv tests write (test_gpu_abn.REPORT)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from gpu_util import DEV, DT, rel_err, ws
from mbconv_cases import BN_ACTS, BN_SHAPES, DW_CASES, SE_SHAPES, dw_id, dw_reference, out_hw, pad64, rb, se_reference
from mmskin import _lib
from mmskin._lib import call, ptr, stream
from test_gpu_abn import REPORT   # one report file for all parity tests

pytestmark = pytest.mark.gpu
TOL = {"fp32": 2e-4, "bf16": 5e-2}     # test_gpu_kernels.py


def report(**rec):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(json.dumps(rec) + "\n")


def half_ulp_excess(got, want):
    """max of |got - want| - (|want| * 2^-8 + 1e-5 * rms(want)): <= 0 when every element is within half a bf16 ulp"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float(((got - want).abs() - (want.abs() * 2.0 ** -8 + 1e-5 * float(want.pow(2).mean().sqrt()))).max())


def l2_vs_rounded(got, want):
    got, want = got.detach().double().cpu(), rb(want.detach().float().cpu()).double()
    return float((got - want).norm() / (want.norm() + 1e-30))


def check_tensor(what, got, want, dtype, rec):
    """the fp32 or the bf16 criterion of the module docstring on one tensor (or one slice of it); records the figures first"""
    if dtype == "fp32":
        rec[what] = rel_err(got, want)
        assert rec[what] < TOL["fp32"], (what, rec)
    else:
        rec[what + "_half_ulp_excess"] = half_ulp_excess(got, want)
        rec[what + "_l2r"] = l2_vs_rounded(got, want)
        assert rec[what + "_half_ulp_excess"] <= 0 and rec[what + "_l2r"] < 1e-3, (what, rec)


def edges(H, W):
    """border rows / columns and the interior of an [N][C][H][W] tensor, by name"""
    s = slice(None)
    out = [("top row", (s, s, 0)), ("bottom row", (s, s, H - 1)), ("left column", (s, s, s, 0)), ("right column", (s, s, s, W - 1))]
    if H > 2 and W > 2:
        out.append(("interior", (s, s, slice(1, H - 1), slice(1, W - 1))))
    return out


# ------------------------------------------------------------------ depthwise convolution
def dw_run(c, dtype, r):
    lib = _lib.load()
    OH, OW = out_hw(c.H, c.W, c.ksize, c.stride)
    nbytes = lib.mmskin_dwconv2d_workspace_bytes(c.N, c.C, c.H, c.W, c.ksize, c.stride)
    assert nbytes > 0
    wsp = ws(nbytes)
    x, w, dy = r["x"].to(DEV), r["w"].to(DEV), r["dy"].to(DEV)
    y = torch.full((c.N, c.C, OH, OW), float("nan"), device=DEV)
    dx = torch.full((c.N, c.C, c.H, c.W), float("nan"), device=DEV)
    dw = torch.full((c.c_valid, 1, c.ksize, c.ksize), float("nan"), device=DEV)
    call("mmskin_dwconv2d_forward", ptr(x), ptr(w), ptr(y), c.N, c.C, c.H, c.W, c.ksize, c.stride, c.c_valid, DT[dtype], ptr(wsp), stream())
    call("mmskin_dwconv2d_backward", ptr(dy), ptr(x), ptr(w), ptr(dx), ptr(dw), c.N, c.C, c.H, c.W, c.ksize, c.stride, c.c_valid,
         DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    return y.cpu(), dx.cpu(), dw.cpu()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", DW_CASES, ids=dw_id)
def test_depthwise_forward_dgrad_wgrad(case, dtype):
    """dwconv3_fwd / dwconv3_dgrad / dwconv3_wgrad (row-walking kernel for 3x3 stride 1, tapped kernel otherwise; MMSKIN_DWW_ROWS=0: tapped
    for all) with dw_stage_weights' zero fill, against F.conv2d(groups = C) in fp64.  Borders separately from the interior."""
    c = case
    r = dw_reference(c)
    y, dx, dw = dw_run(c, dtype, r)
    OH, OW = out_hw(c.H, c.W, c.ksize, c.stride)
    rec = dict(test="mbconv_depthwise", case=dw_id(c), dtype=dtype, dww_rows=os.environ.get("MMSKIN_DWW_ROWS", "1"))
    rec["dw"] = rel_err(dw, r["dw"])
    try:
        check_tensor("y", y, r["y"], dtype, rec)
        check_tensor("dx", dx, r["dx"], dtype, rec)
        for name, got, want, (h, w_) in (("y", y, r["y"], (OH, OW)), ("dx", dx, r["dx"], (c.H, c.W))):
            for ename, sl in edges(h, w_):
                if float(want[sl].abs().max()) > 0:
                    check_tensor(f"{name} {ename}", got[sl], want[sl], dtype, rec)
        assert rec["dw"] < 1e-4, ("dw", rec)
        if c.c_valid < c.C:   # zero-staged weights: nothing of the padding channels' x / dy comes out
            assert torch.equal(y[:, c.c_valid:], torch.zeros_like(y[:, c.c_valid:])), "y in the padding channels"
            assert torch.equal(dx[:, c.c_valid:], torch.zeros_like(dx[:, c.c_valid:])), "dx in the padding channels"
            assert tuple(dw.shape) == (c.c_valid, 1, c.ksize, c.ksize)
    finally:
        report(**rec)


def test_depthwise_3x3_stride1_cases_on_the_tapped_weight_gradient_kernel():
    """MMSKIN_DWW_ROWS=0 (read once per process -> fresh interpreter) sends the 3x3 / stride-1 rows of the table to the tapped kernel, so
    both weight-gradient kernels meet them -- the rpl rows become four- and six-strip launches there."""
    env = dict(os.environ, MMSKIN_DWW_ROWS="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", "test_depthwise_forward_dgrad_wgrad and k3s1"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ------------------------------------------------------------------ BatchNorm + ReLU6 / SiLU
def _bn_inputs(shape, dtype, with_res, seed):
    g = torch.Generator().manual_seed(seed)
    x = rb(torch.randn(shape, generator=g))
    res = rb(torch.randn(shape, generator=g) * 0.5) if with_res else None
    dy = rb(torch.randn(shape, generator=g))
    C = shape[1]
    return x, res, dy, torch.full((C,), 3.0), torch.full((C,), 3.0)


def _bn_stats64(x, eps):
    x = x.double()
    mean = x.mean((0, 2, 3), keepdim=True)
    var = x.var((0, 2, 3), unbiased=False, keepdim=True)
    invstd = 1.0 / torch.sqrt(var + eps)
    return mean, var, invstd, (x - mean) * invstd


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("act", ["relu6", "silu"])
@pytest.mark.parametrize("shape", BN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batchnorm_with_the_plans_activations(shape, act, with_res, dtype):
    """bn_apply's clamp (relu_cap = 6) and SiLU instantiations, and bn_bwd_reduce / bn_bwd_apply with MASK_FROM_Y6 / MASK_SILU_X, against
    BatchNorm2d(train) + ReLU6 / SiLU in fp64.  gamma = beta = 3 puts >= 10 % of the elements on each side of both clamp edges (asserted).
    The backward reference masks from the y the kernel STORED (ReLU6: 0 < y < 6 on the stored value, so a bf16 value that rounds to exactly
    6.0 is masked there too); dgamma / dbeta are compared with fp64 sums over the same masked values.
    SiLU behind a residual has no backward kernel (the plans' residual units carry no activation): the entry must say so."""
    N, C, H, W = shape
    eps, mom = 1e-3, 0.01
    x, res, dy, gamma, beta = _bn_inputs(shape, dtype, with_res, C + 10 * BN_ACTS[act] + with_res)
    mean, var, invstd, xhat = _bn_stats64(x, eps)
    t = 3.0 * xhat + 3.0 + (res.double() if with_res else 0.0)
    for region in (t <= 0, (t > 0) & (t < 6), t >= 6):   # a condition on the inputs: all three regions of the clamp are populated
        assert float(region.double().mean()) >= 0.10
    y_ref = t.clamp(0, 6) if act == "relu6" else t * torch.sigmoid(t)

    lib = _lib.load()
    wsp = ws(lib.mmskin_batchnorm_act_workspace_bytes(N, C, H, W))
    xd, gd, bd, dyd = x.to(DEV), gamma.to(DEV), beta.to(DEV), dy.to(DEV)
    resd = res.to(DEV) if with_res else None
    rmd, rvd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y = torch.full(shape, float("nan"), device=DEV)
    sm, si = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    call("mmskin_batchnorm_act_forward", ptr(xd), ptr(resd), ptr(gd), ptr(bd), ptr(rmd), ptr(rvd), ptr(y), ptr(sm), ptr(si), N, C, H, W,
         eps, mom, BN_ACTS[act], DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    rec = dict(test="mbconv_batchnorm_act", shape=list(shape), act=act, residual=with_res, dtype=dtype)
    try:
        check_tensor("y", y, y_ref, dtype, rec)
        n = N * H * W
        rec["stats"] = max(rel_err(sm, mean.flatten()), rel_err(si, invstd.flatten()), rel_err(rmd, mom * mean.flatten()),
                           rel_err(rvd, (1 - mom) + mom * var.flatten() * n / (n - 1)))
        assert rec["stats"] < TOL["fp32"], rec

        dx = torch.full(shape, float("nan"), device=DEV)
        dres = torch.full(shape, float("nan"), device=DEV) if with_res else None
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        bwd = lambda: call("mmskin_batchnorm_act_backward", ptr(dyd), ptr(xd), ptr(y), ptr(gd), ptr(bd), ptr(sm), ptr(si), ptr(dx), ptr(dres),
                           ptr(dg), ptr(db), N, C, H, W, BN_ACTS[act], int(with_res), DT[dtype], ptr(wsp), stream())
        if act == "silu" and with_res:
            with pytest.raises(_lib.MMSkinError):
                bwd()
            return
        bwd()
        torch.cuda.synchronize()
        ys = y.double().cpu()
        if act == "relu6":
            dz = dy.double() * ((ys > 0) & (ys < 6))
            rec["masked_share"] = float(((ys > 0) & (ys < 6)).double().mean())
            rec["stored_exactly_6"] = int((ys == 6).sum())
        else:
            sg = torch.sigmoid(t)
            dz = dy.double() * (sg * (1 + t * (1 - sg)))
        dbeta_ref, dgamma_ref = dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3))
        dx_ref = 3.0 * invstd * (dz - dz.mean((0, 2, 3), keepdim=True) - xhat * (dz * xhat).mean((0, 2, 3), keepdim=True))
        rec["dx"], rec["dgamma"], rec["dbeta"] = rel_err(dx, dx_ref), rel_err(dg, dgamma_ref), rel_err(db, dbeta_ref)
        assert rec["dx"] < TOL[dtype], rec
        assert rec["dgamma"] < 2e-4 and rec["dbeta"] < 2e-4, rec
        if with_res:   # the residual's gradient is the masked dy, stored in the element type: exact for bf16-representable dy
            assert torch.equal(dres.double().cpu(), dz), "dres"
    finally:
        report(**rec)


def test_batchnorm_act_on_the_two_stage_reduction():
    """MMSKIN_BN_SINGLE_ROWS=1 (read once per process -> fresh interpreter) sends the (4, 64, 9, 7) ReLU6 case -- 4 partial rows in fp32, 2 in
    bf16 -- through partial_reduce + the table epilogue on the two split slabs of column_stats, and its backward through the two-stage
    bn_bwd_finalize."""
    env = dict(os.environ, MMSKIN_BN_SINGLE_ROWS="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                        "test_batchnorm_with_the_plans_activations and 4x64x9x7 and relu6 and plain"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ------------------------------------------------------------------ squeeze-excitation
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", SE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_squeeze_excitation_chain(shape, dtype):
    """se_forward / se_backward of csrc/mbconv.hip (gap_reduce in both forms, pad_matrix, the two small Linear layers, ew_act_fwd / bwd,
    se_scale_fwd, se_dx and the un-padding copies) against torchvision's SqueezeExcitation math in fp64, at the unpadded shapes.  The
    padding channels of y are zero, as the plan keeps them; those of dy are not, and nothing of them may reach a parameter gradient."""
    N, C, Csq, HW = shape
    Cp = pad64(C)
    g = torch.Generator().manual_seed(C + HW)
    y = torch.zeros(N, Cp, HW)
    y[:, :C] = rb(torch.randn(N, C, HW, generator=g) + 0.3)
    dyse = rb(torch.randn(N, Cp, HW, generator=g))
    w1, b1 = torch.randn(Csq, C, generator=g) / C ** 0.5, torch.randn(Csq, generator=g) * 0.3
    w2, b2 = torch.randn(C, Csq, generator=g) / Csq ** 0.5, torch.randn(C, generator=g) * 0.3
    yse_ref, dy_ref, dw1_ref, db1_ref, dw2_ref, db2_ref = se_reference(y[:, :C], w1, b1, w2, b2, dyse[:, :C])

    lib = _lib.load()
    wsp = ws(lib.mmskin_se_workspace_bytes(N, Cp, Csq, HW))
    dev = [t.to(DEV) for t in (y, w1, b1, w2, b2)]
    dysed = dyse.to(DEV)
    yse = torch.full((N, Cp, HW), float("nan"), device=DEV)
    dyo = torch.full((N, Cp, HW), float("nan"), device=DEV)
    dw1, db1, dw2, db2 = (torch.full(s, float("nan"), device=DEV) for s in ((Csq, C), (Csq,), (C, Csq), (C,)))
    call("mmskin_se_forward", *[ptr(t) for t in dev], ptr(yse), N, C, Cp, Csq, HW, DT[dtype], ptr(wsp), stream())
    call("mmskin_se_backward", ptr(dysed), *[ptr(t) for t in dev], ptr(dyo), ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), N, C, Cp, Csq,
         HW, DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    rec = dict(test="mbconv_squeeze_excitation", shape=list(shape), dtype=dtype)
    try:
        check_tensor("y_se", yse[:, :C], yse_ref, dtype, rec)
        check_tensor("dx", dyo[:, :C], dy_ref, dtype, rec)
        for name, got, want in (("dW1", dw1, dw1_ref), ("db1", db1, db1_ref), ("dW2", dw2, dw2_ref), ("db2", db2, db2_ref)):
            rec[name] = rel_err(got, want)
            assert rec[name] < 2e-4, (name, rec)
        assert torch.equal(yse[:, C:].cpu(), torch.zeros(N, Cp - C, HW)), "y_se in the padding channels"
    finally:
        report(**rec)


# ------------------------------------------------------------------ stochastic depth
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stochastic_depth_values(dtype):
    """sd_residual_add / sd_row_scale: y = branch * mask[n] + res and out = dy * mask[n] with mask in {0, 1 / (1 - p)}.  branch and dy are
    bf16-representable, so branch * 1.25 is exact in fp32 and the fp32 result has one rounding, fused or not: equal to the fp64 result
    rounded once.  Dropped rows: exactly the residual forward, exactly zero backward."""
    N, per = 5, 7 * 7 * 64
    g = torch.Generator().manual_seed(3)
    mask = torch.tensor([1.25, 0.0, 1.25, 1.25, 0.0])   # p = 0.2
    assert set(mask.tolist()) == {0.0, 1.25}
    branch, dy = rb(torch.randn(N, per, generator=g)), rb(torch.randn(N, per, generator=g))
    res = torch.randn(N, per, generator=g)
    if dtype == "bf16":
        res = rb(res)
    y_ref = branch.double() * mask.double()[:, None] + res.double()
    out_ref = dy.double() * mask.double()[:, None]
    lib = _lib.load()
    wsp = ws(lib.mmskin_sd_workspace_bytes(N, per))
    y, out = torch.full((N, per), float("nan"), device=DEV), torch.full((N, per), float("nan"), device=DEV)
    bd, rd, md, dyd = (t.to(DEV) for t in (branch, res, mask, dy))   # named: a temporary's memory is reused by the next .to()
    call("mmskin_sd_forward", ptr(bd), ptr(rd), ptr(md), ptr(y), N, per, DT[dtype], ptr(wsp), stream())
    call("mmskin_sd_backward", ptr(dyd), ptr(md), ptr(out), N, per, DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    y, out = y.cpu(), out.cpu()
    rec = dict(test="mbconv_stochastic_depth", dtype=dtype, fwd=rel_err(y, y_ref), bwd=rel_err(out, out_ref))
    try:
        if dtype == "fp32":
            assert torch.equal(y, y_ref.float()) and torch.equal(out, out_ref.float()), rec
        else:
            check_tensor("y", y, y_ref, dtype, rec)
            check_tensor("out", out, out_ref, dtype, rec)
        drop = mask == 0
        assert torch.equal(y[drop], res[drop]) and torch.equal(out[drop], torch.zeros_like(out[drop])), "dropped rows"
    finally:
        report(**rec)
