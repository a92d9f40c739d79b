"""-m gpu: every HIP kernel behind the C ABI vs a plain PyTorch fp32 CPU reference of the same op.

Tolerances (written per test) are on max|got-want| / rms(want): the exact-f32 MFMA path must agree to
2e-4 (fp32 arithmetic, different summation order only); the bf16 path to 5e-2 -- bf16 storage rounds
every element to 2^-9 relative, i.e. up to ~1% of the rms for the largest (4-5 sigma) elements, on top of
the rounded operands.
"""
import os

import pytest
import torch
import torch.nn.functional as F

import conv_route_cases as CR
from gpu_util import DEV, DT, conv_backward, conv_forward, rel_err, ws
from mmskin import _lib, ops
from mmskin._lib import call, ptr, stream

pytestmark = pytest.mark.gpu
TOL = {"fp32": 2e-4, "bf16": 5e-2}

CONV_CASES = [
    # N, Cin, H, W, Cout, k, stride, pad
    (2, 64, 14, 14, 64, 1, 1, 0),      # layer1-style 1x1, BN=64 tile
    (2, 64, 14, 14, 256, 1, 1, 0),     # expand 1x1, single K tile
    (2, 256, 9, 11, 128, 1, 1, 0),     # odd spatial dims, ragged last row block
    (3, 64, 12, 12, 64, 3, 1, 1),      # 3x3 stride 1
    (2, 128, 14, 14, 128, 3, 2, 1),    # 3x3 stride 2 (dgrad parity classes)
    (2, 128, 15, 13, 128, 3, 2, 1),    # 3x3 stride 2, odd sizes
    (2, 256, 14, 14, 512, 1, 2, 0),    # downsample 1x1 stride 2
    (1, 512, 7, 7, 512, 3, 1, 1),      # layer4-style, M < one row block
    (2, 64, 56, 56, 64, 3, 1, 1),      # all-taps 3x3 wgrad: one image row per stage
    (3, 128, 28, 28, 64, 3, 1, 1),     # ... two rows per stage, two cin tiles
    (5, 64, 14, 14, 128, 3, 1, 1),     # ... four rows per stage, ragged last stage of every image (14 = 4+4+4+2)
    (2, 64, 9, 13, 64, 3, 1, 1),       # ... odd sizes (4 rows of 13 per stage)
]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_forward_backward(case, dtype):
    N, Cin, H, W, Cout, k, stride, pad = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, stride=stride, padding=pad)
    dy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(dy)
    # what these cases cover: the two-stage 128-row tile with the plain epilogue, 128 | 64 columns wide (tests/conv_route_cases.py has the rest)
    eb = CR.BF16 if dtype == "bf16" else CR.F32
    assert CR.route(_lib.load(), CR.FWD, case, eb)[:6] == (CR.CG_TILE128, 128, 128, 128 if Cout % 128 == 0 else 64, 2, 0)
    assert CR.route(_lib.load(), CR.DGRAD, case, eb)[:6] == (CR.CG_TILE128, 128, 128, 128 if Cin % 128 == 0 else 64, 2, 0)
    y = conv_forward(x.to(DEV), w.to(DEV), stride, pad, dtype)
    assert rel_err(y, y_ref) < TOL[dtype], ("fwd", rel_err(y, y_ref))
    dx, dw = conv_backward(dy.to(DEV), x.to(DEV), w.to(DEV), stride, pad, dtype)
    assert rel_err(dx, xr.grad) < TOL[dtype], ("dgrad", rel_err(dx, xr.grad))
    assert rel_err(dw, wr.grad) < TOL[dtype], ("wgrad", rel_err(dw, wr.grad))


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_bf16_tight_on_representable_inputs(case):
    """The bf16 kernels on bf16-REPRESENTABLE inputs against an fp64 reference: the operands are exact, so what is
    left is the rounding of the stored result (forward / dgrad: EVERY element within half a bf16 ulp of the exact value, relative L2 against the reference
    rounded to bf16 < 1e-3) and the fp32 summation order (wgrad, fp32 output: < 1e-4).  A dropped 8-element fragment fails all three."""
    import json
    N, Cin, H, W, Cout, k, stride, pad = case
    g = torch.Generator().manual_seed(sum(case) + 1)
    rb = lambda t: t.bfloat16().float()
    x = rb(torch.randn(N, Cin, H, W, generator=g))
    w = rb(torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, stride=stride, padding=pad)
    dy = rb(torch.randn(y_ref.shape, generator=g))
    y_ref.backward(dy.double())
    y = conv_forward(x.to(DEV), w.to(DEV), stride, pad, "bf16")
    dx, dw = conv_backward(dy.to(DEV), x.to(DEV), w.to(DEV), stride, pad, "bf16")
    def l2r(got, want):
        got, want = got.double().cpu(), rb(want.float()).double()
        return float((got - want).norm() / (want.norm() + 1e-30))
    rec = dict(test="conv_bf16_tight", case=list(case), fwd=rel_err(y, y_ref), fwd_l2r=l2r(y, y_ref.detach()), dgrad=rel_err(dx, xr.grad),
               dgrad_l2r=l2r(dx, xr.grad), wgrad=rel_err(dw, wr.grad))
    rep = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity_report.jsonl")
    os.makedirs(os.path.dirname(rep), exist_ok=True)
    with open(rep, "a") as f:
        f.write(json.dumps(rec) + "\n")
    # every stored element within half a bf16 ulp (2^-8 relative) of the exact value, plus the fp32 summation noise
    for got, want in ((y, y_ref.detach()), (dx, xr.grad)):
        got, want = got.double().cpu(), want.double()
        assert bool(((got - want).abs() <= want.abs() * 2.0 ** -8 + 1e-5 * float(want.pow(2).mean().sqrt())).all()), rec
    assert rec["fwd_l2r"] < 1e-3 and rec["dgrad_l2r"] < 1e-3, rec
    assert rec["wgrad"] < 1e-4, rec


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("hw,nst", [(203, 1), (202, 2)])
def test_conv_single_buffer_and_two_stage_tiles(hw, nst, dtype):
    """The 128-row tile on both sides of its 640-workgroup threshold: a 1x1 convolution 64 -> 128 over 2 x 203 x 203 pixels is 644 row blocks
    (single LDS buffer, NST 1), over 2 x 202 x 202 it is 638 (two stages); the data gradient (64 columns) likewise.  bf16: representable
    inputs against fp64, every element within half a bf16 ulp and relative L2 < 1e-3 against the rounded reference (the bound of
    test_conv_bf16_tight_on_representable_inputs); fp32: this file's fp32 bound."""
    case = (2, 64, hw, hw, 128, 1, 1, 0)
    lib, eb = _lib.load(), CR.BF16 if dtype == "bf16" else CR.F32
    assert CR.route(lib, CR.FWD, case, eb)[:6] == (CR.CG_TILE128, 128, 128, 128, nst, 0)
    assert CR.route(lib, CR.DGRAD, case, eb)[:6] == (CR.CG_TILE128, 128, 128, 64, nst, 0)
    g = torch.Generator().manual_seed(hw)
    rb = (lambda t: t.bfloat16().float()) if dtype == "bf16" else (lambda t: t)
    x, w = rb(torch.randn(2, 64, hw, hw, generator=g)), rb(torch.randn(128, 64, 1, 1, generator=g) / 8)
    dy = rb(torch.randn(2, 128, hw, hw, generator=g))
    y_ref = torch.einsum("nchw,oc->nohw", x.double(), w.double()[:, :, 0, 0])
    dx_ref = torch.einsum("nohw,oc->nchw", dy.double(), w.double()[:, :, 0, 0])
    y = conv_forward(x.to(DEV), w.to(DEV), 1, 0, dtype)
    dx, _ = conv_backward(dy.to(DEV), x.to(DEV), w.to(DEV), 1, 0, dtype)
    for name, got, want in (("fwd", y, y_ref), ("dgrad", dx, dx_ref)):
        got = got.double().cpu()
        if dtype == "fp32":
            assert rel_err(got, want) < TOL["fp32"], (name, rel_err(got, want))
            continue
        wr = want.float().bfloat16().double()
        l2 = float((got - wr).norm() / wr.norm())
        print(name, "max err / rms", rel_err(got, want), "rel l2 vs rounded", l2)
        assert bool(((got - want).abs() <= want.abs() * 2.0 ** -8 + 1e-5 * float(want.pow(2).mean().sqrt())).all()), name
        assert l2 < 1e-3, (name, l2)


def test_batchnorm_two_stage_reduction():
    """Statistics tables above MMSKIN_BN_SINGLE_ROWS rows take two reduction stages (partial_reduce + finalize): MMSKIN_BN_SINGLE_ROWS=4 sends
    every case of test_batchnorm_train_forward_backward with more than four partial rows through them (G = 1 .. 5 groups), and
    test_batchnorm_train_forward_backward_reduction_scratch, selected by the same -k, fails there unless the first stage really ran."""
    import subprocess, sys
    env = dict(os.environ, MMSKIN_BN_SINGLE_ROWS="4")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k", "batchnorm_train_forward_backward"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_conv_rejects_unsupported_shapes():
    x = torch.zeros(1, 3, 8, 8, device=DEV)
    w = torch.zeros(16, 3, 3, 3, device=DEV)
    with pytest.raises(_lib.MMSkinError):
        conv_forward(x, w, 1, 1, "fp32")


def partial_rows(rows, C, epc):
    """col_geom of csrc/ops_internal.h: the partial rows column_stats / bn_bwd_reduce leave (epc = 4 fp32, 8 bf16 elements per 16-byte chunk)"""
    cpr = C // epc
    rl = 256 // min(cpr, 256)
    rb = max((rows + 1023) // 1024, rl * 4)
    rb = (rb + rl - 1) // rl * rl
    return (rows + rb - 1) // rb


# The first three leave 4 / 5 / 37 (fp32) and 2 / 5 / 19 (bf16) partial rows: the <= 64-row forms of the finalize kernels.  The last two have
# 5 * 32 * 52 = 8320 rows.  C = 64: 130 partial rows in fp32 (16 row lanes x 4 rows per lane = 64 rows per block) and 65 in bf16 (32 lanes:
# 128 per block) -- the smallest counts that put both element types on the 65 .. 512-row forms (64 x 16 forward, 16 x 16 backward).  C = 72:
# 149 in fp32 (18 chunks per row: 14 lanes, 56 rows per block) and 75 in bf16 (9 chunks: 28 lanes, 112 per block); 72 is a multiple of
# neither 64 nor 16, so the c < C guard of the last column block is live in the 64-wide and in the 16-wide form.
BN_TRAIN_SHAPES = [(4, 64, 9, 7), (2, 2048, 3, 3), (3, 256, 14, 14), (5, 64, 32, 52), (5, 72, 32, 52)]
assert [partial_rows(8320, C, epc) for C in (64, 72) for epc in (4, 8)] == [130, 65, 149, 75]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", BN_TRAIN_SHAPES)
def test_batchnorm_train_forward_backward(shape, relu, dtype):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(C + relu)
    x = torch.randn(shape, generator=g) * 2 + 0.5
    if dtype == "bf16":
        x = x.bfloat16().float()     # bf16-representable input: the reference sees what the kernel stores
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    rm, rv = torch.zeros(C), torch.ones(C)
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y_ref = F.batch_norm(xr, rm, rv, gr, br, training=True, momentum=0.1, eps=1e-5)
    if relu:
        y_ref = F.relu(y_ref)
    dy = torch.randn(shape, generator=g)
    if dtype == "bf16":
        dy = dy.bfloat16().float()
    y_ref.backward(dy)
    lib = _lib.load()
    wsp = ws(lib.mmskin_batchnorm_workspace_bytes(N, C, H, W))
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    rmd, rvd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y, sm, si = torch.empty_like(xd), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    call("mmskin_batchnorm_forward", ptr(xd), ptr(gd), ptr(bd), ptr(rmd), ptr(rvd), ptr(y), ptr(sm), ptr(si), N, C, H,
         W, 1e-5, 0.1, relu, DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    tol = TOL[dtype]
    assert rel_err(y, y_ref) < tol
    assert rel_err(rmd, rm) < tol and rel_err(rvd, rv) < tol          # running stats (updated in place by F.batch_norm)
    dx, dg, db = torch.empty_like(xd), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    call("mmskin_batchnorm_backward", ptr(dy.to(DEV)), ptr(xd), ptr(gd), ptr(bd), ptr(sm), ptr(si), ptr(dx), ptr(dg),
         ptr(db), N, C, H, W, relu, DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    assert rel_err(dx, xr.grad) < 3 * tol, rel_err(dx, xr.grad)
    assert rel_err(dg, gr.grad) < 3 * tol and rel_err(db, br.grad) < 3 * tol


def test_batchnorm_train_forward_backward_reduction_scratch():
    """Which reduction the forward's finalize took, read off a workspace poisoned to NaN beforehand.  (5, 72, 32, 52) in fp32 leaves 149 partial
    rows.  Above MMSKIN_BN_SINGLE_ROWS (test_batchnorm_two_stage_reduction's child: 4) the first stage must have left G = ceil(149 / 32) = 5
    fp64 group rows per slab at the head of the scratch carve -- the last 2 * 64 * C doubles of the workspace -- which add up to the column sums
    of x and x^2, with the rest of the carve untouched; at the default (512) the whole carve is untouched.  The statistics are finite and right
    either way.  Bound on the group sums: they add fp32 partials whose longest chain is 4 rows per lane + 14 lanes = 18 < 64 additions, so
    each column's error is below 64 * 2^-24 * sum |x| (resp. x^2); the fp64 stages add nothing at that scale."""
    N, C, H, W = shape = (5, 72, 32, 52)
    nrows, single = partial_rows(N * H * W, C, 4), int(os.environ.get("MMSKIN_BN_SINGLE_ROWS", "512"))
    assert nrows == 149
    x = torch.randn(shape, generator=torch.Generator().manual_seed(7)) * 2 + 0.5
    lib = _lib.load()
    wsp = ws(lib.mmskin_batchnorm_workspace_bytes(N, C, H, W))
    wsp.fill_(0xFF)                                                    # every float and double of the workspace: NaN
    xd, gd, bd = x.to(DEV), torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    rmd, rvd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y, sm, si = torch.empty_like(xd), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    call("mmskin_batchnorm_forward", ptr(xd), ptr(gd), ptr(bd), ptr(rmd), ptr(rvd), ptr(y), ptr(sm), ptr(si), N, C, H, W, 1e-5, 0.1, 0, DT["fp32"],
         ptr(wsp), stream())
    torch.cuda.synchronize()
    x64 = x.double()
    assert bool(torch.isfinite(sm).all()) and bool(torch.isfinite(si).all()) and bool(torch.isfinite(y).all())
    assert rel_err(sm, x64.mean((0, 2, 3))) < TOL["fp32"] and rel_err(si, 1 / torch.sqrt(x64.var((0, 2, 3), unbiased=False) + 1e-5)) < TOL["fp32"]
    scratch = wsp[-2 * 64 * C * 8:].view(torch.float64).cpu()
    if nrows > single:
        G = min(64, (nrows + 31) // 32)
        head, rest = scratch[:2 * G * C].view(2, G, C), scratch[2 * G * C:]
        assert bool(torch.isfinite(head).all()), "the first stage left no group sums"
        for got, v in ((head[0].sum(0), x64), (head[1].sum(0), x64 * x64)):
            assert bool(((got - v.sum((0, 2, 3))).abs() <= 64 * 2.0 ** -24 * v.abs().sum((0, 2, 3))).all())
    else:
        rest = scratch
    assert bool(torch.isnan(rest).all()), "doubles of the scratch carve that no stage of this reduction writes were written"


def test_stem_backward_sums_from_the_pooled_side_and_zero_gamma():
    """BatchNorm-backward sums of the stem from the pooled tensors (x at the argmax reconstructed as (y - shift) / scale; default) against
    the conv-output form (MMSKIN_STEM_SUMS_POOLED=0 is exercised by test_stem_forward_backward's reference either way): fp32 operands, so
    both must match torch to the fp32 tolerance -- including two channels with gamma = 0, whose scale cannot be inverted and which read x at
    the recorded argmax instead."""
    N, H, W = 3, 50, 70
    g = torch.Generator().manual_seed(9)
    x = torch.randn(N, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    gamma[5] = 0.0; gamma[40] = 0.0; beta[5] = 0.3; beta[40] = -0.2
    wr, gr, br = (t.clone().requires_grad_(True) for t in (w, gamma, beta))
    z = F.relu(F.batch_norm(F.conv2d(x, wr, stride=2, padding=3), None, None, gr, br, training=True, eps=1e-5))
    y_ref = F.max_pool2d(z, 3, 2, 1)
    dy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(dy)
    lib = _lib.load()
    wsp = ws(lib.mmskin_stem_workspace_bytes(N, H, W))
    keep = [x.to(DEV), w.to(DEV), gamma.to(DEV), beta.to(DEV)]
    dw, dg, db = torch.empty(64, 3, 7, 7, device=DEV), torch.empty(64, device=DEV), torch.empty(64, device=DEV)
    dyd = dy.to(DEV)
    call("mmskin_stem_backward", ptr(dyd), *[ptr(t) for t in keep], ptr(dw), ptr(dg), ptr(db), N, H, W, 1e-5, DT["fp32"], ptr(wsp), stream())
    torch.cuda.synchronize()
    tol = TOL["fp32"]
    assert rel_err(dg, gr.grad) < 3 * tol and rel_err(db, br.grad) < 3 * tol, (rel_err(dg, gr.grad), rel_err(db, br.grad))
    assert abs(float(dg[5]) - float(gr.grad[5])) <= 3 * tol * float(gr.grad.abs().max())
    assert rel_err(dw, wr.grad) < 3 * tol, rel_err(dw, wr.grad)


def test_stem_direct_7x7_kernel_at_224():
    """224 x 224 images in bf16 take the direct 7x7 convolution (csrc/stem7x7.hip, launch counter asserted).  Inputs and weights are
    bf16-representable, so the fp64 reference multiplies what the kernel multiplies: pooled output within 4e-3 relative L2 (two bf16
    storages: the conv output and the result).  The same call with MMSKIN_STEM7X7=0 (gather-GEMM form, fresh interpreter) must give the
    SAME bits: both accumulate kernel row by kernel row in fp32 on the same MFMA shape, and the statistics only differ in summation order
    (scale / shift equal to ~1e-7, which cannot move a bf16 result except on a rounding tie -- a handful of elements are allowed)."""
    import subprocess, sys, tempfile
    N, H, W = 3, 224, 224
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, 3, H, W, generator=g).bfloat16().float()
    w = (torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5).bfloat16().float()
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    z = F.conv2d(x.double(), w.double(), stride=2, padding=3).float().bfloat16().double()       # stored in bf16
    y_ref = F.max_pool2d(F.relu(F.batch_norm(z, None, None, gamma.double(), beta.double(), training=True, eps=1e-5)), 3, 2, 1)
    lib = _lib.load()
    wsp = ws(lib.mmskin_stem_workspace_bytes(N, H, W))
    y = torch.empty(y_ref.shape, device=DEV)
    keep = [x.to(DEV), w.to(DEV), gamma.to(DEV), beta.to(DEV)]
    n0 = lib.mmskin_stem7x7_launches()
    call("mmskin_stem_forward", *[ptr(t) for t in keep], ptr(y), N, H, W, 1e-5, DT["bf16"], ptr(wsp), stream())
    torch.cuda.synchronize()
    assert lib.mmskin_stem7x7_launches() == n0 + 1
    l2 = float((y.double().cpu() - y_ref).norm() / y_ref.norm())
    assert l2 < 4e-3, l2
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import sys, torch
sys.path[:0] = [%r, %r]
from gpu_util import DEV, DT, ws
from mmskin import _lib
from mmskin._lib import call, ptr, stream
lib = _lib.load()
d = torch.load(sys.argv[1])
keep = [d[k].to(DEV) for k in ("x", "w", "gamma", "beta")]
N, _, H, W = d["x"].shape
wsp = ws(lib.mmskin_stem_workspace_bytes(N, H, W))
y = torch.empty(N, 64, H // 4, W // 4, device=DEV)
call("mmskin_stem_forward", *[ptr(t) for t in keep], ptr(y), N, H, W, 1e-5, DT["bf16"], ptr(wsp), stream())
torch.cuda.synchronize()
assert lib.mmskin_stem7x7_launches() == 0
torch.save(y.cpu(), sys.argv[2])
"""
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.pt"), os.path.join(td, "out.pt")
        torch.save(dict(x=x, w=w, gamma=gamma, beta=beta), fi)
        r = subprocess.run([sys.executable, "-c", code % (os.path.join(root, "tests"), os.path.join(root, "multimodal-model-skin-lesion-classifier_amd")), fi, fo],
                           env=dict(os.environ, MMSKIN_STEM7X7="0"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        y_old = torch.load(fo)
    ndiff = int((y.cpu() != y_old).sum())
    assert ndiff <= 64 and float((y.cpu() - y_old).abs().max()) <= 2.0 ** -6 * float(y_old.abs().max()), ndiff


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("hw", [(64, 64), (48, 80), (50, 70), (37, 45)])   # the last two: odd conv / pool output sizes
def test_stem_forward_backward(hw, dtype):
    """conv7x7/2 + BN(train) + ReLU + maxpool3x3/2, incl. the padded-NHWC4 'virtual conv' trick."""
    H, W = hw
    N = 3
    g = torch.Generator().manual_seed(H)
    x = torch.randn(N, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    wr, gr, br = (t.clone().requires_grad_(True) for t in (w, gamma, beta))
    z = F.conv2d(x, wr, stride=2, padding=3)
    z = F.relu(F.batch_norm(z, None, None, gr, br, training=True, eps=1e-5))
    y_ref = F.max_pool2d(z, 3, 2, 1)
    dy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(dy)
    lib = _lib.load()
    wsp = ws(lib.mmskin_stem_workspace_bytes(N, H, W))
    y = torch.empty(y_ref.shape, device=DEV)
    args = (ptr(x.to(DEV)), ptr(w.to(DEV)), ptr(gamma.to(DEV)), ptr(beta.to(DEV)))
    keep = [x.to(DEV), w.to(DEV), gamma.to(DEV), beta.to(DEV)]
    args = tuple(ptr(t) for t in keep)
    call("mmskin_stem_forward", *args, ptr(y), N, H, W, 1e-5, DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    tol = TOL[dtype]
    assert rel_err(y, y_ref) < tol, rel_err(y, y_ref)
    dw, dg, db = torch.empty(64, 3, 7, 7, device=DEV), torch.empty(64, device=DEV), torch.empty(64, device=DEV)
    dyd = dy.to(DEV)
    call("mmskin_stem_backward", ptr(dyd), *args, ptr(dw), ptr(dg), ptr(db), N, H, W, 1e-5, DT[dtype], ptr(wsp),
         stream())
    torch.cuda.synchronize()
    if dtype == "fp32":
        assert rel_err(dw, wr.grad) < 3 * tol, rel_err(dw, wr.grad)
        assert rel_err(dg, gr.grad) < 3 * tol and rel_err(db, br.grad) < 3 * tol
    else:
        # bf16: the conv output is rounded before BN/ReLU/max-pool, so a few activations land on the other
        # side of 0 or hand the pooling window to a neighbour; each flip moves one gradient entry by O(1).
        # Those are sparse, so the check is in relative L2 rather than max-norm.
        l2 = lambda a, b: float((a.cpu().double() - b.double()).norm() / b.double().norm())
        assert l2(dw, wr.grad) < 0.1, l2(dw, wr.grad)
        assert l2(dg, gr.grad) < 0.1 and l2(db, br.grad) < 0.1


# ------------------------------------------------------------------------------- head operators
def _chk(got, want, tol=2e-5):
    if float((got.detach().cpu().double() - want.detach().double()).abs().max()) < 1e-5:
        return               # mathematically-zero gradients (e.g. softmax over one key): absolute check
    assert rel_err(got, want) < tol, rel_err(got, want)


@pytest.mark.parametrize("M,K,N", [(4, 20, 256), (256, 512, 512), (7, 85, 64), (130, 1024, 6), (33, 2048, 512),
                                   (20992, 32, 96), (5003, 128, 32)])   # batch*tokens rows: split-K dW, two-stage bias sum
@pytest.mark.parametrize("relu", [False, True])
def test_linear(M, K, N, relu):
    g = torch.Generator().manual_seed(M * N)
    x = torch.randn(M, K, generator=g); w = torch.randn(N, K, generator=g) / K ** 0.5; b = torch.randn(N, generator=g)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    y_ref = F.linear(xr, wr, br)
    if relu:
        y_ref = F.relu(y_ref)
    dy = torch.randn(M, N, generator=g)
    y_ref.backward(dy)
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    y = ops.linear(xd, wd, bd, relu)
    y.backward(dy.to(DEV))
    _chk(y, y_ref); _chk(xd.grad, xr.grad); _chk(wd.grad, wr.grad); _chk(bd.grad, br.grad)


@pytest.mark.parametrize("M,N", [(4, 64), (256, 512), (9, 2048), (5, 32), (20992, 32), (4099, 96)])
@pytest.mark.parametrize("relu", [False, True])
def test_layernorm(M, N, relu):
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, N, generator=g) * 3 + 1; w = torch.rand(N, generator=g) + 0.5; b = torch.randn(N, generator=g) * 0.2
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    y_ref = F.layer_norm(xr, (N,), wr, br)
    if relu:
        y_ref = F.relu(y_ref)
    dy = torch.randn(M, N, generator=g)
    y_ref.backward(dy)
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    y = ops.layernorm(xd, wd, bd, 1e-5, relu)
    y.backward(dy.to(DEV))
    _chk(y, y_ref); _chk(xd.grad, xr.grad, 1e-4); _chk(wd.grad, wr.grad, 1e-4); _chk(bd.grad, br.grad, 1e-4)


def test_pointwise_gates():
    g = torch.Generator().manual_seed(3)
    a, b, c = (torch.randn(37, 64, generator=g) for _ in range(3))
    dy = torch.randn(37, 64, generator=g)
    for name, fn_ref, fn in (
        ("sigmoid_gate", lambda z, v: torch.sigmoid(z) * v, ops.sigmoid_gate),
        ("gated_mix", lambda z, p, q: torch.sigmoid(z) * p + (1 - torch.sigmoid(z)) * q, ops.gated_mix),
        ("metablock_gate", lambda V, t1, t2: torch.sigmoid(torch.tanh(V * t1) + t2), ops.metablock_gate),
    ):
        nargs = 2 if name == "sigmoid_gate" else 3
        ref_in = [t.clone().requires_grad_(True) for t in (a, b, c)[:nargs]]
        dev_in = [t.to(DEV).requires_grad_(True) for t in (a, b, c)[:nargs]]
        yr = fn_ref(*ref_in); yr.backward(dy)
        yd = fn(*dev_in); yd.backward(dy.to(DEV))
        _chk(yd, yr)
        for r, d in zip(ref_in, dev_in):
            _chk(d.grad, r.grad)


def test_concat_dropout_embedding():
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(6, 10, generator=g), torch.randn(6, 7, generator=g)
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = ops.concat2(ad, bd)
    assert torch.equal(y.cpu(), torch.cat([a, b], 1))
    dy = torch.randn(6, 17, generator=g)
    y.backward(dy.to(DEV))
    assert torch.equal(ad.grad.cpu(), dy[:, :10]) and torch.equal(bd.grad.cpu(), dy[:, 10:])
    # dropout: inverted scaling, mask reused in backward, keep-rate close to 1-p, eval = identity
    x = torch.ones(400, 500, device=DEV, requires_grad=True)
    y = ops.dropout(x, 0.3, True)
    keep = (y != 0).float().mean().item()
    assert abs(keep - 0.7) < 0.01
    assert torch.allclose(y[y != 0], torch.tensor(1 / 0.7, device=DEV))
    y.sum().backward()
    assert torch.equal((x.grad != 0), (y != 0))
    assert ops.dropout(x, 0.3, False) is x
    # embedding
    table = torch.randn(5, 10, 8, generator=g)
    ids = torch.randint(0, 10, (9, 5), generator=g)
    tr = table.clone().requires_grad_(True)
    ref = torch.stack([tr[c][ids[:, c]] for c in range(5)], dim=1)
    dyo = torch.randn(9, 5, 8, generator=g)
    ref.backward(dyo)
    td = table.to(DEV).requires_grad_(True)
    out = ops.embedding(td, ids.to(DEV))
    out.backward(dyo.to(DEV))
    _chk(out, ref); _chk(td.grad, tr.grad)


@pytest.mark.parametrize("B,H,L,Dh", [(3, 4, 82, 8), (2, 8, 1, 64), (2, 2, 17, 16)])
def test_attention(B, H, L, Dh):
    g = torch.Generator().manual_seed(L)
    q, k, v = (torch.randn(B, H, L, Dh, generator=g) for _ in range(3))
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qr, kr, vr)
    dO = torch.randn(B, H, L, Dh, generator=g)
    ref.backward(dO)
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    out = ops.attention(qd, kd, vd)
    out.backward(dO.to(DEV))
    _chk(out, ref, 1e-4); _chk(qd.grad, qr.grad, 1e-4); _chk(kd.grad, kr.grad, 1e-4); _chk(vd.grad, vr.grad, 1e-4)


def test_attention_probability_dropout():
    """Training-mode dropout on the attention probabilities (nn.MultiheadAttention(dropout=p) inside the
    TabTransformer encoder).  RNG streams cannot match torch's, so the check is structural: with V = identity the
    output IS the dropped probability matrix, which gives the mask; forward and backward must then equal the
    torch formula softmax(qk^T/sqrt(d)) * mask / (1-p) @ v for that mask, and the keep rate must be ~1-p."""
    B, H, L, p = 4, 4, 32, 0.3
    g = torch.Generator().manual_seed(5)
    q, k = (torch.randn(B, H, L, L, generator=g) for _ in range(2))
    eye = torch.eye(L).expand(B, H, L, L).contiguous()
    torch.manual_seed(77)
    cnt0 = ops._dropout_counter[0]
    probe = ops.attention(q.to(DEV), k.to(DEV), eye.to(DEV), p, True).cpu()          # = P * mask / (1-p)
    mask = (probe != 0).float()
    soft = torch.softmax(q @ k.transpose(-1, -2) / L ** 0.5, dim=-1)
    _chk(probe, soft * mask / (1 - p), 1e-4)
    assert abs(float(mask.mean()) - (1 - p)) < 0.02
    # same (seed, offset) -> same mask: rerun with a real V and compare with autograd through the torch formula
    ops._dropout_counter[0] = cnt0
    v = torch.randn(B, H, L, L, generator=g)
    dO = torch.randn(B, H, L, L, generator=g)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = (torch.softmax(qr @ kr.transpose(-1, -2) / L ** 0.5, dim=-1) * mask / (1 - p)) @ vr
    ref.backward(dO)
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    out = ops.attention(qd, kd, vd, p, True)
    out.backward(dO.to(DEV))
    _chk(out, ref, 1e-4); _chk(qd.grad, qr.grad, 1e-4); _chk(kd.grad, kr.grad, 1e-4); _chk(vd.grad, vr.grad, 1e-4)
    # eval mode / p = 0: no dropout
    _chk(ops.attention(qd, kd, vd, p, False), soft @ v, 1e-4)


def test_custom_cnn_pieces():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 3, 32, 32, generator=g)
    w = torch.randn(16, 3, 3, 3, generator=g) * 0.2; b = torch.randn(16, generator=g) * 0.1
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = F.adaptive_avg_pool2d(F.max_pool2d(F.relu(F.conv2d(x, wr, br, stride=2, padding=1)), 2), 1).flatten(1)
    dy = torch.randn(3, 16, generator=g)
    ref.backward(dy)
    wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = ops.pool_gap(ops.direct_conv2d(x.to(DEV), wd, bd, 2, 1, True), 2)
    out.backward(dy.to(DEV))
    _chk(out, ref); _chk(wd.grad, wr.grad, 1e-4); _chk(bd.grad, br.grad, 1e-4)


def test_linear_rows_gives_whole_parameter_gradients():
    """ops.linear_rows (value projection of nn.MultiheadAttention with one key): y and dx as F.linear on the row block, dW / db of the WHOLE
    stacked parameter with exact zeros outside it -- what autograd's slice backward produces with two fills and two copies."""
    g = torch.Generator().manual_seed(21)
    D, B = 96, 37
    x = torch.randn(B, D, generator=g)
    W = torch.randn(3 * D, D, generator=g) / D ** 0.5
    b = torch.randn(3 * D, generator=g)
    dy = torch.randn(B, D, generator=g)
    xr, Wr, br = (t.clone().requires_grad_(True) for t in (x, W, b))
    F.linear(xr, Wr[2 * D:], br[2 * D:]).backward(dy)
    xd, Wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, W, b))
    y = ops.linear_rows(xd, Wd, bd, 2 * D, 3 * D)
    y.backward(dy.to(DEV))
    _chk(y, F.linear(x, W[2 * D:], b[2 * D:])); _chk(xd.grad, xr.grad); _chk(Wd.grad, Wr.grad, 1e-4); _chk(bd.grad, br.grad, 1e-4)
    assert float(Wd.grad[:2 * D].abs().max()) == 0.0 and float(bd.grad[:2 * D].abs().max()) == 0.0


def test_linear_bf16_operand_mode():
    """MMSKIN_LINEAR_DTYPE=bf16: Linear layers over batch x tokens rows run on the bf16 MFMA kernels (fp32 accumulate,
    fp32 tensors at the boundary).  Checked in a fresh process (the mode is read once) against torch on bf16-rounded inputs."""
    import subprocess, sys
    code = r'''
import sys, os
sys.path[:0] = [%r, %r]
import torch, torch.nn.functional as F
from mmskin import ops
g = torch.Generator().manual_seed(3)
M, K, N = 4096, 256, 192
rb = lambda t: t.bfloat16().float()
x = rb(torch.randn(M, K, generator=g)); w = rb(torch.randn(N, K, generator=g) / K ** 0.5); b = torch.randn(N, generator=g)
dy = rb(torch.randn(M, N, generator=g))
xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
y_ref = F.linear(xr, wr, br); y_ref.backward(dy)
xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, w, b))
y = ops.linear(xd, wd, bd, False); y.backward(dy.cuda())
def l2(a, r): return float((a.cpu().double() - r.double()).norm() / r.double().norm())
errs = [l2(y, y_ref), l2(xd.grad, xr.grad), l2(wd.grad, wr.grad), l2(bd.grad, br.grad)]
print("ERRS", errs)
assert all(e < 1e-2 for e in errs), errs
assert errs[0] > 1e-5      # really the bf16 path (outputs rounded to bf16), not the fp32 one
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MMSKIN_LINEAR_DTYPE="bf16")
    r = subprocess.run([sys.executable, "-c", code % (root, os.path.join(root, "multimodal-model-skin-lesion-classifier_amd"))],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def test_linear_bf16_grouped_tile_order():
    """The grouped tile order of large-weight Linear GEMMs (csrc/conv_gemm.hip conv_gemm_route, group_m: groups of 8 row blocks x all column blocks, on
    for weights above 2 MB with >= 16 row blocks and >= 4 column blocks -- BEiT / BERT fc1, fc2, qkv and their dx GEMMs): M = 19 x 128 rows
    (the last group is ragged: 19 % 8 = 3), K = 1024, N = 2048 in bf16-operand mode, forward and backward, against torch on bf16-rounded
    inputs AND bit-for-bit against the same launches with MMSKIN_GEMM_GROUP_M=0 (the remap only reorders tiles).  Both knobs
    are read once per process -> two fresh interpreters, tensors exchanged through a file."""
    import subprocess, sys, tempfile
    code = r'''
import sys, os
sys.path[:0] = [%r, %r]
import torch, torch.nn.functional as F
from mmskin import ops
g = torch.Generator().manual_seed(5)
M, K, N = 19 * 128, 1024, 2048
rb = lambda t: t.bfloat16().float()
x = rb(torch.randn(M, K, generator=g)); w = rb(torch.randn(N, K, generator=g) / K ** 0.5); b = torch.randn(N, generator=g)
dy = rb(torch.randn(M, N, generator=g))
xr, wr, br = (t.clone().double().requires_grad_(True) for t in (x, w, b))
y_ref = F.linear(xr, wr, br); y_ref.backward(dy.double())
xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, w, b))
y = ops.linear(xd, wd, bd, False); y.backward(dy.cuda())
def l2(a, r): return float((a.cpu().double() - r.double()).norm() / r.double().norm())
errs = [l2(y, y_ref), l2(xd.grad, xr.grad), l2(wd.grad, wr.grad), l2(bd.grad, br.grad)]
print("ERRS", errs)
assert all(e < 5e-3 for e in errs), errs
torch.save([t.detach().cpu() for t in (y, xd.grad, wd.grad, bd.grad)], sys.argv[1])
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the forward launch of the case: 19 row blocks x 16 column blocks of the 128-row tile, grouped by 8 (80 tiles of 256 rows: not pipelined)
    assert CR.route(_lib.load(), CR.FWD, CR.linear(19 * 128, 1024, 2048), CR.BF16, CR.BIAS | CR.OUT_F32) == (CR.CG_TILE128, 128, 128, 128, 2, 2, 8, 19, 16)
    outs = []
    with tempfile.TemporaryDirectory() as td:
        for gm in ("8", "0"):
            f = os.path.join(td, f"g{gm}.pt")
            env = dict(os.environ, MMSKIN_LINEAR_DTYPE="bf16", MMSKIN_GEMM_GROUP_M=gm)
            r = subprocess.run([sys.executable, "-c", code % (root, os.path.join(root, "multimodal-model-skin-lesion-classifier_amd")), f],
                               env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            outs.append(torch.load(f, weights_only=True))
    for a, b in zip(*outs):
        assert torch.equal(a, b), "grouped and plain tile orders differ"


@pytest.mark.parametrize("blocks", ["3", "7"])
def test_wgrad3x3_multi_stage_splits(blocks):
    """All-taps 3x3 weight gradient with few workgroups (MMSKIN_WGRAD3_BLOCKS, read once -> fresh process).  The knob belongs to the
    register-staged all-taps kernel (WG_TAPS3), which runs only where the ring refuses the shape: the first three shapes run the ring
    (WG_RING3, asserted), the fourth -- 12 rows of 5 per stage, three stages per image with a ragged last one (30 = 12 + 12 + 6), 111
    stages -- runs WG_TAPS3 over 3 splits of 37 stages or 6 of 19, so splits start inside images.  Family, tile and split count come from
    the route table (tests/wgrad_plan_cases.py) and are asserted through mmskin_conv_wgrad_plan.  bf16 path against torch on the same
    inputs, every tap plane separately."""
    import subprocess, sys
    code = r'''
import sys
sys.path[:0] = [%r, %r, %r]
import torch, torch.nn.functional as F
from gpu_util import DEV, conv_backward, rel_err
from mmskin import _lib
from wgrad_plan_cases import MULTI_STAGE_ROWS, TAPS3_KNOB, WG_TAPS3, plan
lib = _lib.load()
g = torch.Generator().manual_seed(11)
for row in MULTI_STAGE_ROWS:
    N, Cin, H, W, Cout = row.shape[:5]
    got = plan(lib, row.shape, 2)
    assert got[:4] == (row.family, row.tile_o, row.tile_k, row.variant), (row, got)
    if row.family == WG_TAPS3:
        assert got[4:6] == TAPS3_KNOB[%r], got
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv2d(xr, wr, stride=1, padding=1)
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    n0 = lib.mmskin_wgrad3_ring_launches()
    dx, dw = conv_backward(dy.to(DEV), x.to(DEV), w.to(DEV), 1, 1, "bf16")
    assert lib.mmskin_wgrad3_ring_launches() == n0 + (0 if row.family == WG_TAPS3 else 1), row
    e = rel_err(dw, wr.grad)
    per_tap = [rel_err(dw[:, :, t // 3, t %% 3], wr.grad[:, :, t // 3, t %% 3]) for t in range(9)]
    print("ERR", (N, Cin, H, W, Cout), e, max(per_tap))
    assert e < 5e-2 and max(per_tap) < 5e-2, (e, per_tap)
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MMSKIN_WGRAD3_BLOCKS=blocks)
    r = subprocess.run([sys.executable, "-c", code % (os.path.join(root, "tests"), root,
                                                     os.path.join(root, "multimodal-model-skin-lesion-classifier_amd"), blocks)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
