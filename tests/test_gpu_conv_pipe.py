"""-m gpu: the 8-phase pipelined conv / dgrad kernel (csrc/conv_gemm.hip, NST == 8: 224 / 256-row x 256-channel tiles, LDS-DMA ring with
counted vmcnt, two wave groups one barrier apart) against torch's conv2d on the same inputs.

The kernel is selected per launch by a tile-count model and a minimum reduction depth; here MMSKIN_CONV_PIPE_FORCE=1 sends every eligible
launch to it and MMSKIN_CONV_PIPE_TILE pins the tile height (256 / 224 computed rows, or 196 valid rows of a 224-row tile), so every tile
shape meets every case: ragged last row blocks, M smaller than one tile, stride-2 gathers, the four parity classes of a stride-2 dgrad,
a one-K-tile reduction (prologue-only pipeline) and 72 K-tiles.  Both knobs are read once per process -> fresh interpreters.
Reference semantics: F.conv2d forward / backward as reached through torchvision's ResNet (loadImageModelClassifier.py:65-75).
Tolerance (round 4): inputs, weights and upstream gradients are bf16-REPRESENTABLE and the reference runs in fp64,
so the only error left is the bf16 rounding of the stored result: EVERY element within half a bf16 ulp (2^-8 relative) of the exact value,
and against the reference ROUNDED to bf16 the relative L2 is < 1e-3 (only rounding ties may differ) -- one dropped 8-element fragment of a
K = 4608 reduction moves an element by ~4e-2 of the rms and fails both.  Measured errors go to
gpurun_out/parity_report.jsonl."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CODE = r'''
import sys
sys.path[:0] = [%(tests)r, %(root)r, %(pkg)r]
import json, os, torch, torch.nn.functional as F
import conv_route_cases as CR
from gpu_util import DEV, conv_backward, conv_forward, rel_err
from mmskin import _lib
lib = _lib.load()
REPORT = os.path.join(%(root)r, "gpurun_out", "parity_report.jsonl")
def rb(t): return t.bfloat16().float()
def l2r(got, want):
    got, want = got.double().cpu(), rb(want.float()).double()
    return float((got - want).norm() / want.norm())
CASES = [  # N, Cin, H, W, Cout, k, stride, pad, pipe launches expected (forward, dgrad)
    (3, 256, 14, 14, 256, 3, 1, 1, 1, 1),     # layer3 3x3: 588 rows = 3 images of 196
    (2, 256, 28, 28, 256, 3, 2, 1, 1, 1),     # stride-2 3x3: strided gather forward, four parity classes backward
    (2, 512, 9, 11, 256, 1, 1, 0, 1, 1),      # 1x1, odd sizes, ragged last row block
    (1, 256, 7, 7, 512, 3, 1, 1, 1, 1),       # fewer rows than one tile, 36 K-tiles
    (2, 256, 14, 14, 512, 1, 2, 0, 1, 1),     # stride-2 1x1 downsample: zero-filled parity classes + one GEMM class
    (5, 64, 14, 14, 256, 1, 1, 0, 1, 0),      # ONE K-tile forward (the ring never refills); its dgrad has Cin = 64 outputs: 128-row kernel
    (4, 128, 14, 14, 256, 3, 1, 1, 1, 0),     # 18 K-tiles of a 128-channel input
    (1, 512, 7, 7, 512, 3, 1, 1, 1, 1),       # 72 K-tiles
    (2, 256, 15, 13, 256, 3, 2, 1, 1, 1),     # stride 2 on odd sizes
]
g = torch.Generator().manual_seed(5)
for (N, Cin, H, W, Cout, k, s, p, ef, eb) in CASES:
    x = rb(torch.randn(N, Cin, H, W, generator=g))
    w = rb(torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, stride=s, padding=p)
    dy = rb(torch.randn(y_ref.shape, generator=g))
    y_ref.backward(dy.double())
    for op, taken in ((CR.FWD, ef), (CR.DGRAD, eb)):   # the route the counters below confirm: the pinned tile, or the 128-row family
        r = CR.route(lib, op, (N, Cin, H, W, Cout, k, s, p), CR.BF16)
        assert r[:6] == ((CR.CG_PIPE,) + CR.KNOB_TILES[os.environ["MMSKIN_CONV_PIPE_TILE"]][:2] + (256, 8, 0) if taken else (CR.CG_TILE128, 128, 128, 128 if Cin %% 128 == 0 else 64, 2, 0)), (op, r)   # only data gradients (Cin columns) decline
    n0 = lib.mmskin_conv_pipe_launches()
    y = conv_forward(x.to(DEV), w.to(DEV), s, p, "bf16")
    n1 = lib.mmskin_conv_pipe_launches()
    dx, dw = conv_backward(dy.to(DEV), x.to(DEV), w.to(DEV), s, p, "bf16")
    n2 = lib.mmskin_conv_pipe_launches()
    ef_, eb_ = rel_err(y, y_ref), rel_err(dx, xr.grad)
    lf_, lb_ = l2r(y, y_ref.detach()), l2r(dx, xr.grad)
    print("CASE", (N, Cin, H, W, Cout, k, s, p), "fwd", ef_, lf_, "dgrad", eb_, lb_, "pipe launches", n1 - n0, n2 - n1, flush=True)
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(json.dumps(dict(test="conv_pipe", tile=os.environ.get("MMSKIN_CONV_PIPE_TILE"), case=[N, Cin, H, W, Cout, k, s, p], fwd_max_err_over_rms=ef_,
                                fwd_rel_l2_vs_bf16_rounded_ref=lf_, dgrad_max_err_over_rms=eb_, dgrad_rel_l2_vs_bf16_rounded_ref=lb_)) + "\n")
    assert n1 - n0 == ef and n2 - n1 == eb, "pipelined kernel not selected as expected"
    for got, want in ((y, y_ref.detach()), (dx, xr.grad)):   # every stored element within half a bf16 ulp (2^-8 relative) of the exact value
        got, want = got.double().cpu(), want.double()
        assert bool(((got - want).abs() <= want.abs() * 2.0 ** -8 + 1e-5 * float(want.pow(2).mean().sqrt())).all()), (ef_, eb_)
    assert lf_ < 1e-3 and lb_ < 1e-3, (lf_, lb_)
'''


@pytest.mark.parametrize("tile", ["256", "224", "196"])
def test_pipelined_conv_kernel_matches_torch(tile):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MMSKIN_CONV_PIPE_FORCE="1", MMSKIN_CONV_PIPE_TILE=tile)
    code = CODE % dict(tests=os.path.join(root, "tests"), root=root,
                       pkg=os.path.join(root, "multimodal-model-skin-lesion-classifier_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]


def test_pipelined_conv_kernel_is_bit_identical_across_repeats():
    """A race in the LDS ring (a fragment read overtaking its DMA, or a refill overtaking a read) shows up as run-to-run differences:
    200 launches of a 36-K-tile layer must give one result."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import sys
sys.path[:0] = [%(tests)r, %(root)r, %(pkg)r]
import torch
from gpu_util import DEV, conv_forward
from mmskin import _lib
lib = _lib.load()
g = torch.Generator().manual_seed(9)
x = torch.randn(64, 256, 14, 14, generator=g).to(DEV)
w = (torch.randn(256, 256, 3, 3, generator=g) / 48).to(DEV)
ref = conv_forward(x, w, 1, 1, "bf16")
assert lib.mmskin_conv_pipe_launches() == 1
for i in range(200):
    y = conv_forward(x, w, 1, 1, "bf16")
    assert torch.equal(y, ref), i
print("OK")
''' % dict(tests=os.path.join(root, "tests"), root=root, pkg=os.path.join(root, "multimodal-model-skin-lesion-classifier_amd"))
    env = dict(os.environ, MMSKIN_CONV_PIPE_FORCE="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]


C3_CODE = r'''
import sys
sys.path[:0] = [%(tests)r, %(root)r, %(pkg)r]
import torch, torch.nn.functional as F
from gpu_util import DEV, conv_backward, conv_forward, rel_err
from mmskin import _lib
lib = _lib.load()
EXPECT_C64 = %(expect)d
g = torch.Generator().manual_seed(13)
for (N, H) in [(3, 56), (2, 8), (1, 12), (2, 20)]:
    x = torch.randn(N, 64, H, 56, generator=g)
    w = torch.randn(64, 64, 3, 3, generator=g) / 24
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y_ref = F.conv2d(xr, wr, stride=1, padding=1)
    dy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(dy)
    n0 = lib.mmskin_conv3x3_c64_launches()
    y = conv_forward(x.to(DEV), w.to(DEV), 1, 1, "bf16")
    dx, dw = conv_backward(dy.to(DEV), x.to(DEV), w.to(DEV), 1, 1, "bf16")
    assert lib.mmskin_conv3x3_c64_launches() - n0 == 2 * EXPECT_C64, "layer-1 3x3 kernel selection"
    ef, eb = rel_err(y, y_ref), rel_err(dx, xr.grad)
    print("CASE", (N, H), "fwd", ef, "dgrad", eb, flush=True)
    assert ef < 5e-2 and eb < 5e-2
    # every border pixel and the interior separately: a wrong ring slot or a missing zero row shows at the image edges first
    for name, got, want in (("fwd", y.cpu(), y_ref.detach()), ("dgrad", dx.cpu(), xr.grad)):
        for sl in ((slice(None), slice(None), 0), (slice(None), slice(None), H - 1), (slice(None), slice(None), slice(None), 0), (slice(None), slice(None), slice(None), 55)):
            assert rel_err(got[sl], want[sl]) < 5e-2, (name, sl)
'''


@pytest.mark.parametrize("on", ["1", "0"])
def test_layer1_3x3_all_taps_kernel_matches_torch(on):
    """conv3x3_c64.hip (64 -> 64 channels, 3x3 / stride 1 / pad 1 at width 56: ResNet-50 layer1 conv2), forward and data gradient, against
    torch's conv2d: image heights of 14 / 2 / 3 / 5 four-row tiles (ring wrap-around, the zero row above the first and below the last
    tile), borders checked separately.  MMSKIN_CONV3X3_C64_MIN_N=1 sends the small batches to it; on = 0 runs the same cases on the
    tapped kernel (the A/B knob must keep working).  Tolerance: the bf16 kernel bound of test_gpu_kernels.py."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MMSKIN_CONV3X3_C64=on, MMSKIN_CONV3X3_C64_MIN_N="1")
    code = C3_CODE % dict(tests=os.path.join(root, "tests"), root=root, pkg=os.path.join(root, "multimodal-model-skin-lesion-classifier_amd"), expect=int(on))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]


FUSED_CODE = r'''
import sys, ctypes
sys.path[:0] = [%(tests)r, %(root)r, %(pkg)r]
import torch, torch.nn.functional as F
import conv_route_cases as CR
from gpu_util import DEV, rel_err, ws
from mmskin import _lib
from mmskin._lib import call, ptr, stream
lib = _lib.load()
rb = lambda t: t.bfloat16().float()
g = torch.Generator().manual_seed(21)
# N, Cin, H, W, Cout, k, stride, pad, layer-1 kernel expected
for (N, Cin, H, W, Cout, k, s, p, c64) in [(3, 64, 56, 56, 64, 3, 1, 1, %(expect)d), (2, 64, 14, 14, 256, 1, 1, 0, 0), (2, 128, 12, 12, 128, 3, 1, 1, 0), (2, 256, 9, 11, 128, 1, 1, 0, 0)]:
    x_in = torch.randn(N, Cin, H, W, generator=g)
    w = rb(torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5)
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = rb(torch.randn(N, Cout, OH, OW, generator=g))
    xc = rb(torch.randn(N, Cin, H, W, generator=g))                      # raw BatchNorm input of the unit that produced this conv's input
    scale = torch.rand(Cin, generator=g) + 0.5; shift = torch.randn(Cin, generator=g) * 0.3
    xin = x_in.double().requires_grad_(True)
    F.conv2d(xin, w.double(), stride=s, padding=p).backward(dy.double())
    mask = (xc.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)) > 0
    dz_ref = xin.grad * mask
    rows = lib.mmskin_conv2d_dgrad_fused_rows(N, Cin, H, W, Cout, k, k, s, p)
    dz = torch.empty(N, Cin, H, W, device=DEV); part = torch.zeros(rows, 2, Cin, device=DEV)
    nw = ctypes.c_int(0)
    wsp = ws(lib.mmskin_conv2d_workspace_bytes(N, Cin, H, W, Cout, k, k, s, p))
    dev = [t.to(DEV) for t in (dy, w, xc, scale, shift)]
    r = CR.route(lib, CR.DGRAD, (N, Cin, H, W, Cout, k, s, p), CR.BF16, CR.EPI_FLAGS[3])   # profile 3 of the 128-row tile, or its twin
    assert r[0] == CR.CG_C64 if c64 else r[:6] == (CR.CG_TILE128, 128, 128, 128 if Cin %% 128 == 0 else 64, 2, 3), r
    n0 = lib.mmskin_conv3x3_c64_launches()
    call("mmskin_conv2d_dgrad_fused", *[ptr(t) for t in dev], ptr(dz), ptr(part), ctypes.addressof(nw), N, Cin, H, W, Cout, k, k, s, p, ptr(wsp), stream())
    torch.cuda.synchronize()
    assert lib.mmskin_conv3x3_c64_launches() - n0 == c64, "kernel selection"
    e = rel_err(dz, dz_ref)
    # the sums are taken on the STORED (bf16) dz: compare with sums of the returned dz, and with the exact ones loosely
    sums = part[: nw.value].double().sum(0).cpu()
    dzs = dz.double().cpu()
    s1, s2 = dzs.sum((0, 2, 3)), (dzs * xc.double()).sum((0, 2, 3))
    e1 = float((sums[0] - s1).abs().max() / (s1.abs().max() + 1e-30)); e2 = float((sums[1] - s2).abs().max() / (s2.abs().max() + 1e-30))
    print("CASE", (N, Cin, H, W, Cout, k), "dz", e, "sum dz", e1, "sum dz x", e2, "rows", nw.value, flush=True)
    ok = ((dz.double().cpu() - dz_ref).abs() <= dz_ref.abs() * 2.0 ** -8 + 1e-5 * float(dz_ref.pow(2).mean().sqrt())).all()
    assert bool(ok), "dz off by more than half a bf16 ulp"
    assert e1 < 1e-4 and e2 < 1e-4, (e1, e2)
'''


@pytest.mark.parametrize("on", ["1", "0"])
def test_dgrad_with_fused_batchnorm_backward_epilogue(on):
    """The data gradient with the consumer's BatchNorm-backward prologue in its epilogue (mask from x * scale + shift, sums of dz and
    dz * x per row block: profile 3 of csrc/conv_gemm.hip and its twin in csrc/conv3x3_c64.hip), op level through
    mmskin_conv2d_dgrad_fused -- until round 4 only the ResNet end-to-end tests reached it.  dz: every element within half
    a bf16 ulp of the masked fp64 gradient; the partial rows must sum to the column sums of the dz that was stored (1e-4)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MMSKIN_CONV3X3_C64=on, MMSKIN_CONV3X3_C64_MIN_N="1")
    code = FUSED_CODE % dict(tests=os.path.join(root, "tests"), root=root, pkg=os.path.join(root, "multimodal-model-skin-lesion-classifier_amd"), expect=int(on))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]


def test_two_stage_256x256_tile_matches_fp64():
    """The 256 x 256 two-stage tile (NST 2) is reached only where the pipelined kernel declines a deep plain GEMM; K = 8256 = 129 K-tiles
    (one past its table) is the smallest such reduction: a 1x1 convolution 8256 -> 1024 over 120 x 120 pixels, 57 x 4 = 228 tiles.  Same
    bound as the pipelined cases above: bf16-representable inputs, fp64 reference (taken on the device), every element within half a
    bf16 ulp, relative L2 against the rounded reference < 1e-3."""
    import torch
    import conv_route_cases as CR
    from gpu_util import DEV, conv_forward, rel_err
    from mmskin import _lib
    case = (1, 8256, 120, 120, 1024, 1, 1, 0)
    lib = _lib.load()
    assert CR.route(lib, CR.FWD, case, CR.BF16) == (CR.CG_BIG256, 256, 256, 256, 2, 0, 0, 57, 4)
    n0 = lib.mmskin_conv_pipe_launches()
    g = torch.Generator(device=DEV).manual_seed(31)
    x = torch.randn(1, 8256, 120, 120, generator=g, device=DEV).bfloat16().float()
    w = (torch.randn(1024, 8256, 1, 1, generator=g, device=DEV) / 8256 ** 0.5).bfloat16().float()
    y = conv_forward(x, w, 1, 0, "bf16")
    assert lib.mmskin_conv_pipe_launches() == n0
    want = torch.einsum("chw,oc->ohw", x[0].double(), w[:, :, 0, 0].double())[None]
    got = y.double()
    wr = want.float().bfloat16().double()
    l2 = float((got - wr).norm() / wr.norm())
    print("256x256 two-stage: max err / rms", rel_err(got, want), "rel l2 vs rounded", l2)
    assert bool(((got - want).abs() <= want.abs() * 2.0 ** -8 + 1e-5 * float(want.pow(2).mean().sqrt())).all())
    assert l2 < 1e-3, l2
