"""-m gpu: the pooling kernels of the VGG plan (csrc/vgg.hip) on their own, through mmskin_maxpool2_relu_* and mmskin_adaptive_avgpool_*,
against plain torch in fp64 on the CPU.  Cases: tests/densenet_cases.py (MAXPOOL_CASES, ADAPTIVE_CASES; checked on the CPU by
tests/test_cpu_densenet_cases.py).

Max-pool: no arithmetic, so value, index and the routed gradient are EXACT in both element types; the inputs hold equal positive maxima at
every pair of taps and an all-zero window, so the tie-break against F.max_pool2d(return_indices=True) is decided by the data.
Adaptive average pool: fp32 rel_err < 2e-4; bf16 dx (stored once in bf16) within half a bf16 ulp and relative L2 < 1e-3 of the rounded
reference; the forward output is fp32 in both element types (fp32 bound)."""
import pytest
import torch
import torch.nn.functional as F

from densenet_cases import ADAPTIVE_CASES, MAXPOOL_CASES, maxpool_backward_reference, maxpool_input, maxpool_reference
from gpu_util import DEV, DT, rel_err, ws
from mbconv_cases import rb
from mmskin import _lib
from mmskin._lib import call, ptr, stream
from test_gpu_mbconv_ops import check_tensor, report

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", MAXPOOL_CASES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool2_value_index_and_routed_gradient_are_exact(shape, dtype):
    N, C, H, W = shape
    PH, PW = H // 2, W // 2
    y, plants = maxpool_input(N, C, H, W)
    pooled_ref, tap_ref = maxpool_reference(y)
    g = torch.Generator().manual_seed(H + W)
    dpool = rb(torch.randn(N, C, PH, PW, generator=g))
    dpool[dpool == 0] = 1.0
    dz_ref = maxpool_backward_reference(y, tap_ref, dpool)
    lib = _lib.load()
    wsp = ws(lib.mmskin_maxpool2_relu_workspace_bytes(N, C, H, W))
    yd, dpd = y.to(DEV), dpool.to(DEV)
    pooled = torch.full((N, C, PH, PW), float("nan"), device=DEV)
    idx = torch.full((N, PH, PW, C), 255, dtype=torch.uint8, device=DEV)
    dz = torch.full((N, C, H, W), float("nan"), device=DEV)
    call("mmskin_maxpool2_relu_forward", ptr(yd), ptr(pooled), ptr(idx), N, C, H, W, DT[dtype], ptr(wsp), stream())
    call("mmskin_maxpool2_relu_backward", ptr(dpd), ptr(yd), ptr(dz), N, C, H, W, DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    tap = idx.cpu().permute(0, 3, 1, 2)
    assert torch.equal(pooled.cpu().double(), pooled_ref), "pooled value"
    for n, c, ph, pw, first in plants:
        assert int(tap[n, c, ph, pw]) == first, ("tie-break", (n, c, ph, pw), int(tap[n, c, ph, pw]), first)
    assert torch.equal(tap, tap_ref), "argmax tap"
    assert torch.equal(dz.cpu().double(), dz_ref), "dz is dpool routed to the argmax where y > 0, else zero"
    if H % 2:
        assert float(dz[:, :, -1].abs().max()) == 0.0
    if W % 2:
        assert float(dz[:, :, :, -1].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", ADAPTIVE_CASES, ids=lambda s: "x".join(map(str, s)))
def test_adaptive_avgpool_to_7x7(shape, dtype):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(H * 100 + W + C)
    x = rb(torch.randn(N, C, H, W, generator=g))
    dout = rb(torch.randn(N, C, 7, 7, generator=g))
    xd = x.double().requires_grad_(True)
    out_ref = F.adaptive_avg_pool2d(xd, 7)
    out_ref.backward(dout.double())
    lib = _lib.load()
    wsp = ws(lib.mmskin_adaptive_avgpool_workspace_bytes(N, C, H, W))
    xg, dg = x.to(DEV), dout.to(DEV)
    out = torch.full((N, C, 7, 7), float("nan"), device=DEV)
    dx = torch.full((N, C, H, W), float("nan"), device=DEV)
    call("mmskin_adaptive_avgpool_forward", ptr(xg), ptr(out), N, C, H, W, DT[dtype], ptr(wsp), stream())
    call("mmskin_adaptive_avgpool_backward", ptr(dg), ptr(dx), N, C, H, W, DT[dtype], ptr(wsp), stream())
    torch.cuda.synchronize()
    rec = dict(test="vgg_adaptive_avgpool", shape=list(shape), dtype=dtype, out=rel_err(out, out_ref))
    try:
        assert rec["out"] < 2e-4, rec
        check_tensor("dx", dx, xd.grad, dtype, rec)
        if (H, W) == (7, 7):   # the identity
            assert torch.equal(out.cpu(), x) and torch.equal(dx.cpu(), dout)
    finally:
        report(**rec)


def test_pools_refuse_a_map_smaller_than_the_window():
    lib = _lib.load()
    t = torch.zeros(4096, device=DEV)
    out = torch.full((4096,), 5.0, device=DEV)
    idx = torch.full((4096,), 9, dtype=torch.uint8, device=DEV)
    big = ws(1 << 20)
    for args in ((1, 64, 1, 4), (1, 64, 4, 1), (1, 60, 4, 4)):   # H < 2, W < 2, C not a multiple of the chunk
        with pytest.raises(_lib.MMSkinError):
            call("mmskin_maxpool2_relu_forward", ptr(t), ptr(out), ptr(idx), *args, DT["fp32"], ptr(big), stream())
        with pytest.raises(_lib.MMSkinError):
            call("mmskin_maxpool2_relu_backward", ptr(t), ptr(t), ptr(out), *args, DT["bf16"], ptr(big), stream())
        assert lib.mmskin_last_error() and lib.mmskin_maxpool2_relu_workspace_bytes(*args) == -1
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((idx == 9).all()), "a refused call wrote to an output"
