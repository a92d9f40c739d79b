"""-m gpu: the ring weight-gradient kernel (csrc/wgrad_ring.hip: LDS-DMA ring with counted vmcnt, 8 waves, pixel groups reduced
through LDS) against torch's conv2d weight gradient (the ATen op the reference reaches through loss.backward(), train_pad_20.py:112).

Inputs are bf16-REPRESENTABLE, so the bf16 kernel multiplies exactly what the fp64 reference multiplies and the only difference left
is the fp32 accumulation order: the bound is 1e-4 of the gradient's rms on the WORST element (measured ~2e-6), i.e. one dropped
8-pixel fragment, one stale ring slot or one row taken from the neighbouring split fails it -- unlike the 5e-2 bf16 bound of
test_gpu_kernels.py, which has to absorb operand rounding.  Every case asserts through mmskin_conv_wgrad_plan that the library
plans the family, tile and variant the route table (tests/wgrad_plan_cases.py) names for it, and through mmskin_wgrad_ring_launches() that the ring
kernel is what ran.  Measured errors go to gpurun_out/parity_report.jsonl."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV, conv_backward, rel_err
from mmskin import _lib
from wgrad_plan_cases import BF16, RING3_ROWS, RING_ROWS, WG_RING, WG_RING3, plan

pytestmark = pytest.mark.gpu
REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity_report.jsonl")
TOL = 1e-4

# N, Cin, H, W, Cout, k, stride, pad, what -- with the family and tile every case must run, from the route table (tests/wgrad_plan_cases.py)
CASES = [r.shape + (r.note,) for r in RING_ROWS]


def _record(**kw):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(json.dumps(kw) + "\n")


def _bf16_exact(t):
    return t.bfloat16().float()


@pytest.mark.parametrize("case", CASES, ids=[f"c{i}" for i in range(len(CASES))])
def test_ring_wgrad_matches_fp64_reference(case):
    N, Cin, H, W, Cout, k, stride, pad, what = case
    lib = _lib.load()
    g = torch.Generator().manual_seed(sum(case[:8]))
    x = _bf16_exact(torch.randn(N, Cin, H, W, generator=g))
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = _bf16_exact(torch.randn(N, Cout, OH, OW, generator=g))
    xr, wr = x.double(), w.double().requires_grad_(True)
    F.conv2d(xr, wr, stride=stride, padding=pad).backward(dy.double())
    row = RING_ROWS[CASES.index(case)]
    assert row.family == WG_RING and plan(lib, row.shape, BF16)[:4] == (row.family, row.tile_o, row.tile_k, row.variant), (what, plan(lib, row.shape, BF16))
    n0 = lib.mmskin_wgrad_ring_launches()
    _, dw = conv_backward(dy.to(DEV), x.to(DEV), w.to(DEV), stride, pad, "bf16")
    assert lib.mmskin_wgrad_ring_launches() == n0 + 1, "ring kernel not selected"
    err = rel_err(dw, wr.grad)
    d = (dw.double().cpu() - wr.grad)
    rms_err = float(d.pow(2).mean().sqrt())
    worst_over_rms = float(d.abs().max()) / (rms_err + 1e-30)
    _record(test="wgrad_ring", case=list(case[:8]), what=what, max_err_over_rms=err, worst_over_rms_err=worst_over_rms)
    assert err < TOL, (what, err)


# N, Cin, H, W, Cout, what  (3x3 / stride 1 / pad 1: csrc/wgrad3_ring.hip)
CASES3 = [r.shape[:5] + (r.note,) for r in RING3_ROWS]


@pytest.mark.parametrize("case", CASES3, ids=[f"k{i}" for i in range(len(CASES3))])
def test_ring_wgrad3x3_matches_fp64_reference(case):
    N, Cin, H, W, Cout, what = case
    lib = _lib.load()
    g = torch.Generator().manual_seed(sum(case[:5]))
    x = _bf16_exact(torch.randn(N, Cin, H, W, generator=g))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    dy = _bf16_exact(torch.randn(N, Cout, H, W, generator=g))
    wr = w.double().requires_grad_(True)
    F.conv2d(x.double(), wr, stride=1, padding=1).backward(dy.double())
    row = RING3_ROWS[CASES3.index(case)]
    assert row.family == WG_RING3 and plan(lib, row.shape, BF16)[:4] == (row.family, row.tile_o, row.tile_k, row.variant), (what, plan(lib, row.shape, BF16))
    n0 = lib.mmskin_wgrad3_ring_launches()
    _, dw = conv_backward(dy.to(DEV), x.to(DEV), w.to(DEV), 1, 1, "bf16")
    assert lib.mmskin_wgrad3_ring_launches() == n0 + 1, "3x3 ring kernel not selected"
    err = rel_err(dw, wr.grad)
    # every tap separately: a wrong window row / column offset shows in one tap plane only
    per_tap = [rel_err(dw[:, :, t // 3, t % 3], wr.grad[:, :, t // 3, t % 3]) for t in range(9)]
    _record(test="wgrad3_ring", case=list(case[:5]), what=what, max_err_over_rms=err, worst_tap=max(per_tap))
    assert err < TOL and max(per_tap) < TOL, (what, err, per_tap)


def test_ring_wgrad_is_bit_identical_across_repeats():
    """A race in the ring (a fragment read overtaking its DMA, a refill overtaking a read, the group reduction overtaking the drain of
    the trailing pieces) shows as run-to-run differences: 100 launches of a multi-split two-group layer must give one result."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    x = _bf16_exact(torch.randn(64, 64, 28, 28, generator=g)).to(DEV)
    dy = _bf16_exact(torch.randn(64, 256, 28, 28, generator=g)).to(DEV)
    w = torch.zeros(256, 64, 1, 1, device=DEV)
    n0 = lib.mmskin_wgrad_ring_launches()
    _, ref = conv_backward(dy, x, w, 1, 0, "bf16")
    assert lib.mmskin_wgrad_ring_launches() == n0 + 1
    for i in range(100):
        _, dw = conv_backward(dy, x, w, 1, 0, "bf16")
        assert torch.equal(dw, ref), i
    # and the 3x3 ring (two groups, ring of two iterations: the tightest WAR distance)
    x3 = _bf16_exact(torch.randn(32, 64, 28, 28, generator=g)).to(DEV)
    dy3 = _bf16_exact(torch.randn(32, 64, 28, 28, generator=g)).to(DEV)
    w3 = torch.zeros(64, 64, 3, 3, device=DEV)
    n0 = lib.mmskin_wgrad3_ring_launches()
    _, ref3 = conv_backward(dy3, x3, w3, 1, 1, "bf16")
    assert lib.mmskin_wgrad3_ring_launches() == n0 + 1
    for i in range(100):
        _, dw = conv_backward(dy3, x3, w3, 1, 1, "bf16")
        assert torch.equal(dw, ref3), i
