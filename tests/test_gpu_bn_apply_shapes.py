"""-m gpu: the two element-wise BatchNorm apply passes (bn_apply, bn_bwd_apply of csrc/bn.hip) at the shapes where their column-stationary,
four-rows-per-thread launch geometry can go wrong, through mmskin_bn_apply_rows / mmskin_bn_bwd_apply_rows on [rows][C] tensors.

Geometry under test (apply_geom): a 256-thread block is CW = min(C / EPC, 256) chunk columns x RL = 256 / CW row lanes and does 4 * RL rows.
  C = 8 bf16 / 4 fp32  one chunk per row: 256 row lanes, 1024 rows per block (4099 rows: 5 blocks, the last with 3 rows)
  C = 64               8 (bf16) / 16 (fp32) chunks per row
  C = 200 bf16         25 chunks per row: 10 row lanes, 6 idle threads per block
  C = 2048 bf16        256 chunks per row: one row lane, 4 rows per block
  rows = 1, 3          fewer rows than one thread's group; 5, 197, 4099: whole groups and a ragged last one, more than one block

Reference: the same expressions in fp64 on the device.  Every operand that decides a mask (x, scale, shift, the residual and its
coefficients, ymask) is a small dyadic rational, so x * scale + shift is exact in fp32 and in fp64 alike and the two agree on every sign; the
operands that do not (dy, cA, cB, cC) are normal deviates, rounded to bf16 where the tensor is bf16.  Bound: the per-element bound of the
BatchNorm cases of test_gpu_kernels.py, max |got - want| / rms(want) < TOL forward and < 3 TOL backward (TOL 2e-4 fp32, 5e-2 bf16).  Each
launch runs twice into separate buffers that must be bit-equal, and no launch may touch the guard elements behind its outputs.
"""
import pytest
import torch

from gpu_util import DEV, DT, rel_err
from mmskin._lib import call, ptr, stream

pytestmark = pytest.mark.gpu
TOL = {"fp32": 2e-4, "bf16": 5e-2}
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
EPC = {"fp32": 4, "bf16": 8}
MASK_NONE, MASK_FROM_X, MASK_FROM_Y, MASK_FROM_Y6, MASK_SILU_X = range(5)
GUARD = 256
SHAPES = [(dt, C, rows) for dt, Cs in (("bf16", (8, 64, 200, 2048)), ("fp32", (4, 64))) for C in Cs for rows in (1, 3, 5, 197, 4099)]


def dyadic(gen, shape, lo, hi, den, dtype=torch.float32):
    """integers of [lo, hi) over den: exact in bf16 for |numerator| < 256"""
    return (torch.randint(lo, hi, shape, generator=gen).float() / den).to(dtype).to(DEV)


def guarded(rows, C, dtype):
    """an output buffer with GUARD sentinel elements behind its rows * C"""
    buf = torch.full((rows * C + GUARD,), 512.0, dtype=dtype, device=DEV)
    return buf


def payload(buf, rows, C):
    assert bool((buf[rows * C:] == 512.0).all()), "the launch wrote behind its last row"
    return buf[:rows * C].view(rows, C)


def forward_inputs(dt, C, rows):
    g = torch.Generator().manual_seed(1000 * C + rows)
    td = TORCH_DT[dt]
    x = dyadic(g, (rows, C), -64, 64, 8, td)
    res = dyadic(g, (rows, C), -64, 64, 8, td)
    sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
    scale = (torch.randint(1, 9, (C,), generator=g).float() / 4 * sign).to(DEV)
    shift = dyadic(g, (C,), -16, 16, 16)
    rscale = dyadic(g, (C,), 1, 9, 4)
    rshift = dyadic(g, (C,), -16, 16, 16)
    return x, res, scale, shift, rscale, rshift


@pytest.mark.parametrize("dt,C,rows", SHAPES)
def test_bn_apply_every_residual_mode_with_and_without_mask_bytes(dt, C, rows):
    x, res, scale, shift, rscale, rshift = forward_inputs(dt, C, rows)
    td, epc = TORCH_DT[dt], EPC[dt]
    x64, r64 = x.double(), res.double()
    pre = {0: x64 * scale.double() + shift.double()}
    pre[1] = pre[0] + r64
    pre[2] = pre[0] + (r64 * rscale.double() + rshift.double())
    weights = (2 ** torch.arange(epc, device=DEV)).long()
    # (relu, cap): none, ReLU, ReLU6, SiLU; the mask bytes are the ReLU mask of backward, asked for with none and ReLU
    for mode in (0, 1, 2):
        for relu, cap in ((1, 0.0), (0, 0.0), (1, 6.0), (1, -1.0)):
            t = pre[mode]
            want = t if not relu else t * torch.sigmoid(t) if cap < 0 else t.clamp(min=0.0) if cap == 0 else t.clamp(min=0.0, max=cap)
            for with_mask in ((False, True) if cap == 0.0 else (False,)):
                runs = []
                for _ in range(2):
                    y = guarded(rows, C, td)
                    mb = torch.full((rows * C // epc + GUARD,), 0xEE, dtype=torch.uint8, device=DEV) if with_mask else None
                    call("mmskin_bn_apply_rows", ptr(x), ptr(res) if mode else None, ptr(scale), ptr(shift), ptr(rscale) if mode == 2 else None,
                         ptr(rshift) if mode == 2 else None, ptr(y), ptr(mb), rows, C, relu, cap, DT[dt], stream())
                    torch.cuda.synchronize()
                    runs.append((y, mb))
                y = payload(runs[0][0], rows, C)
                tag = (dt, C, rows, mode, relu, cap, with_mask)
                print(tag, "max err / rms", rel_err(y, want))
                assert rel_err(y, want) < TOL[dt], (tag, rel_err(y, want))
                assert torch.equal(runs[0][0], runs[1][0]), tag
                if with_mask:
                    mb = runs[0][1]
                    assert bool((mb[rows * C // epc:] == 0xEE).all()), tag
                    bits = ((want > 0).view(rows, C // epc, epc).long() * weights).sum(-1).to(torch.uint8).flatten()   # stored y > 0
                    assert torch.equal(mb[:rows * C // epc], bits), tag
                    assert torch.equal(runs[0][1], runs[1][1]), tag


@pytest.mark.parametrize("dt,C,rows", SHAPES)
def test_bn_bwd_apply_every_mask_mode_with_and_without_dz(dt, C, rows):
    x, ymask, scale, shift, _, _ = forward_inputs(dt, C, rows)   # ymask in [-8, 8): both ends of the ReLU6 window are inside
    td = TORCH_DT[dt]
    g = torch.Generator().manual_seed(2000 * C + rows)
    dy = torch.randn((rows, C), generator=g).to(td).to(DEV)
    cA, cB, cC = ((torch.randn(C, generator=g) * s).to(DEV) for s in (1.0, 0.25, 0.5))
    x64, y64, dy64 = x.double(), ymask.double(), dy.double()
    t = x64 * scale.double() + shift.double()
    sg = torch.sigmoid(t)
    dz_want = {MASK_NONE: dy64, MASK_FROM_X: dy64 * (t > 0), MASK_FROM_Y: dy64 * (y64 > 0), MASK_FROM_Y6: dy64 * ((y64 > 0) & (y64 < 6)),
               MASK_SILU_X: dy64 * (sg * (1 + t * (1 - sg)))}
    for mode, dzw in dz_want.items():
        dxw = cA.double() * dzw + cB.double() * x64 + cC.double()
        for with_dz in (False, True):
            runs = []
            for _ in range(2):
                dx, dz = guarded(rows, C, td), guarded(rows, C, td) if with_dz else None
                call("mmskin_bn_bwd_apply_rows", ptr(dy), ptr(x), ptr(ymask), ptr(scale), ptr(shift), mode, ptr(cA), ptr(cB), ptr(cC), ptr(dx),
                     ptr(dz), rows, C, DT[dt], stream())
                torch.cuda.synchronize()
                runs.append((dx, dz))
            tag = (dt, C, rows, mode, with_dz)
            dx = payload(runs[0][0], rows, C)
            print(tag, "dx max err / rms", rel_err(dx, dxw))
            assert rel_err(dx, dxw) < 3 * TOL[dt], (tag, rel_err(dx, dxw))
            assert torch.equal(runs[0][0], runs[1][0]), tag
            if with_dz:
                dz = payload(runs[0][1], rows, C)
                assert rel_err(dz, dzw) < 3 * TOL[dt], (tag, rel_err(dz, dzw))
                assert torch.equal(runs[0][1], runs[1][1]), tag
