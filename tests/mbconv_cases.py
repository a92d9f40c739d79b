"""The MBConv op cases as data, with the launch geometry of csrc/ops.hip recomputed in Python and the fp64 references the op tests
share.  No GPU needed to import: tests/test_cpu_mbconv_cases.py checks every claim made here, tests/test_gpu_mbconv_ops.py runs the cases.

A depthwise case is (N, C, c_valid, H, W, ksize, stride, edge, note): C is the padded channel count the kernels see, c_valid the real one
(weights beyond it are staged as zeros), `edge` names the property test_cpu_mbconv_cases.py asserts for the row and `note` says why the
row is there."""
import collections

import torch
import torch.nn.functional as F

DwCase = collections.namedtuple("DwCase", "N C c_valid H W ksize stride edge note")

EPC = {"fp32": 4, "bf16": 8}          # elements per 16-byte chunk (DT<T>::EPC)
DWW_LANES = 32                        # tapped weight-gradient kernel: pixel lanes per block
KS = [(3, 1), (3, 2), (5, 1), (5, 2)]


def out_hw(H, W, k, s):
    return (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1


def dww_strips(opix):
    """dww_strips of ops.hip: strips of ~2048 output pixels for the tapped weight-gradient kernel"""
    return max(1, min(4096, (opix + 2047) // 2048))


def tapped_plan(c):
    """(strips, per_strip, output pixels) of dwconv3_wgrad's tapped launch"""
    OH, OW = out_hw(c.H, c.W, c.ksize, c.stride)
    opix = c.N * OH * OW
    strips = dww_strips(opix)
    return strips, (opix + strips - 1) // strips, opix


def dww_rows_plan(N, H, CPR):
    """dww_rows_plan of ops.hip (3x3 / stride 1 row-walking weight-gradient kernel): CW chunk columns per block, gy column blocks,
    `lanes` row lanes, rpl rows per lane, nb row blocks"""
    CW = CPR if CPR <= 32 else (32 if CPR % 32 == 0 else (24 if CPR % 24 == 0 else 32))
    gy = (CPR + CW - 1) // CW
    lanes = 256 // CW
    NR = N * H
    want = max(1, 512 // gy)
    rpl = max(1, (NR + want * lanes - 1) // (want * lanes))
    nb = (NR + lanes * rpl - 1) // (lanes * rpl)
    return dict(CW=CW, gy=gy, lanes=lanes, rpl=rpl, nb=nb, NR=NR)


def rows_kernel(c):
    return c.ksize == 3 and c.stride == 1


def _every_ks(N, C, cv, H, W, edge, note):
    return [DwCase(N, C, cv, H, W, k, s, edge, note) for k, s in KS]


DW_CASES = (
    # ---- every (ksize, stride) at the four basic sizes; N = 2 so that a read across an image boundary lands in real data
    _every_ks(2, 64, 64, 7, 10, "parities", "non-square, odd H / even W: both parity classes of a stride-2 data gradient, every border")
    + _every_ks(2, 64, 64, 8, 8, "even", "even x even, the maps of a 224 input: under stride 2 the bottom / right border has one tap fewer than the top / left")
    + _every_ks(2, 64, 64, 2, 3, "small", "image smaller than a 5x5 window (and than a 3x3 one in H): every tap row clipped somewhere")
    + _every_ks(2, 64, 64, 1, 1, "one", "1x1 image: only the centre tap is ever in range")
    # ---- channel widths: the chunk-column choices of the row-walking kernel, and the padded staging
    + _every_ks(2, 192, 192, 7, 10, "cw24", "C = 192: fp32 CPR = 48 -> CW = 24 (10 lanes, 16 idle threads), bf16 CPR = 24")
    + _every_ks(2, 320, 320, 7, 10, "ragged_cblock", "C = 320: fp32 CPR = 80 / bf16 CPR = 40, both CW = 32 with a ragged last channel block")
    + _every_ks(2, 192, 144, 7, 10, "padded", "c_valid = 144 of 192: zero-filled staged weights, dw rows beyond c_valid dropped; x / dy non-zero there")
    # ---- the classes of the real plans at 224 / 225 that the rows above miss (odd x odd and even x even, padded and not)
    + _every_ks(2, 64, 64, 5, 5, "odd", "odd x odd at the window size of 5x5: the 113 / 57 / 29 / 15 maps of a 225 input")
    + _every_ks(2, 192, 144, 5, 5, "padded", "padded channels on an odd x odd map")
    + _every_ks(2, 192, 144, 8, 8, "padded", "padded channels on an even x even map")
    + [
        # ---- tapped weight gradient: two ragged strips
        DwCase(3, 64, 64, 57, 57, 3, 2, "strips2", "29x29 outputs, 2523 pixels = strips of 1262 + 1261; 1262 % DWW_LANES != 0"),
        DwCase(3, 64, 64, 58, 58, 5, 2, "strips2", "the same through the five-tap rows of the 5x5 kernel"),
        # ---- row-walking weight gradient: two rows per lane and a partly empty last block
        DwCase(24, 192, 192, 111, 3, 3, 1, "rpl2_fp32", "fp32: NR = 2664 -> rpl = 2, nb = 134, the last block's second rows are past NR"),
        DwCase(47, 192, 192, 111, 2, 3, 1, "rpl2_bf16", "bf16: CPR = 24 -> 10 lanes, want = 512; NR = 5217 -> rpl = 2, nb = 261, ragged"),
    ]
)


def dw_id(c):
    return f"n{c.N}-c{c.C}v{c.c_valid}-{c.H}x{c.W}-k{c.ksize}s{c.stride}-{c.edge}"


def dw_class(k, s, H, W, padded):
    """what the plan-coverage check compares: (ksize, stride, H parity, W parity, H < ksize, padded or not)"""
    return (k, s, H % 2, W % 2, H < k, bool(padded))


def rb(t):
    """round to bf16-representable fp32"""
    return t.bfloat16().float()


_DW_CACHE = {}


def dw_reference(c):
    """bf16-representable x, w, dy (fp32, CPU) and the fp64 y, dx, dw of F.conv2d(groups = C) with zero weights on the padding channels;
    computed once per case and shared (callers must not modify the tensors)"""
    if c in _DW_CACHE:
        return _DW_CACHE[c]
    g = torch.Generator().manual_seed(1000 * c.ksize + 100 * c.stride + 7 * c.H + c.W + c.C + c.c_valid + c.N)
    x = rb(torch.randn(c.N, c.C, c.H, c.W, generator=g))                       # non-zero in the padding channels too
    w = rb(torch.randn(c.c_valid, 1, c.ksize, c.ksize, generator=g) * 0.3)
    OH, OW = out_hw(c.H, c.W, c.ksize, c.stride)
    dy = rb(torch.randn(c.N, c.C, OH, OW, generator=g))
    wfull = torch.zeros(c.C, 1, c.ksize, c.ksize, dtype=torch.float64)
    wfull[: c.c_valid] = w.double()
    xr, wr = x.double().requires_grad_(True), wfull.requires_grad_(True)
    y = F.conv2d(xr, wr, stride=c.stride, padding=c.ksize // 2, groups=c.C)
    assert y.shape == dy.shape
    y.backward(dy.double())
    out = dict(x=x, w=w, dy=dy, y=y.detach(), dx=xr.grad, dw=wr.grad[: c.c_valid].clone())
    _DW_CACHE[c] = out
    return out


# ---- BatchNorm + activation: (N, C, H, W); gamma = beta = 3 puts >= 10 % of a N(0,1) input in each of y <= 0, 0 < y < 6, y >= 6
BN_SHAPES = [(4, 64, 9, 7), (3, 192, 5, 5)]
BN_ACTS = {"relu6": 2, "silu": 3}

# ---- squeeze-excitation: (N, C, Csq, HW); HW = 33 is no multiple of the 32 pixel lanes, C = 96 / 144 are padded to 128 / 192
SE_SHAPES = [(2, 96, 4, 49), (3, 144, 6, 1), (2, 672, 28, 33)]


def pad64(c):
    return (c + 63) // 64 * 64


def se_reference(y, w1, b1, w2, b2, dyse):
    """torchvision SqueezeExcitation (avgpool -> fc1 -> SiLU -> fc2 -> sigmoid -> scale) in fp64 on y [N][C][HW]; returns y_se and the
    gradients of y, w1, b1, w2, b2"""
    y, w1, b1, w2, b2 = (t.double().requires_grad_(True) for t in (y, w1, b1, w2, b2))
    s = y.mean(2)
    a1 = F.silu(s @ w1.T + b1)
    gate = torch.sigmoid(a1 @ w2.T + b2)
    yse = y * gate[:, :, None]
    yse.backward(dyse.double())
    return yse.detach(), y.grad, w1.grad, b1.grad, w2.grad, b2.grad
