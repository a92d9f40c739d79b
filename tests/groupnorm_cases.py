"""Cases, inputs and the plain-torch reference of the GroupNorm(8, C) + ReLU (+ MaxPool2d(2, 2)) op (csrc/groupnorm.hip), shared by
tests/test_cpu_groupnorm_cases.py (no GPU: the properties the inputs must have) and tests/test_gpu_groupnorm_ops.py.

Shapes: N = 3 with H x W in {6x10, 7x9, 32x32} (7x9: the row and column MaxPool2d's floor drops) and C in {64, 128, 256} (a group is 1, 2 or
4 sixteen-byte bf16 vectors per pixel); one larger map, N = 2 at 112x112x64, whose statistics span 13 workgroups.

Inputs are bf16-representable.  A pre-activation within rounding distance of zero, or two window taps that close to each other, would let
fp32 rounding flip a ReLU mask bit or an argmax -- a whole gradient element moves, and through the group sums every element of its group --
so `conditioned` moves such an input one bf16 step up until every |pre-activation| and every deciding tap gap is at least MARGIN (1e-4, a
hundred fp32 roundings of an O(1) value) in fp64.  The element-wise comparisons of the bf16 runs still exclude what lies within
BF16_MARGIN = 2^-6, and at most EXCLUDED_CAP of the elements may be excluded."""
import functools

import torch
import torch.nn.functional as F

EPS = 1e-5
GROUPS = 8
MARGIN = 1e-4
BF16_MARGIN = 2.0 ** -6
EXCLUDED_CAP = 0.03
SMALL_SHAPES = [(3, C, H, W) for (H, W) in ((6, 10), (7, 9), (32, 32)) for C in (64, 128, 256)]
LARGE_SHAPE = (2, 64, 112, 112)
CONDITIONING_SHAPE = (3, 128, 7, 9)   # every group: mean 50, std 1


def rb(t):
    return t.bfloat16().float()


def case_id(s):
    return "x".join(map(str, s))


def pre_activation(y, gamma, beta):
    return F.group_norm(y, GROUPS, gamma, beta, EPS)


def window_taps(z):
    """[N, C, PH, PW, 4]: the taps of every 2x2 window, row-major (floor: an odd last row / column is in no window)"""
    N, C, H, W = z.shape
    PH, PW = H // 2, W // 2
    zc = z[:, :, :2 * PH, :2 * PW].reshape(N, C, PH, 2, PW, 2)
    return zc.permute(0, 1, 2, 4, 3, 5).reshape(N, C, PH, PW, 4)


def deciding_gap(z):
    """Distance between the largest and the second largest tap of every window whose maximum is positive (inf elsewhere: an all-zero window
    is decided by the tie-break, not by arithmetic)"""
    top = window_taps(z).topk(2, dim=-1).values
    gap = top[..., 0] - top[..., 1]
    return torch.where(top[..., 0] > 0, gap, torch.full_like(gap, float("inf")))


def bf16_step_up(y):
    """the next bf16 value above y (y bf16-representable)"""
    bits = y.bfloat16().view(torch.int16).to(torch.int32)
    up = torch.where(y > 0, bits + 1, torch.where(y < 0, bits - 1, torch.full_like(bits, 0x0080)))
    return up.to(torch.int16).view(torch.bfloat16).float()


def conditioned(y, gamma, beta, pool, margin=MARGIN):
    assert bool((gamma > 0).all()), "the nudge assumes a positive scale"
    y = y.clone()
    for _ in range(20):
        pre = pre_activation(y.double(), gamma.double(), beta.double())
        bad = pre.abs() < margin
        if pool:
            z = pre.clamp_min(0)
            taps = window_taps(z)
            first = F.one_hot(taps.argmax(dim=-1), 4).bool()
            close = (deciding_gap(z) < margin).unsqueeze(-1) & first   # raise one maximum (two taps may hold the same bf16 value)
            N, C, H, W = y.shape
            PH, PW = H // 2, W // 2
            full = torch.zeros_like(bad)
            full[:, :, :2 * PH, :2 * PW] = close.reshape(N, C, PH, PW, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * PH, 2 * PW)
            bad |= full
        if not bool(bad.any()):
            return y
        up = rb(y + 2.0 ** -6)   # a step that moves the pre-activation by ~100 margins; where bf16 is coarser than that, one bf16 step
        y = torch.where(bad, torch.where(up > y, up, bf16_step_up(y)), y)
    raise AssertionError("inputs did not reach the margin")


@functools.lru_cache(maxsize=None)
def inputs(shape, pool, conditioning=False):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(1000 * C + 10 * H + W + (5 if conditioning else 0))
    y = torch.randn(N, C, H, W, generator=g)
    if conditioning:
        y = y + 50.0
    gamma = rb(1 + 0.2 * torch.randn(C, generator=g))
    beta = rb(0.2 * torch.randn(C, generator=g))
    y = conditioned(rb(y), gamma, beta, pool)
    oh, ow = (H // 2, W // 2) if pool else (H, W)
    gout = rb(torch.randn(N, C, oh, ow, generator=g))
    return y, gamma, beta, gout


def reference(y, gamma, beta, gout, pool, dtype, store=None):
    """plain torch in `dtype`; store (bf16 emulation): the rounding applied once to each tensor the op stores in its element type"""
    store = store or (lambda t: t)
    yv, gv, bv = (t.clone().to(dtype).requires_grad_(True) for t in (y, gamma, beta))   # clone: .to() of the same dtype is the tensor itself
    pre = pre_activation(yv, gv, bv)
    z = F.relu(pre)
    out, tap = z, None
    if pool:
        out, flat = F.max_pool2d(z, 2, return_indices=True)
        W = y.shape[3]
        tap = ((flat // W) % 2) * 2 + (flat % W) % 2
    out.backward(gout.to(dtype))
    grp = yv.detach().reshape(y.shape[0], GROUPS, -1)
    mean, var = grp.mean(-1), grp.var(-1, unbiased=False)
    return dict(mean=mean, rstd=(var + EPS).rsqrt(), out=store(out.detach()), dy=store(yv.grad), dgamma=gv.grad, dbeta=bv.grad,
                pre=pre.detach(), tap=tap)


@functools.lru_cache(maxsize=None)
def references(shape, pool, conditioning=False):
    """fp64, CPU fp32 and the bf16 emulation (fp32 arithmetic, stored tensors rounded once) of one case, computed once"""
    y, gamma, beta, gout = inputs(shape, pool, conditioning)
    return (reference(y, gamma, beta, gout, pool, torch.float64), reference(y, gamma, beta, gout, pool, torch.float32),
            reference(y, gamma, beta, gout, pool, torch.float32, store=rb))


def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm()) / (float(want.norm()) + 1e-30)


def excluded(ref64, pool, margin=BF16_MARGIN):
    """(mask of input elements, mask of pooled elements or None) the element-wise bf16 comparisons leave out"""
    near_zero = ref64["pre"].abs() < margin
    near_tie = (deciding_gap(ref64["pre"].clamp_min(0)) < margin) if pool else None
    return near_zero, near_tie
