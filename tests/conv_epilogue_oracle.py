"""fp64 statement of the fused epilogues of csrc/conv_gemm.hip (the `EPI` profiles 1, 2, 4, 5, 7 and the statistics of profile 0), in torch:
F.conv2d, its autograd and elementwise arithmetic, no kernel code.  tests/test_cpu_conv_epilogues.py checks it against autograd through a
residual block without a device; tests/test_gpu_conv_epilogues.py compares mmskin_conv2d_dgrad_epilogue / mmskin_conv2d_forward_epilogue
with it.

Order of operations, read from the kernel (the epilogue after the K loop):

  acc (fp32 accumulator) -> `staged`: written to the LDS tile as the element type T, so ROUNDED TO T when T is bf16 (fp32: unchanged)
  data gradient : v = staged + addend; v = 0 where the mask says so (mask_y > 0 | mask bits | x * scale + shift > 0); store(v);
                  sums over the STORED (rounded) v: sum v, sum v * x, sum v * x2
  forward       : v = staged * mul; v += addend; v += bias; ReLU; store(v); mask bit = (stored v > 0);
                  statistics of profile 0: sum and sum of squares of `staged` (which is what a plain store writes)

The rounding of the accumulator before the epilogue arithmetic is part of that order: with an addend a bf16 element carries two roundings,
one of the convolution's value and one of the sum, exactly as the unfused sequence conv -> add would.  Where the exact accumulator lies
within the fp32 accumulator's error (`acc_floor`: 1e-5 of the rms) of a bf16 rounding boundary, the first rounding may go either way
(near zero, where a bf16 ulp is smaller than that error, over several values); `staged_pair` returns the roundings of both ends of the
error interval and `within_bound` accepts an element within the bound of the interval between the two references -- everywhere else,
on at least 97 % of the elements (MAX_OPEN_ROUNDINGS, asserted), they are one value.
"""
import torch
import torch.nn.functional as F

ELEM_BYTES = {"fp32": 4, "bf16": 2}


def rb(t):
    """round to bf16 (nearest even), same dtype back"""
    return t.float().bfloat16().to(t.dtype)


def stored(v, dtype):
    """the value as an element of type `dtype` holds it, in fp64"""
    return (rb(v.float()) if dtype == "bf16" else v.float()).double()


def conv_fwd(x, w, shape):
    N, Cin, H, W, Cout, k, s, p = shape
    if k == 1 and s == 1 and p == 0:                     # the same sum as a matrix product (also on a device without an fp64 convolution)
        return torch.einsum("nchw,oc->nohw", x, w[:, :, 0, 0])
    return F.conv2d(x, w, stride=s, padding=p)


def conv_dgrad(dy, w, shape):
    """gradient of conv2d with respect to its input, by autograd"""
    N, Cin, H, W, Cout, k, s, p = shape
    if k == 1 and s == 1 and p == 0:
        return torch.einsum("nohw,oc->nchw", dy, w[:, :, 0, 0])
    x = torch.zeros(N, Cin, H, W, dtype=dy.dtype, device=dy.device, requires_grad=True)
    F.conv2d(x, w, stride=s, padding=p).backward(dy)
    return x.grad


def acc_error(absacc, terms):
    """bound of the fp32 accumulator's own error: `terms` products summed in any order, |error| <= terms * 2^-24 * sum |a||b| (absacc)"""
    return terms * 2.0 ** -24 * absacc


def acc_floor(acc, absacc=None):
    """the fp32 accumulator's error as the project's parity tests already allow it: 1e-5 of the rms (the summation floor in the bound of
    test_conv_bf16_tight_on_representable_inputs, which holds there up to K = 4608) -- two to three orders below the worst case above.
    absacc (sum |a||b|): where it is 0 no product is nonzero (a pixel of a strided data gradient that no tap reaches) and the sum is exact"""
    err = torch.full_like(acc, 1e-5 * float(acc.pow(2).mean().sqrt()))
    return err if absacc is None else torch.where(absacc == 0, torch.zeros_like(err), err)


# Share of elements whose first rounding the floor can leave open, at most: an element a is within err of a bf16 boundary with probability
# <= 2 err / spacing <= 2 * 1e-5 rms * 2^8 / |a|; over a normal distribution E[min(1, 5.1e-3 / |z|)] < 0.03.  More than that means the
# interval is doing the bound's work.
MAX_OPEN_ROUNDINGS = 0.03


def staged_pair(acc, err, dtype):
    """the accumulator as the epilogue reads it: (lo, hi), equal except where acc is within err of a bf16 rounding boundary"""
    if dtype == "bf16":
        return stored(acc - err, dtype), stored(acc + err, dtype)
    return acc, acc


def dgrad_epilogue(a, addend=None, addend_s2=False, mask_y=None, keep_bits=None, x=None, scale=None, shift=None):
    """a: staged data gradient [N,C,H,W] (fp64).  Returns v before the store.  keep_bits: bool [N,C,H,W]."""
    v = a.clone()
    if addend is not None:
        if addend_s2:
            v[:, :, ::2, ::2] += addend
        else:
            v = v + addend
    keep = torch.ones_like(v, dtype=torch.bool)
    if mask_y is not None:
        keep &= mask_y > 0
    if keep_bits is not None:
        keep &= keep_bits
    if scale is not None:
        keep &= (x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)) > 0
    return torch.where(keep, v, torch.zeros_like(v))


def fwd_epilogue(a, mul=None, addend=None, bias=None, relu=False):
    v = a
    if mul is not None:
        v = v * mul.view(1, -1, 1, 1)
    if addend is not None:
        v = v + addend
    if bias is not None:
        v = v + bias.view(1, -1, 1, 1)
    return torch.relu(v) if relu else v


def element_bound(want, dtype):
    """bf16: half an ulp of the exact value (2^-8 relative) plus the summation noise floor, the bound of
    test_conv_bf16_tight_on_representable_inputs; fp32: TOL["fp32"] of tests/test_gpu_kernels.py (2e-4 of the rms)"""
    rms = float(want.pow(2).mean().sqrt())
    if dtype == "bf16":
        return want.abs() * 2.0 ** -8 + 1e-5 * rms
    return torch.full_like(want, 2e-4 * rms)


def within_bound(got, want_pair, dtype):
    """bool tensor: got within element_bound of the interval the two references span (the epilogue is monotone in the staged value, so
    every accumulator inside its error interval gives a value between them; where they coincide this is the plain bound)"""
    lo, hi = torch.minimum(*want_pair), torch.maximum(*want_pair)
    return (got >= lo - element_bound(lo, dtype)) & (got <= hi + element_bound(hi, dtype))


def nhwc_rows(t):
    """[N,C,H,W] -> [N*H*W][C]: the layout the kernels store"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def pack_bits(keep, dtype):
    """bool [N,C,H,W] -> mask bytes in the kernel's layout: one byte per 16-byte chunk of the NHWC `dtype` tensor, byte index
    (row * C + col) * elem_bytes >> 4, bit e = element e of the chunk (8 elements per byte in bf16, 4 in fp32)"""
    epc = 16 // ELEM_BYTES[dtype]
    flat = nhwc_rows(keep).reshape(-1, epc).to(torch.int32)
    weights = (2 ** torch.arange(epc, dtype=torch.int32, device=keep.device)).view(1, -1)
    return (flat * weights).sum(1).to(torch.uint8)


def unpack_bits(packed, shape_nchw, dtype):
    """mask bytes -> bool [N,C,H,W]"""
    N, C, H, W = shape_nchw
    epc = 16 // ELEM_BYTES[dtype]
    shifts = torch.arange(epc, dtype=torch.int32, device=packed.device).view(1, -1)
    bits = ((packed.to(torch.int32).view(-1, 1) >> shifts) & 1).bool()
    return bits.reshape(N, H, W, C).permute(0, 3, 1, 2)


def mask_bytes(rows, C, dtype):
    return rows * C * ELEM_BYTES[dtype] // 16
