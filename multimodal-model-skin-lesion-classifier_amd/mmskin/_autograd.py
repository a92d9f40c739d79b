"""Autograd glue shared by every HIP op: the backward kernels are not themselves differentiable, so a SECOND
differentiation through an op must fail loudly instead of treating the first-order gradient as a constant (which is what
torch does, silently, for a custom Function whose backward is opaque).  The reference never needs it -- its Grad-CAM++
(src/services/XAI/models/cam.py:38-43) calls autograd.grad(..., create_graph=True) and then only squares / cubes the
first-order gradients -- so first-order results under create_graph=True stay exact and free.

Below that: what ops.py and attention.py both need and neither owns -- the tensor checks every Function opens with, the Linear operand
mode and the dropout counter."""
import contextlib
import functools

import torch

from . import _lib
from ._lib import MMSkinError


class _NoSecondOrder(torch.autograd.Function):
    """Identity on `grad`, tied to the op's differentiable inputs; differentiating through it raises."""

    @staticmethod
    def forward(ctx, name, grad, *anchors):
        ctx.op_name = name
        return grad.view_as(grad)

    @staticmethod
    def backward(ctx, g):
        raise MMSkinError(
            f"second-order differentiation through the HIP op {ctx.op_name} is not supported: its backward runs opaque "
            "gfx950 kernels.  First-order gradients, also under autograd.grad(..., create_graph=True), are exact.")


def no_second_order(cls):
    """Class decorator for torch.autograd.Function subclasses whose backward launches HIP kernels."""
    fwd, bwd = cls.forward, cls.backward

    @functools.wraps(fwd)
    def forward(ctx, *args):
        ctx._mmskin_anchors = tuple(a for a in args if isinstance(a, torch.Tensor) and a.requires_grad)
        return fwd(ctx, *args)

    @functools.wraps(bwd)
    def backward(ctx, *grads):
        with torch.no_grad():
            outs = bwd(ctx, *[g.detach() if isinstance(g, torch.Tensor) else g for g in grads])
        anchors = ctx._mmskin_anchors + tuple(g for g in grads if isinstance(g, torch.Tensor) and g.requires_grad)
        if not torch.is_grad_enabled() or not anchors:
            return outs
        single = not isinstance(outs, tuple)
        seq = (outs,) if single else outs
        seq = tuple(_NoSecondOrder.apply(cls.__name__, o, *anchors) if isinstance(o, torch.Tensor) else o for o in seq)
        return seq[0] if single else seq

    cls.forward = staticmethod(forward)
    cls.backward = staticmethod(backward)
    return cls


def _need_gpu(t, what):
    if not t.is_cuda:
        raise _lib.MMSkinError(
            f"mmskin.{what}: tensors must live on a HIP device (got {t.device}); the MI355X path has "
            "no CPU fallback")


def _f32c(t):
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def _dtype_code(t):
    """the C ABI's dtype code of a tensor or of a torch dtype (bf16, or fp32 for everything else)"""
    return _lib.BF16 if getattr(t, "dtype", t) == torch.bfloat16 else _lib.F32


def get_linear_dtype():
    return "bf16" if _lib.load().mmskin_get_linear_dtype() == 1 else "fp32"


_dropout_counter = [0]
_dropout_streams = []                  # [seed, counter] of every open dropout_stream, the innermost last


@contextlib.contextmanager
def dropout_stream(seed):
    """Inside the block every dropout of the library draws from a stream of its own: _dropout_state hands out `seed` and offsets
    from a private counter that starts at 0, so equal seeds and an equal sequence of calls repeat the masks bit for bit.  The
    global counter and torch's seed are neither read nor moved; the stream ends with the block, also after an exception."""
    state = [int(seed) & 0xFFFFFFFFFFFFFFFF, 0]
    _dropout_streams.append(state)
    try:
        yield state
    finally:
        _dropout_streams.remove(state)


def _dropout_state(p, n):
    if p <= 0.0:
        return 0, 0
    if _dropout_streams:               # callers import this function by name: the override lives here
        state = _dropout_streams[-1]
        off = state[1]
        state[1] += n
        return state[0], off
    off = _dropout_counter[0]          # this call consumes counters [off, off + n): ranges of successive calls never overlap
    _dropout_counter[0] += n
    return torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, off
