"""autograd.Function wrappers over the C ABI (fp32 head operators + custom-cnn pieces).

Each Function allocates its outputs with torch (device memory plumbing), launches
the HIP kernels on torch's current stream through ctypes and keeps what the
matching backward entry point needs.  No arithmetic happens in PyTorch here.
"""
import ctypes
import weakref

import numpy as np
import torch

from . import _lib
from ._autograd import (_dropout_counter, _dropout_state, _dtype_code, _f32c, _need_gpu, _needs_grad, get_linear_dtype,  # noqa: F401
                        no_second_order)
from ._lib import call, ptr, stream
from .attention import (LongAttentionFn, _bmm, attention, attention_blhd, attention_packed, attention_route,  # noqa: F401
                        channel_attention, channel_attention_ok, swin_window_attention, swin_window_attention_ok, window_attention,
                        window_attention_ok)


# ---------------------------------------------------------------------------------------------- the Linear family (csrc/linear.hip)
# Everything that drives csrc/linear.hip, in dependency order: the operand mode, LinearFn and its row-block sibling, the inference
# lane, linear(), the activations of the transformer MLPs, LinearGeluFn, and the fused MLP.  The route of a shape is linear.hip's
# decision (linear_path); the wrappers ask it (mmskin_linear_x16_pitch) instead of re-deriving it.
def set_linear_dtype(name):
    """'fp32' (exact-f32 MFMA, default) or 'bf16' (bf16 operands, fp32 accumulate) for the large Linear GEMMs."""
    call("mmskin_set_linear_dtype", {"fp32": _lib.F32, "float32": _lib.F32, "bf16": _lib.BF16, "bfloat16": _lib.BF16}[name.lower()])


def _linear_forward(x, w, b, res, act, want_keep):
    """The forward LinearFn and LinearGeluFn share: y = [res +] act(x @ w.T + b) over the rows of x.  want_keep: ask the library for the
    pitch of the bf16 operand copy of x -- non-zero on the bf16-operand large-GEMM path only -- and have the GEMM that consumes that copy
    leave it behind (the fused residual exists on that path alone).  Returns (xs, w, y, kept): xs is the kept bf16 copy when `kept`,
    the fp32 rows of x otherwise -- what a weight gradient needs."""
    x2 = _f32c(x).reshape(-1, x.shape[-1])
    w = _f32c(w)
    M, K = x2.shape
    N = w.shape[0]
    y = torch.empty((M, N), device=x.device, dtype=torch.float32)
    pitch = _lib.load().mmskin_linear_x16_pitch(M, K, N) if want_keep else 0
    if res is not None and (not pitch or act):
        raise RuntimeError("linear: the fused residual needs the bf16-operand large-GEMM path and no ReLU")
    if not pitch:
        call("mmskin_linear_forward", ptr(x2), ptr(w), ptr(b), ptr(y), M, K, N, int(act), stream())
        return x2, w, y, False
    x16 = torch.empty((M, pitch), device=x.device, dtype=torch.bfloat16)
    r2 = _f32c(res).reshape(M, N) if res is not None else None
    call("mmskin_linear_forward_keep", ptr(x2), ptr(w), ptr(b), ptr(r2), ptr(y), ptr(x16), M, K, N, int(act), stream())
    return x16, w, y, True


@no_second_order
class LinearFn(torch.autograd.Function):
    """y = [res +] x @ w.T + b, optional fused ReLU (nn.Linear [+ nn.ReLU] [+ the block's residual add]).  When the bf16-operand
    large-GEMM path runs and w trains, the bf16 copy of x the forward GEMM consumed is what is saved for the weight gradient (half the
    bytes, no second conversion); the residual is added in the pass that writes y (only offered on that path: see linear())."""

    @staticmethod
    def forward(ctx, x, w, b, relu, res=None):
        _need_gpu(x, "linear")
        need_w = ctx.needs_input_grad[1]
        xs, w, y, kept = _linear_forward(x, w, b, res, relu, need_w or res is not None)
        ctx.save_for_backward(xs if need_w else None, w, y if relu else None)
        ctx.kept = kept and need_w
        ctx.mk = (y.shape[0], x.shape[-1])
        ctx.has_bias = b is not None
        ctx.xshape = x.shape
        ctx.res_shape = None if res is None else res.shape
        return y.reshape(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        xs, w, y = ctx.saved_tensors
        M, K = ctx.mk
        N = w.shape[0]
        dy2 = _f32c(dy).reshape(M, N)
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dx = torch.empty((M, K), device=dy.device, dtype=torch.float32) if need_x else None
        dw = torch.empty_like(w) if need_w else None
        db = torch.empty(N, device=dy.device, dtype=torch.float32) if need_b else None
        scratch = torch.empty_like(dy2) if y is not None else None
        if ctx.kept:
            call("mmskin_linear_backward_keep", ptr(dy2), ptr(xs), ptr(w), ptr(y), None, ptr(scratch), ptr(dx), ptr(dw), ptr(db),
                 M, K, N, stream())
        else:
            call("mmskin_linear_backward", ptr(dy2), ptr(xs), ptr(w), ptr(y), ptr(scratch), ptr(dx), ptr(dw), ptr(db),
                 M, K, N, stream())
        dres = dy2.reshape(ctx.res_shape) if ctx.res_shape is not None and ctx.needs_input_grad[4] else None   # relu is never combined with res
        return (dx.reshape(ctx.xshape) if need_x else None), dw, db, None, dres


class LinearRowsFn(torch.autograd.Function):
    """y = x @ w[r0:r1].T + b[r0:r1] for a ROW BLOCK of a stacked parameter (the value projection of nn.MultiheadAttention's
    in_proj_weight / in_proj_bias when a single key makes the q / k projections dead, multimodalIntraInterModal.py:190-197).  The
    backward hands autograd the gradients of the WHOLE parameters: one zero fill for both, the row block written in place by the
    Linear-backward launch -- autograd's own slice backward costs two fills and two copies per call (16 launches per head step)."""

    @staticmethod
    def forward(ctx, x, w, b, r0, r1):
        _need_gpu(x, "linear_rows")
        x2 = _f32c(x).reshape(-1, x.shape[-1])
        w = _f32c(w)
        b = _f32c(b) if b is not None else None
        M, K = x2.shape
        N = r1 - r0
        y = torch.empty((M, N), device=x.device, dtype=torch.float32)
        call("mmskin_linear_forward", ptr(x2), w.data_ptr() + 4 * r0 * K, (b.data_ptr() + 4 * r0) if b is not None else None, ptr(y),
             M, K, N, 0, stream())
        ctx.save_for_backward(x2 if ctx.needs_input_grad[1] else None, w)
        ctx.rows, ctx.mk, ctx.xshape = (r0, r1), (M, K), x.shape
        ctx.bias = None if b is None else (b.shape, b.dtype)
        return y.reshape(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        xs, w = ctx.saved_tensors
        (r0, r1), (M, K) = ctx.rows, ctx.mk
        N = r1 - r0
        dy2 = _f32c(dy).reshape(M, N)
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        need_b = ctx.bias is not None and ctx.needs_input_grad[2]
        dx = torch.empty((M, K), device=dy.device, dtype=torch.float32) if need_x else None
        nw, nb = (w.numel() if need_w else 0), (ctx.bias[0].numel() if need_b else 0)
        flat = torch.zeros(nw + nb, device=dy.device, dtype=torch.float32) if nw + nb else None
        dw = flat[:nw].view_as(w) if need_w else None
        db = flat[nw:].view(ctx.bias[0]) if need_b else None
        call("mmskin_linear_backward", ptr(dy2), ptr(xs), w.data_ptr() + 4 * r0 * K, None, None, ptr(dx),
             (dw.data_ptr() + 4 * r0 * K) if need_w else None, (db.data_ptr() + 4 * r0) if need_b else None, M, K, N, stream())
        return (dx.reshape(ctx.xshape) if need_x else None), dw, db, None, None


def linear_rows(x, w, b, r0, r1):
    """nn.functional.linear(x, w[r0:r1], b[r0:r1]) with the gradients of w / b produced whole (exact zeros outside the row block)."""
    if x.dtype != torch.float32 or not x.is_cuda:
        return linear(x, w[r0:r1], b[r0:r1] if b is not None else None)
    return LinearRowsFn.apply(x, w, b, r0, r1)


def _rows_f32_or_bf16(x):
    """x as contiguous rows [M, K] in a dtype the lane entry points read: bf16 and fp32 as they are, anything else widened to fp32"""
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    return x2 if x2.dtype in (torch.float32, torch.bfloat16) else x2.float()


def lane_dtype(x, module=None, *tensors):
    """torch.bfloat16 when the INFERENCE LANE applies to a layer -- bf16-operand mode and no gradient flows through it (input,
    the module's parameters and `tensors` all without grad, or grad mode off): activations are then handed between the layer's
    Linear / LayerNorm / attention ops as bf16 tensors, without fp32 <-> bf16 conversion passes.  None otherwise: the layer runs
    its ordinary (differentiable, fp32-boundary) ops."""
    if not x.is_cuda or get_linear_dtype() != "bf16":
        return None
    params = tuple(module.parameters()) if module is not None else ()
    return None if _needs_grad(x, *params, *tensors) else torch.bfloat16


def _linear_ex(x, w, b, act, out_dtype):
    """no-grad Linear with bf16 and / or fp32 tensors at the boundary (mmskin_linear_forward_ex)."""
    _need_gpu(x, "linear")
    if _needs_grad(x, w, b):
        raise _lib.MMSkinError("mmskin.linear: bf16 activations are an inference-lane feature (no gradient may flow through them)")
    x2 = _rows_f32_or_bf16(x)
    w = _f32c(w)
    M, K = x2.shape
    N = w.shape[0]
    od = out_dtype or torch.float32
    y = torch.empty((M, N), device=x.device, dtype=od)
    call("mmskin_linear_forward_ex", ptr(x2), _dtype_code(x2), ptr(w), ptr(b), ptr(y), _dtype_code(od), M, K, N, int(act), stream())
    return y.reshape(*x.shape[:-1], N)


_frozen_cache = {}   # (data_ptr, ...) -> (versions, weakrefs, bf16 tensor)


def frozen_bf16(*ws):
    """bf16 copy of one weight (or of several stacked along dim 0: the q / k / v projections of a BERT layer as ONE [3E, E] operand)
    that no gradient flows into, converted once and reused until a source tensor changes (its version counter moves: optimizer
    step, load_state_dict, .copy_) or is replaced.  Saves the per-step fp32 -> bf16 pass over every frozen encoder weight."""
    key = tuple(w.data_ptr() for w in ws)
    vers = tuple(w._version for w in ws)
    hit = _frozen_cache.get(key)
    if hit is not None and hit[0] == vers and all(r() is w for r, w in zip(hit[1], ws)):
        return hit[2]
    with torch.no_grad():
        w16 = (ws[0] if len(ws) == 1 else torch.cat([w.reshape(w.shape[0], -1) for w in ws], 0)).to(torch.bfloat16).contiguous()
    if len(_frozen_cache) > 4096:
        _frozen_cache.clear()
    drop = lambda _ref, key=key: _frozen_cache.pop(key, None)       # a source tensor died (model deleted / moved): free its bf16 copy too
    _frozen_cache[key] = (vers, tuple(weakref.ref(w, drop) for w in ws), w16)
    return w16


def invalidate_frozen_cache():
    """Drop every cached bf16 weight copy.  Anything that rewrites parameters through `.data` (which does not move the version
    counter) must call this; in-place ops on the parameter or a detach() view are seen by the version check on their own."""
    _frozen_cache.clear()


def lane_ok(x, N, K, fused_tail=False):
    """does mmskin_linear_lane take this shape?  (rows >= 2048, 64-multiple widths; 128-multiple N with a fused residual tail)"""
    M = x.numel() // x.shape[-1]
    return x.is_cuda and get_linear_dtype() == "bf16" and M >= 2048 and K % 64 == 0 and N % (128 if fused_tail else 64) == 0


def linear_lane(x, ws, b=None, act=0, gamma=None, residual=None, drop_p=0.0, training=False, out_dtype=None):
    """y = residual + gamma * dropout(act(x @ W.T + b)) as ONE GEMM launch on the inference lane (no gradient flows: frozen
    encoders / evaluation; bf16-operand mode).  ws: a weight or a tuple of weights stacked along the output dimension; their
    bf16 copy is cached (frozen_bf16).  act 0 none / 1 ReLU / 2 exact GELU.  With residual / gamma / dropout the result is the
    fp32 residual stream; otherwise out_dtype (fp32 default).  Shapes the fused kernel does not take are composed from the
    separate ops (same arithmetic, more launches)."""
    ws = ws if isinstance(ws, (tuple, list)) else (ws,)
    _need_gpu(x, "linear_lane")
    if _needs_grad(x, *ws, b, gamma, residual):
        raise _lib.MMSkinError("mmskin.linear_lane: an inference-lane op (no gradient may flow through it)")
    p = float(drop_p) if training else 0.0
    tail = gamma is not None or residual is not None or p > 0.0
    K = x.shape[-1]
    N = sum(w.shape[0] for w in ws)
    if not lane_ok(x, N, K, tail):
        w = ws[0] if len(ws) == 1 else torch.cat(list(ws), 0)
        h = _linear_ex(x, w, b, act, None if tail else out_dtype)
        if p > 0.0:
            h = dropout(h, p, True)
        if gamma is not None:
            return scale_add(residual if residual is not None else torch.zeros_like(h), h, gamma)
        return add(h, residual) if residual is not None else h
    x2 = _rows_f32_or_bf16(x)
    M = x2.shape[0]
    od = torch.float32 if tail else (out_dtype or torch.float32)
    y = torch.empty((M, N), device=x.device, dtype=od)
    res = None if residual is None else _f32c(residual).reshape(M, N)
    seed, offset = _dropout_state(p, M * N)
    call("mmskin_linear_lane", ptr(x2), _dtype_code(x2), ptr(frozen_bf16(*ws)), _lib.BF16,
         ptr(None if b is None else _f32c(b)), ptr(None if gamma is None else _f32c(gamma)), ptr(res), p, int(seed), int(offset),
         ptr(y), _dtype_code(od), M, K, N, int(act), stream())
    return y.reshape(*x.shape[:-1], N)


def linear(x, w, b=None, relu=False, out_dtype=None, residual=None):
    """nn.Linear (+ ReLU).  residual: y = residual + x @ w.T + b -- added in the pass that writes y when the bf16-operand large-GEMM
    path takes the shape (a transformer block's skip connection), by ops.add otherwise."""
    if w.numel() != w.shape[0] * x.shape[-1]:      # the kernels take K from x alone: a wrong width would read past w
        raise _lib.MMSkinError(f"linear: input of width {x.shape[-1]} for a weight of shape {tuple(w.shape)}")
    if x.dtype == torch.bfloat16 or out_dtype == torch.bfloat16:
        y = linear_lane(x, w, b, 1 if relu else 0, out_dtype=out_dtype)
        return y if residual is None else add(y, residual.reshape(y.shape))
    if residual is not None:
        M = x.numel() // x.shape[-1]
        if (not relu and x.is_cuda and x.dtype == torch.float32 and residual.dtype == torch.float32
                and _lib.load().mmskin_linear_x16_pitch(M, x.shape[-1], w.shape[0])):
            return LinearFn.apply(x, w, b, False, residual)
        y = LinearFn.apply(x, w, b, relu)
        return add(y, residual.reshape(y.shape))
    return LinearFn.apply(x, w, b, relu)


def _gelu_fn(cls_name, what):
    """The autograd Function of a GELU flavour, what = 'gelu' (exact) / 'gelu_tanh': its two entry points are mmskin_<what>_forward
    (x, y, n) and mmskin_<what>_backward (dy, x, dx, n)."""
    fwd, bwd = f"mmskin_{what}_forward", f"mmskin_{what}_backward"

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            _need_gpu(x, what)
            x = _f32c(x)
            y = torch.empty_like(x)
            call(fwd, ptr(x), ptr(y), x.numel(), stream())
            ctx.save_for_backward(x)
            return y

        @staticmethod
        def backward(ctx, dy):
            (x,) = ctx.saved_tensors
            dy = _f32c(dy)
            dx = torch.empty_like(x)
            call(bwd, ptr(dy), ptr(x), ptr(dx), x.numel(), stream())
            return dx

    Fn.__name__ = Fn.__qualname__ = cls_name
    return no_second_order(Fn)


GeluFn, GeluTanhFn = _gelu_fn("GeluFn", "gelu"), _gelu_fn("GeluTanhFn", "gelu_tanh")
gelu, gelu_tanh = GeluFn.apply, GeluTanhFn.apply


def _split_dsb(dsb, s, b, need_s, need_b):
    """The (d scale, d bias) pair a StarReLU backward pass wrote, as gradients shaped like the two one-element parameters; None where
    none is needed."""
    return (dsb[0:1].reshape(s.shape) if need_s else None), (dsb[1:2].reshape(b.shape) if need_b else None)


@no_second_order
class StarReluFn(torch.autograd.Function):
    """timm StarReLU: s * relu(z)^2 + b, s and b one-element tensors; the backward returns their gradients from the pass that writes dz
    (fixed-order reductions)."""

    @staticmethod
    def forward(ctx, z, s, b):
        _need_gpu(z, "star_relu")
        z, s, b = _f32c(z), _f32c(s), _f32c(b)
        y = torch.empty_like(z)
        call("mmskin_star_relu_forward", ptr(z), ptr(s), ptr(b), ptr(y), z.numel(), stream())
        ctx.save_for_backward(z, s)
        return y

    @staticmethod
    def backward(ctx, dy):
        z, s = ctx.saved_tensors
        dy = _f32c(dy)
        dz = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        dsb = torch.empty(2, device=dy.device, dtype=torch.float32)
        call("mmskin_star_relu_backward", ptr(dy), ptr(z), ptr(s), ptr(dz), ptr(dsb), z.numel(), stream())
        return (dz,) + _split_dsb(dsb, s, s, True, True)


star_relu = StarReluFn.apply


@no_second_order
class LinearGeluFn(torch.autograd.Function):
    """h = gelu(x @ w.T + b) with gradients (first half of a transformer MLP).  Forward: Linear, then GELU (the pre-activation z is kept
    for the backward); backward: ONE C call -- gelu'(z) is applied inside the pass that converts dh for the bf16 GEMMs and sums it for
    db (mmskin_linear_gelu_backward), so d(z) is never written in fp32.  The bf16 operand copy of x is kept as in LinearFn."""

    @staticmethod
    def forward(ctx, x, w, b):
        _need_gpu(x, "linear_gelu")
        need_w = ctx.needs_input_grad[1]
        xs, w, z, ctx.kept = _linear_forward(x, w, b, None, 0, need_w)
        ctx.save_for_backward(xs if need_w else None, w, z)
        h = torch.empty_like(z)
        call("mmskin_gelu_forward", ptr(z), ptr(h), z.numel(), stream())
        ctx.mk = (z.shape[0], x.shape[-1])
        ctx.has_bias = b is not None
        ctx.xshape = x.shape
        return h.reshape(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dh):
        xs, w, z = ctx.saved_tensors
        M, K = ctx.mk
        N = w.shape[0]
        dh2 = _f32c(dh).reshape(M, N)
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dx = torch.empty((M, K), device=dh.device, dtype=torch.float32) if need_x else None
        dw = torch.empty_like(w) if need_w else None
        db = torch.empty(N, device=dh.device, dtype=torch.float32) if need_b else None
        # off the bf16-operand large-GEMM path (linear.hip: linear_path) the C side applies gelu'(z) in a pass of its own
        # (mmskin_linear_x16_pitch(M, K, N) > 0 IS that predicate, asked of the library instead of re-derived here: ADVICE r03)
        fused = _lib.load().mmskin_linear_x16_pitch(M, K, N) > 0
        scratch = None if fused else torch.empty_like(dh2)
        if ctx.kept:
            call("mmskin_linear_backward_keep", ptr(dh2), ptr(xs), ptr(w), None, ptr(z), ptr(scratch), ptr(dx), ptr(dw), ptr(db), M, K, N, stream())
        else:
            call("mmskin_linear_gelu_backward", ptr(dh2), ptr(xs), ptr(w), ptr(z), ptr(scratch), ptr(dx), ptr(dw), ptr(db), M, K, N, stream())
        return (dx.reshape(ctx.xshape) if need_x else None), dw, db


def linear_gelu(x, w, b=None, out_dtype=None):
    """gelu(x @ w.T + b) -- the first half of a transformer MLP.  Without gradients (frozen encoders, inference) bias and the
    exact GELU run in the GEMM epilogue (one launch, the pre-activation never reaches memory); with gradients the two ops
    stay separate because GELU's backward needs the pre-activation."""
    if _needs_grad(x, w, b):
        if x.is_cuda and x.dtype == torch.float32 and w.dtype == torch.float32:
            return LinearGeluFn.apply(x, w, b)
        return gelu(linear(x, w, b))
    if x.dtype == torch.bfloat16 or out_dtype == torch.bfloat16:
        return linear_lane(x, w, b, 2, out_dtype=out_dtype)
    with torch.no_grad():
        return LinearFn.apply(x, w, b, 2)


@no_second_order
class MlpFn(torch.autograd.Function):
    """[res +] fc2(act(fc1(x))) with gradients (timm Mlp.forward and the block's skip connection) on the bf16-operand large-GEMM path;
    act is the exact GELU (s and sb None) or timm's StarReLU s * relu(z)^2 + sb.  The hidden activation exists only as the
    pre-activation z (fp32, for the derivative) and as the bf16 operand of fc2 -- act(z) is never written in fp32; the residual is
    added in the pass that writes the output.  Backward: two C calls (fc2's, then fc1's with act'(z) inside the pass that converts dh
    -- for StarReLU the gradients of s and sb come from that pass too), each on the bf16 operand copy kept from the forward."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, s, sb, res, p1, p2):
        _need_gpu(x, "mlp")
        x2 = _f32c(x).reshape(-1, x.shape[-1])
        w1, w2 = _f32c(w1), _f32c(w2)
        M, K = x2.shape
        Hd, N = w1.shape[0], w2.shape[0]
        z = torch.empty((M, Hd), device=x.device, dtype=torch.float32)
        x16 = torch.empty((M, p1), device=x.device, dtype=torch.bfloat16)
        call("mmskin_linear_forward_keep", ptr(x2), ptr(w1), ptr(b1), None, ptr(z), ptr(x16), M, K, Hd, 0, stream())
        h16 = torch.empty((M, p2), device=x.device, dtype=torch.bfloat16)
        if s is None:
            call("mmskin_gelu_forward_bf16", ptr(z), ptr(h16), M, Hd, p2, stream())
        else:
            s, sb = _f32c(s), _f32c(sb)
            call("mmskin_star_relu_forward_bf16", ptr(z), ptr(s), ptr(sb), ptr(h16), M, Hd, p2, stream())
        y = torch.empty((M, N), device=x.device, dtype=torch.float32)
        r2 = _f32c(res).reshape(M, N) if res is not None else None
        call("mmskin_linear_forward_x16", ptr(h16), ptr(w2), ptr(b2), ptr(r2), ptr(y), M, Hd, N, 0, stream())
        ctx.save_for_backward(x16, w1, z, h16, w2, s)
        ctx.dims = (M, K, Hd, N)
        ctx.bias = (b1 is not None, b2 is not None)
        ctx.xshape = x.shape
        ctx.res_shape = None if res is None else res.shape
        return y.reshape(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x16, w1, z, h16, w2, s = ctx.saved_tensors
        M, K, Hd, N = ctx.dims
        dy2 = _f32c(dy).reshape(M, N)
        ng = ctx.needs_input_grad
        dev = dy.device
        dh = torch.empty((M, Hd), device=dev, dtype=torch.float32)
        dw2 = torch.empty_like(w2) if ng[3] else None
        db2 = torch.empty(N, device=dev, dtype=torch.float32) if ctx.bias[1] and ng[4] else None
        call("mmskin_linear_backward_keep", ptr(dy2), ptr(h16), ptr(w2), None, None, None, ptr(dh), ptr(dw2), ptr(db2), M, Hd, N, stream())
        dx = torch.empty((M, K), device=dev, dtype=torch.float32) if ng[0] else None
        dw1 = torch.empty_like(w1) if ng[1] else None
        db1 = torch.empty(Hd, device=dev, dtype=torch.float32) if ctx.bias[0] and ng[2] else None
        if s is None:
            call("mmskin_linear_backward_keep", ptr(dh), ptr(x16), ptr(w1), None, ptr(z), None, ptr(dx), ptr(dw1), ptr(db1), M, K, Hd, stream())
            ds = dsbias = None
        else:
            dsb = torch.empty(2, device=dev, dtype=torch.float32)
            call("mmskin_linear_star_relu_backward_keep", ptr(dh), ptr(x16), ptr(w1), ptr(z), ptr(s), ptr(dsb), ptr(dx), ptr(dw1), ptr(db1),
                 M, K, Hd, stream())
            ds, dsbias = _split_dsb(dsb, s, s, ng[5], ng[6])
        dres = dy2.reshape(ctx.res_shape) if ctx.res_shape is not None and ng[7] else None
        return (dx.reshape(ctx.xshape) if dx is not None else None), dw1, db1, dw2, db2, ds, dsbias, dres, None, None


def mlp(x, w1, b1, w2, b2, residual=None, star_relu=None):
    """[residual +] fc2(act(fc1(x))), act = exact GELU (default) or, with star_relu=(scale, bias), timm's StarReLU
    scale * relu(z)^2 + bias.  With gradients, fp32 tensors on the GPU and both Linears on the bf16-operand large-GEMM path: MlpFn
    (no fp32 act(z), kept bf16 operands, residual added by the output pass; its StarReLU kernels take hidden widths that are multiples
    of 4); otherwise the separate ops."""
    s, sb = star_relu if star_relu is not None else (None, None)
    if (_needs_grad(x, w1, b1, w2, b2, s, sb) and x.is_cuda and x.dtype == torch.float32 and w1.dtype == torch.float32 and w2.dtype == torch.float32
            and w1.requires_grad and w2.requires_grad and (s is None or w1.shape[0] % 4 == 0)
            and (residual is None or residual.dtype == torch.float32)):
        M = x.numel() // x.shape[-1]
        lib = _lib.load()
        p1 = lib.mmskin_linear_x16_pitch(M, x.shape[-1], w1.shape[0])
        p2 = lib.mmskin_linear_x16_pitch(M, w1.shape[0], w2.shape[0])
        if p1 and p2:
            return MlpFn.apply(x, w1, b1, w2, b2, s, sb, residual, p1, p2)
    if s is None:
        return linear(linear_gelu(x, w1, b1), w2, b2, residual=residual)
    return linear(StarReluFn.apply(linear(x, w1, b1), s, sb), w2, b2, residual=residual)


@no_second_order
class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm over the last dim, optional fused ReLU; b may be None (a LayerNorm without bias: no bias gradient)."""

    @staticmethod
    def forward(ctx, x, g, b, eps, relu):
        _need_gpu(x, "layernorm")
        N = x.shape[-1]
        x2 = _f32c(x).reshape(-1, N)
        M = x2.shape[0]
        y = torch.empty_like(x2)
        mean = torch.empty(M, device=x.device, dtype=torch.float32)
        rstd = torch.empty(M, device=x.device, dtype=torch.float32)
        call("mmskin_layernorm_forward", ptr(x2), ptr(g), ptr(b), ptr(y), ptr(mean), ptr(rstd), M, N, float(eps),
             int(relu), stream())
        ctx.save_for_backward(x2, g, b, mean, rstd)
        ctx.relu = relu
        ctx.xshape = x.shape
        return y.reshape(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, g, b, mean, rstd = ctx.saved_tensors
        M, N = x2.shape
        dy2 = _f32c(dy).reshape(M, N)
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        dg = torch.empty_like(g) if ctx.needs_input_grad[1] else None
        db = torch.empty_like(b) if b is not None and ctx.needs_input_grad[2] else None
        call("mmskin_layernorm_backward", ptr(dy2), ptr(x2), ptr(g), ptr(b), ptr(mean), ptr(rstd), ptr(dx), ptr(dg),
             ptr(db), M, N, int(ctx.relu), stream())
        return (dx.reshape(ctx.xshape) if dx is not None else None), dg, db, None, None


def layernorm(x, g, b, eps=1e-5, relu=False, out_dtype=None, keep_f32=False):
    """nn.LayerNorm (b=None: without bias).  out_dtype=torch.bfloat16 (inference lane): the result as a bf16 tensor -- and with keep_f32 also the fp32
    one (post-LN residual streams), returned as (fp32, bf16) -- from one pass over the row."""
    N = x.shape[-1]
    if out_dtype == torch.bfloat16 and not relu and N % 4 == 0 and N <= 2048 and not _needs_grad(x, g, b):
        _need_gpu(x, "layernorm")
        x2 = _f32c(x).reshape(-1, N)
        y16 = torch.empty(x2.shape, device=x.device, dtype=torch.bfloat16)
        y32 = torch.empty_like(x2) if keep_f32 else None
        call("mmskin_layernorm_forward_mixed", ptr(x2), ptr(_f32c(g)), ptr(None if b is None else _f32c(b)), ptr(y32), ptr(y16), x2.shape[0], N, float(eps), stream())
        return (y32.reshape(x.shape), y16.reshape(x.shape)) if keep_f32 else y16.reshape(x.shape)
    y = LayerNormFn.apply(x, g, b, eps, relu)
    return (y, y) if keep_f32 else y


@no_second_order
class SigmoidGateFn(torch.autograd.Function):
    """sigmoid(z) * v."""

    @staticmethod
    def forward(ctx, z, v):
        _need_gpu(z, "sigmoid_gate")
        z, v = _f32c(z), _f32c(v)
        out = torch.empty_like(z)
        call("mmskin_sigmoid_gate_forward", ptr(z), ptr(v), ptr(out), z.numel(), stream())
        ctx.save_for_backward(z, v)
        return out

    @staticmethod
    def backward(ctx, dout):
        z, v = ctx.saved_tensors
        dout = _f32c(dout)
        dz, dv = torch.empty_like(z), torch.empty_like(v)
        call("mmskin_sigmoid_gate_backward", ptr(dout), ptr(z), ptr(v), ptr(dz), ptr(dv), z.numel(), stream())
        return dz, dv


sigmoid_gate = SigmoidGateFn.apply


@no_second_order
class GatedMixFn(torch.autograd.Function):
    """g*a + (1-g)*q with g = sigmoid(z)."""

    @staticmethod
    def forward(ctx, z, a, q):
        _need_gpu(z, "gated_mix")
        z, a, q = _f32c(z), _f32c(a), _f32c(q)
        out = torch.empty_like(z)
        call("mmskin_gated_mix_forward", ptr(z), ptr(a), ptr(q), ptr(out), z.numel(), stream())
        ctx.save_for_backward(z, a, q)
        return out

    @staticmethod
    def backward(ctx, dout):
        z, a, q = ctx.saved_tensors
        dout = _f32c(dout)
        dz, da, dq = torch.empty_like(z), torch.empty_like(a), torch.empty_like(q)
        call("mmskin_gated_mix_backward", ptr(dout), ptr(z), ptr(a), ptr(q), ptr(dz), ptr(da), ptr(dq), z.numel(),
             stream())
        return dz, da, dq


gated_mix = GatedMixFn.apply


@no_second_order
class MetaBlockGateFn(torch.autograd.Function):
    """sigmoid(tanh(V*t1) + t2)."""

    @staticmethod
    def forward(ctx, V, t1, t2):
        _need_gpu(V, "metablock_gate")
        V, t1, t2 = _f32c(V), _f32c(t1), _f32c(t2)
        out = torch.empty_like(V)
        call("mmskin_metablock_gate_forward", ptr(V), ptr(t1), ptr(t2), ptr(out), V.numel(), stream())
        ctx.save_for_backward(V, t1, t2)
        return out

    @staticmethod
    def backward(ctx, dout):
        V, t1, t2 = ctx.saved_tensors
        dout = _f32c(dout)
        dV, d1, d2 = torch.empty_like(V), torch.empty_like(t1), torch.empty_like(t2)
        call("mmskin_metablock_gate_backward", ptr(dout), ptr(V), ptr(t1), ptr(t2), ptr(dV), ptr(d1), ptr(d2),
             V.numel(), stream())
        return dV, d1, d2


metablock_gate = MetaBlockGateFn.apply


@no_second_order
class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, offset):
        _need_gpu(x, "dropout")
        x = _f32c(x)
        y = torch.empty_like(x)
        mask = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
        call("mmskin_dropout_forward", ptr(x), ptr(y), ptr(mask), x.numel(), float(p), int(seed), int(offset), stream())
        ctx.save_for_backward(mask)
        ctx.p = p
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        dy = _f32c(dy)
        dx = torch.empty_like(dy)
        call("mmskin_dropout_backward", ptr(dy), ptr(mask), ptr(dx), dy.numel(), float(ctx.p), stream())
        return dx, None, None, None


def dropout(x, p, training):
    if not training or p <= 0.0:
        return x
    # seed from torch's generator state so torch.manual_seed controls the masks; the call consumes counters [offset, offset + numel)
    seed, offset = _dropout_state(p, x.numel())
    return DropoutFn.apply(x, p, seed, offset)


@no_second_order
class Concat2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _need_gpu(a, "concat2")
        a, b = _f32c(a), _f32c(b)
        M, Na = a.shape
        Nb = b.shape[1]
        out = torch.empty((M, Na + Nb), device=a.device, dtype=torch.float32)
        call("mmskin_concat2_forward", ptr(a), ptr(b), ptr(out), M, Na, Nb, stream())
        ctx.dims = (M, Na, Nb)
        return out

    @staticmethod
    def backward(ctx, dout):
        M, Na, Nb = ctx.dims
        dout = _f32c(dout)
        da = torch.empty((M, Na), device=dout.device, dtype=torch.float32)
        db = torch.empty((M, Nb), device=dout.device, dtype=torch.float32)
        call("mmskin_concat2_backward", ptr(dout), ptr(da), ptr(db), M, Na, Nb, stream())
        return da, db


concat2 = Concat2Fn.apply


@no_second_order
class MDNetFuseFn(torch.autograd.Function):
    """mean_hw(sigmoid(z) * f + sigmoid(tanh(f * t1) + t2)) for f [N, C, H, W]; z, t1, t2 [N, C] -> [N, C]."""

    @staticmethod
    def forward(ctx, feat, z, t1, t2):
        _need_gpu(feat, "mdnet_fuse")
        feat, z, t1, t2 = _f32c(feat), _f32c(z), _f32c(t1), _f32c(t2)
        N, C, H, W = feat.shape
        pooled = torch.empty((N, C), device=feat.device, dtype=torch.float32)
        call("mmskin_mdnet_fuse_forward", ptr(feat), ptr(z), ptr(t1), ptr(t2), ptr(pooled), N * C, H * W, stream())
        ctx.save_for_backward(feat, z, t1, t2)
        return pooled

    @staticmethod
    def backward(ctx, dp):
        feat, z, t1, t2 = ctx.saved_tensors
        N, C, H, W = feat.shape
        dp = _f32c(dp)
        dfeat = torch.empty_like(feat) if ctx.needs_input_grad[0] else None
        dz, dt1, dt2 = torch.empty_like(z), torch.empty_like(t1), torch.empty_like(t2)
        call("mmskin_mdnet_fuse_backward", ptr(dp), ptr(feat), ptr(z), ptr(t1), ptr(t2),
             ptr(dfeat) if dfeat is not None else None, ptr(dz), ptr(dt1), ptr(dt2), N * C, H * W, stream())
        return dfeat, dz, dt1, dt2


mdnet_fuse = MDNetFuseFn.apply


@no_second_order
class AddFn(torch.autograd.Function):
    """a + b with b broadcast over a's leading dimensions (residual sums, position embeddings)."""

    @staticmethod
    def forward(ctx, a, b):
        _need_gpu(a, "add")
        a, b = _f32c(a), _f32c(b)
        y = torch.empty_like(a)
        call("mmskin_add", ptr(a), ptr(b), ptr(y), a.numel(), b.numel(), stream())
        ctx.bshape = b.shape
        ctx.lead = a.numel() // b.numel()
        return y

    @staticmethod
    def backward(ctx, dy):
        db = dy if ctx.lead == 1 else dy.reshape(ctx.lead, -1).sum(0).reshape(ctx.bshape)
        return dy, db


add = AddFn.apply


@no_second_order
class ScaleAddFn(torch.autograd.Function):
    """x + gamma[c] * b   (timm LayerScale residual: x + gamma_1 * attn(norm1(x)))."""

    @staticmethod
    def forward(ctx, x, b, gamma):
        _need_gpu(x, "scale_add")
        x, b, gamma = _f32c(x), _f32c(b), _f32c(gamma)
        y = torch.empty_like(x)
        call("mmskin_scale_add_forward", ptr(x), ptr(b), ptr(gamma), ptr(y), x.numel(), gamma.numel(), stream())
        ctx.save_for_backward(b, gamma)
        return y

    @staticmethod
    def backward(ctx, dy):
        b, gamma = ctx.saved_tensors
        dy = _f32c(dy)
        C = gamma.numel()
        db = torch.empty_like(dy)
        call("mmskin_scale_mul", ptr(dy), ptr(gamma), ptr(db), dy.numel(), C, 1, stream())
        prod = torch.empty_like(dy)
        call("mmskin_scale_mul", ptr(dy), ptr(b), ptr(prod), dy.numel(), C, 0, stream())
        dgamma = torch.empty_like(gamma)
        call("mmskin_colsum", ptr(prod), ptr(dgamma), dy.numel() // C, C, stream())
        return dy, db, dgamma


scale_add = ScaleAddFn.apply


@no_second_order
class TokenMeanFn(torch.autograd.Function):
    """mean over tokens [start, L) of x [B, L, E]   (timm global_pool='avg' over the patch tokens)."""

    @staticmethod
    def forward(ctx, x, start):
        _need_gpu(x, "token_mean")
        x = _f32c(x)
        B, L, E = x.shape
        out = torch.empty((B, E), device=x.device, dtype=torch.float32)
        call("mmskin_token_mean_forward", ptr(x), ptr(out), B, L, E, int(start), stream())
        ctx.dims = (B, L, E, int(start))
        return out

    @staticmethod
    def backward(ctx, dout):
        B, L, E, start = ctx.dims
        dout = _f32c(dout)
        dx = torch.empty((B, L, E), device=dout.device, dtype=torch.float32)
        call("mmskin_token_mean_backward", ptr(dout), ptr(dx), B, L, E, start, stream())
        return dx, None


token_mean = TokenMeanFn.apply


@no_second_order
class PatchColsFn(torch.autograd.Function):
    """im2col for the patch-embedding GEMMs: x [N, C, H, W] (channels_last=False) or [N, H, W, C] (True), fp32 ->
    cols [N*OH*OW, C*k*k] with columns ordered (c, ky, kx) like conv.weight.flatten(1); zero padding."""

    @staticmethod
    def forward(ctx, x, k, stride, pad, channels_last):
        _need_gpu(x, "patch_cols")
        x = _f32c(x)
        if channels_last:
            N, H, W, C = x.shape
        else:
            N, C, H, W = x.shape
        OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        cols = torch.empty((N * OH * OW, C * k * k), device=x.device, dtype=torch.float32)
        call("mmskin_im2col_forward", ptr(x), N, C, H, W, k, stride, pad, int(channels_last), ptr(cols), stream())
        ctx.geom = (N, C, H, W, k, stride, pad, int(channels_last), tuple(x.shape))
        return cols

    @staticmethod
    def backward(ctx, dcols):
        N, C, H, W, k, stride, pad, cl, shape = ctx.geom
        dcols = _f32c(dcols)
        dx = torch.empty(shape, device=dcols.device, dtype=torch.float32)
        call("mmskin_im2col_backward", ptr(dcols), N, C, H, W, k, stride, pad, cl, ptr(dx), stream())
        return dx, None, None, None, None


def patch_cols(x, k, stride, pad=0, channels_last=False):
    return PatchColsFn.apply(x, k, stride, pad, channels_last)


@no_second_order
class DwConv3Fn(torch.autograd.Function):
    """Depthwise 3x3 (stride 1, pad 1) on NHWC fp32: x [N, H, W, C], w [C, 1, 3, 3] -> [N, H, W, C]."""

    @staticmethod
    def forward(ctx, x, w):
        _need_gpu(x, "dwconv3")
        x, w = _f32c(x), _f32c(w)
        N, H, W, C = x.shape
        y = torch.empty_like(x)
        stage = torch.empty(9 * C, device=x.device, dtype=torch.float32)
        call("mmskin_dwconv3_forward", ptr(x), ptr(w), ptr(stage), ptr(y), N, H, W, C, stream())
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        N, H, W, C = x.shape
        dy = _f32c(dy)
        stage = torch.empty(9 * C, device=x.device, dtype=torch.float32)
        scratch = torch.empty(_lib.load().mmskin_dwconv3_scratch_floats(N, H, W, C), device=x.device, dtype=torch.float32)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        call("mmskin_dwconv3_backward", ptr(dy), ptr(x), ptr(w), ptr(stage), ptr(scratch), ptr(dx) if dx is not None else None,
             ptr(dw) if dw is not None else None, N, H, W, C, stream())
        return dx, dw


dwconv3 = DwConv3Fn.apply


@no_second_order
class ConvPosEncFn(torch.autograd.Function):
    """x + dwconv3(x, w) + b on NHWC fp32 (timm davit.py ConvPosEnc.forward) in one kernel; the backward's dx = dy + dgrad(dy) in one
    kernel and dw, db from one pass over dy."""

    @staticmethod
    def forward(ctx, x, w, b):
        _need_gpu(x, "conv_pos_enc")
        x, w, b = _f32c(x), _f32c(w), _f32c(b)
        N, H, W, C = x.shape
        y = torch.empty_like(x)
        stage = torch.empty(9 * C, device=x.device, dtype=torch.float32)
        call("mmskin_conv_pos_enc_forward", ptr(x), ptr(w), ptr(b), ptr(stage), ptr(y), N, H, W, C, stream())
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        N, H, W, C = x.shape
        dy = _f32c(dy)
        stage = torch.empty(9 * C, device=x.device, dtype=torch.float32)
        scratch = torch.empty(_lib.load().mmskin_dwconv3_scratch_floats(N, H, W, C), device=x.device, dtype=torch.float32)
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if need_w else None
        db = torch.empty(C, device=x.device, dtype=torch.float32) if ctx.needs_input_grad[2] else None
        call("mmskin_conv_pos_enc_backward", ptr(dy), ptr(x), ptr(w), ptr(stage), ptr(scratch), ptr(dx), ptr(dw), ptr(db), N, H, W, C, stream())
        return dx, (dw if ctx.needs_input_grad[1] else None), db


conv_pos_enc = ConvPosEncFn.apply


@no_second_order
class ConvPosEncTokensFn(torch.autograd.Function):
    """timm coat.py ConvPosEnc.forward on a token tensor with a class token, fp32 x [B, 1 + H * W, C]: the class row passes through, the
    image rows get x + dwconv3(x, w) + b on the H x W grid -- one kernel, no slice / concat copies; dw and db from one pass over dy."""

    @staticmethod
    def forward(ctx, x, H, W, w, b):
        _need_gpu(x, "conv_pos_enc_tokens")
        x, w, b = _f32c(x), _f32c(w), _f32c(b)
        B, N, C = x.shape
        if N != 1 + H * W:
            raise _lib.MMSkinError(f"mmskin.conv_pos_enc_tokens: {N} tokens are not 1 + {H} * {W}")
        y = torch.empty_like(x)
        call("mmskin_conv_pos_enc_tokens_forward", ptr(x), ptr(w), ptr(b), ptr(y), B, H, W, C, stream())
        ctx.save_for_backward(x, w)
        ctx.hw = (int(H), int(W))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        B, N, C = x.shape
        H, W = ctx.hw
        dy = _f32c(dy)
        need_w = ctx.needs_input_grad[3] or ctx.needs_input_grad[4]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[3] else None
        db = torch.empty(C, device=x.device, dtype=torch.float32) if ctx.needs_input_grad[4] else None
        scratch = None
        if need_w:
            scratch = torch.empty(_lib.load().mmskin_conv_pos_enc_tokens_scratch_floats(B, H, W, C), device=x.device, dtype=torch.float32)
        call("mmskin_conv_pos_enc_tokens_backward", ptr(dy), ptr(x), ptr(w), ptr(scratch), ptr(dx), ptr(dw), ptr(db), B, H, W, C, stream())
        return dx, None, None, dw, db


def conv_pos_enc_tokens(x, H, W, w, b):
    return ConvPosEncTokensFn.apply(x, H, W, w, b)


FACTOR_ATTENTION_WIDTHS = (8, 16, 32, 40, 64)


@no_second_order
class FactorAttentionFn(torch.autograd.Function):
    """CoaT factorized attention with convolutional relative position encoding (timm coat.py FactorAttnConvRelPosEnc.forward) on the packed
    qkv of a fused Linear, qkv [B, 1 + H * W, 3, 8, Ch] -> [B, 1 + H * W, 8 * Ch] (token-major, what the output projection reads):
    Ch^-0.5 * q (softmax_tokens(k)^T v) + q_img * (dwconv(v_img) + bias) with the 3x3 / 5x5 / 7x7 windows on heads 0-1 / 2-4 / 5-7.
    No permute / contiguous copies; the backward writes d(qkv) in the packed layout and recomputes the softmax and the convolution."""

    @staticmethod
    def forward(ctx, qkv, H, W, w3, w5, w7, b3, b5, b7):
        _need_gpu(qkv, "factor_attention")
        qkv = _f32c(qkv)
        B, N, three, heads, Ch = qkv.shape
        if three != 3 or heads != 8 or Ch not in FACTOR_ATTENTION_WIDTHS or N != 1 + H * W:
            raise _lib.MMSkinError(f"mmskin.factor_attention: qkv {tuple(qkv.shape)} is not [B, 1 + {H} * {W}, 3, 8, Ch in {FACTOR_ATTENTION_WIDTHS}]")
        ws = [_f32c(t) for t in (w3, b3, w5, b5, w7, b7)]
        for t, k, n in zip(ws[0::2], (3, 5, 7), (2, 3, 3)):
            if tuple(t.shape) != (n * Ch, 1, k, k):
                raise _lib.MMSkinError(f"mmskin.factor_attention: window-{k} weight {tuple(t.shape)}, expected {(n * Ch, 1, k, k)}")
        for t, n in zip(ws[1::2], (2, 3, 3)):
            if tuple(t.shape) != (n * Ch,):
                raise _lib.MMSkinError(f"mmskin.factor_attention: bias {tuple(t.shape)}, expected {(n * Ch,)}")
        att = torch.empty((B, N, 8 * Ch), device=qkv.device, dtype=torch.float32)
        F = torch.empty((B * 8, Ch, Ch), device=qkv.device, dtype=torch.float32)
        stats = torch.empty((B * 8, 2, Ch), device=qkv.device, dtype=torch.float32)
        scratch = torch.empty(_lib.load().mmskin_factor_attention_scratch_floats(B, H, W, Ch, 0), device=qkv.device, dtype=torch.float32)
        call("mmskin_factor_attention_forward", ptr(qkv), *[ptr(t) for t in ws], ptr(att), ptr(F), ptr(stats), ptr(scratch), B, H, W, Ch, stream())
        ctx.save_for_backward(qkv, F, stats, *ws)
        ctx.hw = (int(H), int(W))
        return att

    @staticmethod
    def backward(ctx, dO):
        qkv, F, stats, *ws = ctx.saved_tensors
        B, N, three, heads, Ch = qkv.shape
        H, W = ctx.hw
        dO = _f32c(dO)
        dqkv = torch.empty_like(qkv)
        dws = [torch.empty_like(t) for t in ws]
        scratch = torch.empty(_lib.load().mmskin_factor_attention_scratch_floats(B, H, W, Ch, 1), device=qkv.device, dtype=torch.float32)
        call("mmskin_factor_attention_backward", ptr(dO), ptr(qkv), *[ptr(t) for t in ws], ptr(F), ptr(stats), ptr(dqkv), *[ptr(t) for t in dws],
             ptr(scratch), B, H, W, Ch, stream())
        dw3, db3, dw5, db5, dw7, db7 = dws
        return dqkv, None, None, dw3, dw5, dw7, db3, db5, db7


def factor_attention(qkv, H, W, crpe_weights, crpe_biases):
    """qkv [B, 1 + H * W, 3, 8, Ch]; crpe_weights / crpe_biases: the three conv_list weights (window 3, 5, 7) and biases."""
    w3, w5, w7 = crpe_weights
    b3, b5, b7 = crpe_biases
    return FactorAttentionFn.apply(qkv, H, W, w3, w5, w7, b3, b5, b7)


@no_second_order
class Dw7StarFn(torch.autograd.Function):
    """CAFormer SepConv core on NHWC fp32: dwconv7x7(s * relu(z)^2 + b, w), z [N, H, W, C], w [C, 1, 7, 7] (stride 1, pad 3, no bias).
    The StarReLU is applied as z is staged (act(z) is never written); the backward reads dy and z once for dz, dw and the gradients of
    s and b (fixed-order reductions over per-workgroup partials in a scratch buffer)."""

    @staticmethod
    def forward(ctx, z, w, s, b):
        _need_gpu(z, "dw7_star")
        z, w, s, b = _f32c(z), _f32c(w), _f32c(s), _f32c(b)
        N, H, W, C = z.shape
        y = torch.empty_like(z)
        call("mmskin_dw7_star_forward", ptr(z), ptr(w), ptr(s), ptr(b), ptr(y), N, H, W, C, stream())
        ctx.save_for_backward(z, w, s, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        z, w, s, b = ctx.saved_tensors
        N, H, W, C = z.shape
        dy = _f32c(dy)
        ng = ctx.needs_input_grad
        scratch = torch.empty(_lib.load().mmskin_dw7_star_scratch_floats(N, H, W, C), device=dy.device, dtype=torch.float32)
        dz = torch.empty_like(z) if ng[0] else None
        dw = torch.empty_like(w) if ng[1] else None
        dsb = torch.empty(2, device=dy.device, dtype=torch.float32) if ng[2] or ng[3] else None
        call("mmskin_dw7_star_backward", ptr(dy), ptr(z), ptr(w), ptr(s), ptr(b), ptr(scratch), ptr(dz), ptr(dw), ptr(dsb), N, H, W, C, stream())
        return (dz, dw) + _split_dsb(dsb, s, b, ng[2], ng[3])


dw7_star = Dw7StarFn.apply


@no_second_order
class EmbeddingFn(torch.autograd.Function):
    """table [ncols, card, E], ids [B, ncols] -> [B, ncols, E]."""

    @staticmethod
    def forward(ctx, table, ids):
        _need_gpu(table, "embedding")
        table = _f32c(table)
        ids = ids.long().contiguous()
        ncols, card, E = table.shape
        B = ids.shape[0]
        out = torch.empty((B, ncols, E), device=table.device, dtype=torch.float32)
        call("mmskin_embedding_forward", ptr(table), ptr(ids), ptr(out), B, ncols, card, E, stream())
        ctx.save_for_backward(ids)
        ctx.dims = (B, ncols, card, E)
        return out

    @staticmethod
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        B, ncols, card, E = ctx.dims
        dout = _f32c(dout)
        dtable = torch.empty((ncols, card, E), device=dout.device, dtype=torch.float32)
        call("mmskin_embedding_backward", ptr(dout), ptr(ids), ptr(dtable), B, ncols, card, E, stream())
        return dtable, None


embedding = EmbeddingFn.apply


@no_second_order
class DirectConvFn(torch.autograd.Function):
    """Small direct NCHW conv (+bias, optional ReLU) for the `custom-cnn` stem (no input gradient)."""

    @staticmethod
    def forward(ctx, x, w, b, stride, pad, relu):
        _need_gpu(x, "direct_conv2d")
        x, w = _f32c(x), _f32c(w)
        N, Cin, H, W = x.shape
        Cout, _, kh, kw = w.shape
        OH, OW = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
        y = torch.empty((N, Cout, OH, OW), device=x.device, dtype=torch.float32)
        call("mmskin_direct_conv2d_forward", ptr(x), ptr(w), ptr(b), ptr(y), N, Cin, H, W, Cout, kh, kw, stride, pad,
             int(relu), stream())
        ctx.save_for_backward(x, w, y if relu else None)
        ctx.cfg = (stride, pad, b is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        stride, pad, has_bias = ctx.cfg
        dy = _f32c(dy)
        N, Cin, H, W = x.shape
        Cout, _, kh, kw = w.shape
        dw = torch.empty_like(w)
        db = torch.empty(Cout, device=dy.device, dtype=torch.float32) if has_bias else None
        call("mmskin_direct_conv2d_backward", ptr(dy), ptr(x), ptr(y), ptr(dw), ptr(db), N, Cin, H, W, Cout, kh, kw,
             stride, pad, stream())
        return None, dw, db, None, None, None


direct_conv2d = DirectConvFn.apply


@no_second_order
class PoolGapFn(torch.autograd.Function):
    """MaxPool2d(k) followed by AdaptiveAvgPool2d(1)+Flatten: [N,C,H,W] -> [N,C]."""

    @staticmethod
    def forward(ctx, x, k):
        _need_gpu(x, "pool_gap")
        x = _f32c(x)
        N, C, H, W = x.shape
        y = torch.empty((N, C), device=x.device, dtype=torch.float32)
        idx = torch.empty((N, C, H // k, W // k), device=x.device, dtype=torch.int32)
        call("mmskin_pool_gap_forward", ptr(x), ptr(y), ptr(idx), N, C, H, W, k, stream())
        ctx.save_for_backward(idx)
        ctx.cfg = (N, C, H, W, k)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        N, C, H, W, k = ctx.cfg
        dy = _f32c(dy)
        dx = torch.empty((N, C, H, W), device=dy.device, dtype=torch.float32)
        call("mmskin_pool_gap_backward", ptr(dy), ptr(idx), ptr(dx), N, C, H, W, k, stream())
        return dx, None


pool_gap = PoolGapFn.apply


# ---------------------------------------------------------------------------------------------- Score-CAM (forward only)
def _scorecam_dims(fmap, size):
    _need_gpu(fmap, "scorecam")
    if fmap.dim() != 3 or fmap.dtype != torch.float32 or not fmap.is_contiguous():
        raise _lib.MMSkinError(f"scorecam: the feature map must be a contiguous fp32 [C, fh, fw] tensor, got {tuple(fmap.shape)} {fmap.dtype}")
    return tuple(fmap.shape) + (int(size[0]), int(size[1]))


def scorecam_minmax(fmap, size):
    """(min, max) of every channel of fmap [C, fh, fw] after the bilinear upsample to size = (H, W) -> [C, 2]."""
    C, fh, fw, H, W = _scorecam_dims(fmap, size)
    out = torch.empty((C, 2), device=fmap.device, dtype=torch.float32)
    call("mmskin_scorecam_minmax", ptr(fmap), C, fh, fw, H, W, ptr(out), stream())
    return out


def scorecam_mask(fmap, minmax, image, c0, n, n_pad, out=None):
    """Masked inputs of channels c0 .. c0 + n: image [3, H, W] times each channel's normalised upsampled map -> [n_pad, 3, H, W],
    rows n .. n_pad zero.  `out` (same shape, fp32, contiguous) is overwritten when given."""
    _need_gpu(image, "scorecam_mask")
    if image.dim() != 3 or image.shape[0] != 3 or image.dtype != torch.float32 or not image.is_contiguous():
        raise _lib.MMSkinError(f"scorecam_mask: the image must be a contiguous fp32 [3, H, W] tensor, got {tuple(image.shape)} {image.dtype}")
    C, fh, fw, H, W = _scorecam_dims(fmap, image.shape[1:])
    if tuple(minmax.shape) != (C, 2) or minmax.dtype != torch.float32 or not minmax.is_contiguous():
        raise _lib.MMSkinError("scorecam_mask: minmax must be the [C, 2] fp32 result of scorecam_minmax")
    if out is None:
        out = torch.empty((max(int(n_pad), 0), 3, H, W), device=fmap.device, dtype=torch.float32)
    elif tuple(out.shape) != (n_pad, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous():
        raise _lib.MMSkinError(f"scorecam_mask: out must be a contiguous fp32 {(n_pad, 3, H, W)} tensor")
    call("mmskin_scorecam_mask", ptr(fmap), ptr(minmax), ptr(image), C, fh, fw, H, W, int(c0), int(n), int(n_pad), ptr(out), stream())
    return out


def scorecam_combine(fmap, minmax, scores, size, channel_block=0):
    """Heat map [H, W]: sum of scores[c] * normalised upsampled channel c (fp32, ascending c), ReLU, min-max normalised.  A flat
    combined map comes back as NaN, as in the reference (no zero guard on the last division)."""
    C, fh, fw, H, W = _scorecam_dims(fmap, size)
    if tuple(minmax.shape) != (C, 2) or minmax.dtype != torch.float32 or not minmax.is_contiguous():
        raise _lib.MMSkinError("scorecam_combine: minmax must be the [C, 2] fp32 result of scorecam_minmax")
    if tuple(scores.shape) != (C,) or scores.dtype != torch.float32 or not scores.is_contiguous() or not scores.is_cuda:
        raise _lib.MMSkinError(f"scorecam_combine: scores must be a contiguous fp32 [{C}] device tensor")
    heat = torch.empty((H, W), device=fmap.device, dtype=torch.float32)
    call("mmskin_scorecam_combine", ptr(fmap), ptr(minmax), ptr(scores), C, fh, fw, H, W, int(channel_block), ptr(heat), stream())
    return heat


# ---------------------------------------------------------------------------------------------- Grad-CAM / Grad-CAM++ (forward only)
GRADCAM, GRADCAM_PLUSPLUS = 0, 1          # `mode` of mmskin_gradcam_weights


def _gradcam_dims(acts, row_image, what):
    _need_gpu(acts, what)
    if acts.dim() != 4 or acts.dtype != torch.float32 or not acts.is_contiguous():
        raise ValueError(f"{what}: the activations must be a contiguous fp32 [N, C, fh, fw] tensor, got {tuple(acts.shape)} {acts.dtype}")
    if not torch.is_tensor(row_image) or not row_image.is_cuda or row_image.dim() != 1 or row_image.dtype != torch.int32 \
            or not row_image.is_contiguous() or row_image.shape[0] < 1:
        raise ValueError(f"{what}: row_image must be a contiguous int32 [R] device tensor with R >= 1")
    return tuple(acts.shape) + (row_image.shape[0],)


def gradcam_weights(acts, jac, dfeat, row_image, mode):
    """Channel weights [R, C] of Grad-CAM (mode GRADCAM: mean of the gradient) or Grad-CAM++ (mode GRADCAM_PLUSPLUS) for R rows
    over the activations acts [N, C, fh, fw] of N images; row_image int32 [R] maps a row to its image (clamped to [0, N - 1] on
    the device).  With dfeat [R, C] the gradient of row r is jac[row_image[r]] * dfeat[r, :, None, None], jac [N, C, fh, fw];
    with dfeat None jac is the gradient itself, [R, C, fh, fw]."""
    N, C, fh, fw, R = _gradcam_dims(acts, row_image, "gradcam_weights")
    if mode not in (GRADCAM, GRADCAM_PLUSPLUS):
        raise ValueError(f"gradcam_weights: mode must be GRADCAM (0) or GRADCAM_PLUSPLUS (1), got {mode!r}")
    _dev_tensor(jac, torch.float32, (N if dfeat is not None else R, C, fh, fw), "gradcam_weights: jac")
    if dfeat is not None:
        _dev_tensor(dfeat, torch.float32, (R, C), "gradcam_weights: dfeat")
    weights = torch.empty((R, C), device=acts.device, dtype=torch.float32)
    call("mmskin_gradcam_weights", ptr(acts), ptr(jac), ptr(dfeat), ptr(row_image), N, R, C, fh, fw, int(mode), ptr(weights), stream())
    return weights


def gradcam_map(acts, weights, row_image, size):
    """(raw [R, fh, fw], cam [R, H, W]): raw[r] = sum_c weights[r, c] * acts[row_image[r], c]; cam[r] = relu(raw[r]) min-max
    normalised over its fh x fw map (+1e-8 in the denominator: a flat map gives zeros), then upsampled bilinearly
    (align_corners=False) to size = (H, W)."""
    N, C, fh, fw, R = _gradcam_dims(acts, row_image, "gradcam_map")
    H, W = int(size[0]), int(size[1])
    _dev_tensor(weights, torch.float32, (R, C), "gradcam_map: weights")
    raw = torch.empty((R, fh, fw), device=acts.device, dtype=torch.float32)
    cam = torch.empty((R, max(H, 0), max(W, 0)), device=acts.device, dtype=torch.float32)
    call("mmskin_gradcam_map", ptr(acts), ptr(weights), ptr(row_image), N, R, C, fh, fw, H, W, ptr(raw), ptr(cam), stream())
    return raw, cam


# ---------------------------------------------------------------------------------------------- CAM faithfulness (forward only)
FAITH_DELETION, FAITH_INSERTION, FAITH_EXPLANATION = 0, 1, 2          # `mode` of a row-table entry of mmskin_faith_perturb
FAITH_MAX_STEPS, FAITH_MAX_KSIZE = 1024, 31


def faith_max_pixels():
    """the largest H * W the rank and perturb kernels take"""
    return int(_lib.load().mmskin_faith_max_pixels())


def gaussian_taps(ksize, sigma):
    """The ksize taps of a Gaussian of standard deviation sigma, computed in fp64, normalised to sum 1, rounded to fp32."""
    ksize = int(ksize)
    if ksize < 1 or ksize % 2 == 0 or ksize > FAITH_MAX_KSIZE:
        raise ValueError(f"gaussian_taps: ksize must be odd and in 1 .. {FAITH_MAX_KSIZE}, got {ksize}")
    if not float(sigma) > 0:
        raise ValueError(f"gaussian_taps: sigma must be > 0, got {sigma}")
    x = np.arange(ksize, dtype=np.float64) - ksize // 2
    w = np.exp(-0.5 * (x / float(sigma)) ** 2)
    return (w / w.sum()).astype(np.float32)


def _faith_saliency(saliency, what):
    _need_gpu(saliency, what)
    if saliency.dim() != 3 or saliency.dtype != torch.float32 or not saliency.is_contiguous() or saliency.shape[0] < 1:
        raise ValueError(f"{what}: the saliency must be a contiguous fp32 [N, H, W] tensor, got {tuple(saliency.shape)} {saliency.dtype}")
    return tuple(saliency.shape)


def faith_rank(saliency, out=None):
    """Rank of every pixel of saliency [N, H, W] within its image -> int32 [N, H, W]: descending saliency, ties by ascending
    row-major index, -0.0 == +0.0, NaN below every number (NaNs tie among themselves)."""
    N, H, W = _faith_saliency(saliency, "faith_rank")
    if out is None:
        out = torch.empty((N, H, W), device=saliency.device, dtype=torch.int32)
    else:
        _dev_tensor(out, torch.int32, (N, H, W), "faith_rank: out")
    call("mmskin_faith_rank", ptr(saliency), N, H * W, ptr(out), stream())
    return out


def _faith_planes(x, what):
    _need_gpu(x, what)
    if x.dim() < 2 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{what}: the input must be a contiguous fp32 [..., H, W] tensor, got {tuple(x.shape)} {x.dtype}")
    H, W = x.shape[-2:]
    return int(x.numel() // max(H * W, 1)), int(H), int(W)


def faith_blur(x, taps, out=None):
    """Separable Gaussian blur with reflect padding of every [H, W] plane of x [..., H, W]; taps: the fp32 numpy array of
    gaussian_taps (horizontal pass, then vertical, ascending taps, every operation rounded to fp32)."""
    planes, H, W = _faith_planes(x, "faith_blur")
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    if taps.ndim != 1:
        raise ValueError(f"faith_blur: taps must be a 1-D array, got shape {taps.shape}")
    if out is None:
        out = torch.empty_like(x)
    else:
        _dev_tensor(out, torch.float32, x.shape, "faith_blur: out")
    call("mmskin_faith_blur", ptr(x), planes, H, W, ctypes.c_void_p(taps.ctypes.data), int(taps.shape[0]), ptr(out), stream())
    return out


def faith_mean(x, out=None):
    """Every [H, W] plane of x [..., H, W] replaced by its mean (fp64 sums in a fixed order, rounded to fp32 once)."""
    planes, H, W = _faith_planes(x, "faith_mean")
    if out is None:
        out = torch.empty_like(x)
    else:
        _dev_tensor(out, torch.float32, x.shape, "faith_mean: out")
    call("mmskin_faith_mean", ptr(x), planes, H * W, ptr(out), stream())
    return out


def faith_perturb(images, baseline, rank, saliency, rows, steps, n, n_pad, out=None):
    """One chunk of model inputs [n_pad, 3, H, W]: row j < n is the image of rows[j] = (image, k, mode), int32 [>= n, 3] on the
    device (FAITH_DELETION: the k * H * W // steps top-ranked pixels come from the baseline; FAITH_INSERTION: only they come
    from the image; FAITH_EXPLANATION: baseline + clamp(saliency, 0, 1) * (image - baseline)); rows n .. n_pad are zeros."""
    N, H, W = _faith_saliency(saliency, "faith_perturb")
    _dev_tensor(images, torch.float32, (N, 3, H, W), "faith_perturb: images")
    _dev_tensor(baseline, torch.float32, (N, 3, H, W), "faith_perturb: baseline")
    _dev_tensor(rank, torch.int32, (N, H, W), "faith_perturb: rank")
    if not torch.is_tensor(rows) or not rows.is_cuda or rows.dtype != torch.int32 or rows.dim() != 2 or rows.shape[1] != 3 \
            or not rows.is_contiguous() or rows.shape[0] < n:
        raise ValueError(f"faith_perturb: rows must be a contiguous int32 [>= {n}, 3] device tensor")
    if out is None:
        out = torch.empty((max(int(n_pad), 0), 3, H, W), device=images.device, dtype=torch.float32)
    else:
        _dev_tensor(out, torch.float32, (n_pad, 3, H, W), "faith_perturb: out")
    call("mmskin_faith_perturb", ptr(images), ptr(baseline), ptr(rank), ptr(saliency), ptr(rows), N, H, W, int(steps), int(n), int(n_pad),
         ptr(out), stream())
    return out


def faith_curves(logits, steps, n_images, target=None):
    """logits fp32 [>= N * (2 S + 3), C], image-major rows (deletion 0 .. S, insertion 0 .. S, explanation); target int32 [N] or
    None = the argmax of every image's deletion step 0 -> (curves [2, N, S + 1], scalars [4, N], means [4], target [N]): fp64
    (target int32); scalars = deletion area, insertion area, average drop, increase."""
    _need_gpu(logits, "faith_curves")
    N, S = int(n_images), int(steps)
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous() or logits.shape[0] < N * (2 * S + 3):
        raise ValueError(f"faith_curves: logits must be a contiguous fp32 [>= {N * (2 * S + 3)}, C] tensor, got {tuple(logits.shape)} "
                         f"{logits.dtype}")
    if target is not None:
        _dev_tensor(target, torch.int32, (N,), "faith_curves: target")
    dev = logits.device
    curves = torch.empty((2, max(N, 0), max(S, 0) + 1), device=dev, dtype=torch.float64)
    scalars = torch.empty((4, max(N, 0)), device=dev, dtype=torch.float64)
    means = torch.empty((4,), device=dev, dtype=torch.float64)
    target_out = torch.empty((max(N, 0),), device=dev, dtype=torch.int32)
    call("mmskin_faith_curves", ptr(logits), ptr(target), N, S, int(logits.shape[1]), ptr(curves), ptr(scalars), ptr(means),
         ptr(target_out), stream())
    return curves, scalars, means, target_out


# ---------------------------------------------------------------------------------------------- RISE saliency (forward only)
RISE_MAX_GRID, RISE_MAX_MASKS = 16, 1 << 20


def _rise_args(seed, grid, p1, what):
    seed, grid, p1 = int(seed), int(grid), float(p1)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"{what}: seed must fit 64 unsigned bits, got {seed}")
    if not 2 <= grid <= RISE_MAX_GRID:
        raise ValueError(f"{what}: grid must be in 2 .. {RISE_MAX_GRID}, got {grid}")
    if not 0.0 < p1 < 1.0:
        raise ValueError(f"{what}: p1 must lie strictly inside (0, 1), got {p1}")
    return seed, grid, p1


def rise_masks(seed, j0, n, grid, p1, H, W, device=None, out=None):
    """Masks j0 .. j0 + n - 1 of (seed, grid, p1) on an H x W image -> fp32 [n, H, W] (the definition: include/mmskin.h).  For
    tests and drawing: RISE itself never materialises a mask."""
    seed, grid, p1 = _rise_args(seed, grid, p1, "rise_masks")
    n, H, W = int(n), int(H), int(W)
    if out is None:
        if device is None or torch.device(device).type != "cuda":
            raise _lib.MMSkinError(f"rise_masks: needs a GPU device, got {device!r}")
        out = torch.empty((max(n, 0), max(H, 0), max(W, 0)), device=device, dtype=torch.float32)
    else:
        _dev_tensor(out, torch.float32, (n, H, W), "rise_masks: out")
    call("mmskin_rise_masks", seed, int(j0), n, grid, p1, H, W, ptr(out), stream())
    return out


def rise_apply(images, baseline, seed, grid, p1, n_masks, r0, n, n_pad, out=None):
    """One chunk of model inputs [n_pad, 3, H, W]: row i < n is baseline + m * (image - baseline) for row r0 + i of the
    image-major row space N * n_masks (image r // n_masks under mask r % n_masks); rows n .. n_pad are zeros."""
    seed, grid, p1 = _rise_args(seed, grid, p1, "rise_apply")
    _need_gpu(images, "rise_apply")
    if images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
        raise ValueError(f"rise_apply: images must be a contiguous fp32 [N, 3, H, W] tensor, got {tuple(images.shape)}")
    N, _, H, W = images.shape
    _dev_tensor(images, torch.float32, (N, 3, H, W), "rise_apply: images")
    _dev_tensor(baseline, torch.float32, (N, 3, H, W), "rise_apply: baseline")
    if out is None:
        out = torch.empty((max(int(n_pad), 0), 3, H, W), device=images.device, dtype=torch.float32)
    else:
        _dev_tensor(out, torch.float32, (n_pad, 3, H, W), "rise_apply: out")
    call("mmskin_rise_apply", ptr(images), ptr(baseline), N, H, W, seed, grid, p1, int(n_masks), int(r0), int(n), int(n_pad), ptr(out),
         stream())
    return out


def rise_accumulate(logits, clean_logits, size, seed, grid, p1, n_masks, target=None, out=None):
    """logits fp32 [>= N * n_masks, K] (image-major rows), clean_logits fp32 [N, K], size = (H, W), target int32 [N] or None =
    the argmax of the clean logits -> (saliency_sum [N, H, W], coverage [H, W], clean_prob [N], target_used int32 [N]): fp64 sums
    over the masks in ascending order, weighted by the soft-max probability of the target class.  out: those four, preallocated."""
    seed, grid, p1 = _rise_args(seed, grid, p1, "rise_accumulate")
    _need_gpu(logits, "rise_accumulate")
    H, W, n_masks = int(size[0]), int(size[1]), int(n_masks)
    if not torch.is_tensor(clean_logits) or clean_logits.dim() != 2 or clean_logits.shape[0] < 1:
        raise ValueError("rise_accumulate: clean_logits must be a contiguous fp32 [N, K] device tensor")
    N, K = clean_logits.shape
    _dev_tensor(clean_logits, torch.float32, (N, K), "rise_accumulate: clean_logits")
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous() or logits.shape[1] != K \
            or logits.shape[0] < N * n_masks:
        raise ValueError(f"rise_accumulate: logits must be a contiguous fp32 [>= {N * n_masks}, {K}] tensor, got {tuple(logits.shape)} "
                         f"{logits.dtype}")
    if target is not None:
        _dev_tensor(target, torch.int32, (N,), "rise_accumulate: target")
    dev = logits.device
    if out is None:
        out = (torch.empty((N, max(H, 0), max(W, 0)), device=dev, dtype=torch.float64),
               torch.empty((max(H, 0), max(W, 0)), device=dev, dtype=torch.float64),
               torch.empty((N,), device=dev, dtype=torch.float64), torch.empty((N,), device=dev, dtype=torch.int32))
    else:
        for t, dtype, shape, name in zip(out, (torch.float64,) * 3 + (torch.int32,), ((N, H, W), (H, W), (N,), (N,)),
                                         ("saliency_sum", "coverage", "clean_prob", "target_used")):
            _dev_tensor(t, dtype, shape, f"rise_accumulate: {name}")
    nbytes = int(_lib.load().mmskin_rise_workspace_bytes(N, n_masks))
    workspace = torch.empty((max(nbytes, 8),), device=dev, dtype=torch.uint8)
    call("mmskin_rise_accumulate", ptr(logits), ptr(target), ptr(clean_logits), N, K, H, W, seed, grid, p1, n_masks, ptr(out[0]),
         ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(workspace), stream())
    return tuple(out)


# ---------------------------------------------------------------------------------------------- metadata sweeps (forward only)
META_NONE, META_CAT_SET, META_CAT_TOGGLE, META_NUM_ADD, META_NUM_SET = 0, 1, 2, 3, 4          # MMSKIN_META_* of mmskin.h
# one record per variant: struct mmskin_meta_variant of include/mmskin.h (32 bytes)
META_VARIANT_DTYPE = np.dtype([("op", "<i4"), ("column", "<i4"), ("a", "<i4"), ("b", "<i4"), ("value", "<f4"), ("reserved", "<u4", (3,))])
assert META_VARIANT_DTYPE.itemsize == 32


def _dev_tensor(t, dtype, shape, what):
    if t is None or not t.is_cuda or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous {str(dtype).replace('torch.', '')} {tuple(shape)} device tensor, got "
                         f"{None if t is None else (t.dtype, tuple(t.shape), str(t.device))}")
    return t


def _encoder_args(what, codes, numeric, col_offset, mean, scale):
    """The encoder's side of a call that encodes rows: codes int32 [B, n_cat] / numeric fp32 [B, n_num] and mean / scale fp32 [n_num]
    on the device, col_offset a HOST int32 array [n_cat + 1] -> (B, n_cat, n_num, the offsets on the host, the offsets on the device)"""
    (B, n_cat), n_num = codes.shape, numeric.shape[1]
    _dev_tensor(codes, torch.int32, (B, n_cat), f"{what}: codes")
    _dev_tensor(numeric, torch.float32, (B, n_num), f"{what}: numeric")
    off_host = np.ascontiguousarray(col_offset, dtype=np.int32)
    if off_host.shape != (n_cat + 1,):
        raise ValueError(f"{what}: col_offset must have {n_cat + 1} entries, got {off_host.shape}")
    if n_num:
        _dev_tensor(mean, torch.float32, (n_num,), f"{what}: mean")
        _dev_tensor(scale, torch.float32, (n_num,), f"{what}: scale")
    return B, n_cat, n_num, off_host, torch.from_numpy(off_host).to(codes.device)


def _logits_arg(what, logits, ndim):
    """The head's logits as the reduce kernels read them: contiguous fp32 or bf16, [V, B, C] or [rows, C]"""
    if logits.dim() != ndim or logits.dtype not in (torch.float32, torch.bfloat16) or not logits.is_contiguous():
        raise ValueError(f"{what}: logits must be a contiguous fp32 or bf16 {'[V, B, C]' if ndim == 3 else '[rows, C]'} tensor, got "
                         f"{logits.dtype} {tuple(logits.shape)}")
    return logits.shape


def metadata_variants(codes, numeric, col_offset, mean, scale, nan_fill, table, out_width, mask=None, missing_code=None, out=None):
    """The V mutated, encoded metadata batches [V, B, out_width] of one batch, in one kernel (mmskin_metadata_variants).
    codes int32 [B, n_cat] and numeric fp32 [B, n_num] on the device; col_offset a HOST int32 array [n_cat + 1]; mean / scale fp32
    [n_num] on the device; table a numpy array of META_VARIANT_DTYPE records (validated by the library); mask uint8
    [V, B, n_cat + n_num] and missing_code int32 [n_cat] on the device, or None."""
    _need_gpu(codes, "metadata_variants")
    table = np.ascontiguousarray(table)
    if table.dtype != META_VARIANT_DTYPE or table.ndim != 1:
        raise ValueError("metadata_variants: table must be a 1-D array of META_VARIANT_DTYPE records")
    V, dev = len(table), codes.device
    B, n_cat, n_num, off_host, off_dev = _encoder_args("metadata_variants", codes, numeric, col_offset, mean, scale)
    if mask is not None:
        _dev_tensor(mask, torch.uint8, (V, B, n_cat + n_num), "metadata_variants: mask")
        if n_cat:
            _dev_tensor(missing_code, torch.int32, (n_cat,), "metadata_variants: missing_code")
    out_width = int(out_width)
    if out is None:
        out = torch.empty((V, B, max(out_width, 0)), device=dev, dtype=torch.float32)
    else:
        _dev_tensor(out, torch.float32, (V, B, out_width), "metadata_variants: out")
    scratch = torch.empty(max(table.nbytes, 1), dtype=torch.uint8, device=dev)      # the library uploads the table into it
    call("mmskin_metadata_variants", ptr(codes), n_cat, ptr(off_dev), ctypes.c_void_p(off_host.ctypes.data), int(off_host[-1]),
         ptr(numeric), n_num, ptr(mean) if n_num else None, ptr(scale) if n_num else None, float(nan_fill),
         ctypes.c_void_p(table.ctypes.data), ptr(scratch), V, ptr(mask), ptr(missing_code) if mask is not None and n_cat else None,
         ptr(out), B, out_width, stream())
    return out


def sweep_reduce(logits, base, flips, transitions, confusion=None, labels=None, want_probs=True):
    """logits [V, B, C] (fp32 or bf16) against the baseline logits base fp32 [B, C] -> (probs or None, pred, margin, stats) per
    (v, b); the flip / transition (/ confusion, with labels int32 [B]) counts are ADDED to the int32 device counters flips [V],
    transitions [V, C, C], confusion [V, C, C] (mmskin_sweep_reduce)."""
    _need_gpu(logits, "sweep_reduce")
    V, B, C = _logits_arg("sweep_reduce", logits, 3)
    dev = logits.device
    _dev_tensor(base, torch.float32, (B, C), "sweep_reduce: base")
    _dev_tensor(flips, torch.int32, (V,), "sweep_reduce: flips")
    _dev_tensor(transitions, torch.int32, (V, C, C), "sweep_reduce: transitions")
    if labels is not None:
        _dev_tensor(labels, torch.int32, (B,), "sweep_reduce: labels")
        _dev_tensor(confusion, torch.int32, (V, C, C), "sweep_reduce: confusion")
    probs = torch.empty((V, B, C), device=dev, dtype=torch.float32) if want_probs else None
    pred = torch.empty((V, B), device=dev, dtype=torch.int32)
    margin = torch.empty((V, B), device=dev, dtype=torch.float32)
    stats = torch.empty((V, B, 4), device=dev, dtype=torch.float32)
    call("mmskin_sweep_reduce", ptr(logits), _dtype_code(logits), ptr(base), ptr(labels), V, B, C, ptr(probs), ptr(pred), ptr(margin),
         ptr(stats), ptr(flips), ptr(transitions), ptr(confusion) if labels is not None else None, stream())
    return probs, pred, margin, stats


# ---------------------------------------------------------------------------------------------- metadata Shapley values (forward only)
SHAPLEY_PROB, SHAPLEY_LOGIT = 0, 1                                                           # MMSKIN_SHAPLEY_* of mmskin.h


def shapley_rows(batch, G, P, M):
    """Rows of a batch's coalition walk, batch * (1 + G + P * 2 * (M - 1) * G), in the row order of include/mmskin.h."""
    n = int(_lib.load().mmskin_shapley_rows(int(batch), int(G), int(P), int(M)))
    if n < 0:
        raise ValueError(f"shapley_rows: batch {batch}, G {G}, P {P}, M {M}: an extent is < 1 or the walk is out of range")
    return n


def _shapley_table(perms, M, what):
    perms = np.ascontiguousarray(perms)
    if perms.dtype != np.int32 or perms.ndim != 2 or perms.shape[1] != M:
        raise ValueError(f"{what}: perms must be an int32 [P, {M}] table, got {perms.dtype} {perms.shape}")
    return perms


def shapley_coalitions(codes, numeric, bg_codes, bg_numeric, col_offset, mean, scale, nan_fill, perms, out_width, row0=0, row1=None,
                       out=None):
    """The encoded metadata rows [row1 - row0, out_width] of rows [row0, row1) of a batch's coalition walk, in one kernel
    (mmskin_shapley_coalitions).  codes int32 [B, n_cat] / numeric fp32 [B, n_num] of the explained rows and bg_codes [G, n_cat] /
    bg_numeric [G, n_num] of the background on the device; col_offset a HOST int32 array [n_cat + 1]; mean / scale fp32 [n_num] on
    the device; perms a HOST int32 [P, M] table of permutations (validated by the library)."""
    _need_gpu(codes, "shapley_coalitions")
    G, dev = bg_codes.shape[0], codes.device
    perms = _shapley_table(perms, codes.shape[1] + numeric.shape[1], "shapley_coalitions")
    B, n_cat, n_num, off_host, off_dev = _encoder_args("shapley_coalitions", codes, numeric, col_offset, mean, scale)
    _dev_tensor(bg_codes, torch.int32, (G, n_cat), "shapley_coalitions: bg_codes")
    _dev_tensor(bg_numeric, torch.float32, (G, n_num), "shapley_coalitions: bg_numeric")
    P, out_width, row0 = len(perms), int(out_width), int(row0)
    row1 = shapley_rows(B, G, P, n_cat + n_num) if row1 is None else int(row1)
    if out is None:
        out = torch.empty((max(row1 - row0, 0), max(out_width, 0)), device=dev, dtype=torch.float32)
    else:
        _dev_tensor(out, torch.float32, (row1 - row0, out_width), "shapley_coalitions: out")
    scratch = torch.empty(max(perms.size, 1), dtype=torch.int32, device=dev)          # the library uploads the inverse table into it
    call("mmskin_shapley_coalitions", ptr(codes), ptr(numeric), B, ptr(bg_codes), ptr(bg_numeric), G, n_cat, ptr(off_dev),
         ctypes.c_void_p(off_host.ctypes.data), int(off_host[-1]), n_num, ptr(mean) if n_num else None, ptr(scale) if n_num else None,
         float(nan_fill), ctypes.c_void_p(perms.ctypes.data), ptr(scratch), P, row0, row1, ptr(out), out_width, stream())
    return out


def shapley_reduce(logits, v, perms, G, row0, output=SHAPLEY_PROB, finish=False, abs_sum=None):
    """logits [rows, C] (fp32 or bf16) of rows [row0, row0 + rows) of the walk -> the coalition means into v fp64 [B, K + 2, C]
    (K = 2 P (M - 1); mmskin_shapley_reduce).  The range is cut at multiples of G.  With finish, on the call that completes v:
    returns (phi fp32 [B, M, C], base [B, C] = v(empty), full [B, C] = v(all)) and ADDS sum_b |phi| into abs_sum fp64 [M, C] when
    that is given; otherwise returns None."""
    _need_gpu(logits, "shapley_reduce")
    rows, C = _logits_arg("shapley_reduce", logits, 2)
    perms = np.ascontiguousarray(perms)
    if perms.dtype != np.int32 or perms.ndim != 2:
        raise ValueError(f"shapley_reduce: perms must be an int32 [P, M] table, got {perms.dtype} {perms.shape}")
    (P, M), dev = perms.shape, logits.device
    if v is None or v.dim() != 3:
        raise ValueError("shapley_reduce: v must be a float64 [B, K + 2, C] device tensor")
    B = v.shape[0]
    _dev_tensor(v, torch.float64, (B, 2 * P * (M - 1) + 2, C), "shapley_reduce: v")
    phi = base = full = scratch = None
    if finish:
        phi = torch.empty((B, M, C), device=dev, dtype=torch.float32)
        base, full = torch.empty((B, C), device=dev, dtype=torch.float32), torch.empty((B, C), device=dev, dtype=torch.float32)
        scratch = torch.empty(max(perms.size, 1), dtype=torch.int32, device=dev)
        if abs_sum is not None:
            _dev_tensor(abs_sum, torch.float64, (M, C), "shapley_reduce: abs_sum")
    call("mmskin_shapley_reduce", ptr(logits), _dtype_code(logits), int(output), B, int(G), P, M, C, int(row0), int(row0) + rows, ptr(v),
         int(bool(finish)), ctypes.c_void_p(perms.ctypes.data), ptr(scratch), ptr(phi), ptr(base), ptr(full),
         ptr(abs_sum) if finish else None, stream())
    return (phi, base, full) if finish else None


# ---------------------------------------------------------------------------------------------- metadata LIME (forward only)
LIME_PROB, LIME_LOGIT = 0, 1                                                                 # MMSKIN_LIME_* of mmskin.h
LIME_MAX_FEATURES = 128


def _lime_stats(mean, scale, F, what):
    _dev_tensor(mean, torch.float64, (F,), f"{what}: mean")
    _dev_tensor(scale, torch.float64, (F,), f"{what}: scale")


def _lime_weight_code(w, what):
    if w.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: the weights must be fp32 or fp64, got {w.dtype}")
    return int(w.dtype == torch.float64)                                                     # MMSKIN_LIME_W_F32 / _F64


def lime_accumulator(batch, N, F, C, device):
    """The zeroed fp64 accumulator lime_reduce adds into and lime_solve reads (mmskin_lime_accumulator_doubles)."""
    n = int(_lib.load().mmskin_lime_accumulator_doubles(int(batch), int(N), int(F), int(C)))
    if n < 0:
        raise ValueError(f"lime_accumulator: batch {batch}, N {N}, F {F}, C {C}: an extent is < 1 or out of range (F <= {LIME_MAX_FEATURES}, "
                         "C <= 64)")
    return torch.zeros(n, dtype=torch.float64, device=device)


def lime_neighbourhood(x, mean, scale, N, seed, out_width=None, row0=0, row1=None, sample0=0, around_instance=False, out=None,
                       weights=None, weight_dtype=torch.float64):
    """Rows [row0, row1) of the B * N neighbourhood rows of x fp32 [B, >= F] (sample-major; row 0 of a sample is x itself, the
    others counter-based normal draws of (seed, sample0 + b, s, f) scaled by mean / scale fp64 [F]) and their LIME kernel weights:
    (rows fp32 [row1 - row0, out_width], weights [row1 - row0]) (mmskin_lime_neighbourhood)."""
    _need_gpu(x, "lime_neighbourhood")
    F = int(mean.shape[0]) if mean is not None and mean.dim() == 1 else -1
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1 or x.shape[1] < F:
        raise ValueError(f"lime_neighbourhood: x must be fp32 [B, >= {F}] with unit column stride, got {x.dtype} {tuple(x.shape)}")
    _lime_stats(mean, scale, F, "lime_neighbourhood")
    B, N, row0 = int(x.shape[0]), int(N), int(row0)
    row1 = B * N if row1 is None else int(row1)
    out_width = F if out_width is None else int(out_width)
    n = max(row1 - row0, 0)
    if out is None:
        out = torch.empty((n, max(out_width, 0)), device=x.device, dtype=torch.float32)
    else:
        _dev_tensor(out, torch.float32, (row1 - row0, out_width), "lime_neighbourhood: out")
    if weights is None:
        weights = torch.empty((n,), device=x.device, dtype=weight_dtype)
    code = _lime_weight_code(weights, "lime_neighbourhood")
    _dev_tensor(weights, weights.dtype, (row1 - row0,), "lime_neighbourhood: weights")
    call("mmskin_lime_neighbourhood", ptr(x), int(x.stride(0)), B, ptr(mean), ptr(scale), F, N, int(seed) & (2 ** 64 - 1), int(sample0),
         int(bool(around_instance)), row0, row1, ptr(out), out_width, ptr(weights), code, stream())
    return out, weights


def lime_reduce(rows, weights, logits, mean, scale, acc, batch, N, row0, output=LIME_PROB):
    """Adds rows [row0, row0 + n) of a batch's neighbourhood -- the rows fp32 [n, >= F], their weights [n] and the head's logits
    [n, C] (fp32 or bf16) -- into acc (lime_accumulator): every weighted sum the ridge fits need (mmskin_lime_reduce)."""
    _need_gpu(logits, "lime_reduce")
    n, C = _logits_arg("lime_reduce", logits, 2)
    F = int(mean.shape[0]) if mean is not None and mean.dim() == 1 else -1
    _lime_stats(mean, scale, F, "lime_reduce")
    if rows is None or rows.dim() != 2:
        raise ValueError("lime_reduce: rows must be an fp32 [rows, width] device tensor")
    _dev_tensor(rows, torch.float32, (n, rows.shape[1]), "lime_reduce: rows")
    code = _lime_weight_code(weights, "lime_reduce")
    _dev_tensor(weights, weights.dtype, (n,), "lime_reduce: weights")
    want = int(_lib.load().mmskin_lime_accumulator_doubles(int(batch), int(N), F, int(C)))
    _dev_tensor(acc, torch.float64, (max(want, 0),), "lime_reduce: acc")
    call("mmskin_lime_reduce", ptr(rows), int(rows.shape[1]), ptr(weights), code, ptr(logits), _dtype_code(logits), int(output), ptr(mean),
         ptr(scale), int(batch), int(N), F, int(C), int(row0), int(row0) + int(n), ptr(acc), stream())


def lime_solve(acc, x, mean, scale, N, C, num_features, want_dense=True, abs_sum=None):
    """The ridge fits of every (sample, class) from the sums in acc: (coef fp64 [B, C, K], feature int32 [B, C, K] in descending
    |coef|, intercept, score, local_pred fp64 [B, C], dense fp64 [B, C, F] or None); ADDS sum_b |coef| into abs_sum fp64 [F, C] when
    given.  Waits for the stream; a factorisation that fails raises MMSkinError (mmskin_lime_solve)."""
    _need_gpu(x, "lime_solve")
    F = int(mean.shape[0]) if mean is not None and mean.dim() == 1 else -1
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1 or x.shape[1] < F:
        raise ValueError(f"lime_solve: x must be fp32 [B, >= {F}] with unit column stride, got {x.dtype} {tuple(x.shape)}")
    _lime_stats(mean, scale, F, "lime_solve")
    B, C, K, dev = int(x.shape[0]), int(C), int(num_features), x.device
    want = int(_lib.load().mmskin_lime_accumulator_doubles(B, int(N), F, C))
    _dev_tensor(acc, torch.float64, (max(want, 0),), "lime_solve: acc")
    if abs_sum is not None:
        _dev_tensor(abs_sum, torch.float64, (F, C), "lime_solve: abs_sum")
    k = max(K, 0)
    coef = torch.empty((B, C, k), dtype=torch.float64, device=dev)
    feature = torch.empty((B, C, k), dtype=torch.int32, device=dev)
    intercept, score, local_pred = (torch.empty((B, C), dtype=torch.float64, device=dev) for _ in range(3))
    dense = torch.empty((B, C, F), dtype=torch.float64, device=dev) if want_dense else None
    nbytes = int(_lib.load().mmskin_lime_solve_workspace_bytes(B, F, C))
    workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    call("mmskin_lime_solve", ptr(acc), ptr(x), int(x.stride(0)), ptr(mean), ptr(scale), B, int(N), F, C, K, ptr(coef), ptr(feature),
         ptr(intercept), ptr(score), ptr(local_pred), ptr(dense), ptr(abs_sum), ptr(workspace), stream())
    return coef, feature, intercept, score, local_pred, dense


# ---------------------------------------------------------------------------------------------- metadata permutation importance (forward only)
PERMUTATION_MAX_SAMPLES = 4096                                                               # MMSKIN_PERMUTATION_MAX_SAMPLES of mmskin.h
PERMUTATION_METRICS = ("accuracy", "balanced_accuracy", "auc")                               # the order of every [3, ...] output


def permutation_indices(seed, R, G, S, device):
    """perm int32 [R, G, S]: per (repeat, group) the argsort of the counter-based keys of (seed, r, g, position)
    (mmskin_permutation_indices)."""
    if not torch.cuda.is_available():
        raise _lib.MMSkinError("permutation_indices needs a HIP device; there is no CPU fallback")
    R, G, S = int(R), int(G), int(S)
    perm = torch.empty((max(R, 0), max(G, 0), max(S, 0)), dtype=torch.int32, device=device)
    call("mmskin_permutation_indices", int(seed) & (2 ** 64 - 1), R, G, S, ptr(perm), stream())
    return perm


def permuted_rows(x, group, perm, row0=0, row1=None, out=None):
    """Rows [row0, row1) of the study, fp32 [row1 - row0, width]: row (r G + g) S + s is x[s] with the columns j of group[j] == g
    taken from x[perm[r, g, s]] (mmskin_permuted_rows).  x fp32 [S, width] with unit column stride, group int32 [width] (-1: never
    shuffled), perm int32 [R, G, S], all on the device."""
    _need_gpu(x, "permuted_rows")
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1:
        raise ValueError(f"permuted_rows: x must be fp32 [S, width] with unit column stride, got {x.dtype} {tuple(x.shape)}")
    S, width = x.shape
    if perm is None or perm.dim() != 3:
        raise ValueError("permuted_rows: perm must be an int32 [R, G, S] device tensor")
    R, G = perm.shape[:2]
    _dev_tensor(perm, torch.int32, (R, G, S), "permuted_rows: perm")
    _dev_tensor(group, torch.int32, (width,), "permuted_rows: group")
    row0 = int(row0)
    row1 = R * G * S if row1 is None else int(row1)
    if out is None:
        out = torch.empty((max(row1 - row0, 0), width), device=x.device, dtype=torch.float32)
    else:
        _dev_tensor(out, torch.float32, (row1 - row0, width), "permuted_rows: out")
    call("mmskin_permuted_rows", ptr(x), int(x.stride(0)), ptr(group), ptr(perm), R, G, S, width, row0, row1, ptr(out), stream())
    return out


def permutation_accumulators(R, G, K, device):
    """(confusion int32 [R, G, K, K], counts int64 [R, G, 3 K + 1]) for permutation_scores to fill."""
    return (torch.zeros((R, G, K, K), dtype=torch.int32, device=device), torch.zeros((R, G, 3 * K + 1), dtype=torch.int64, device=device))


def permutation_scores(logits, labels, confusion, counts, row0):
    """The cells of rows [row0, row0 + n) of the study -- n and row0 multiples of S -- scored from their logits fp32 [n, K]: the
    confusion counts and the one-vs-rest AUC integers of each cell are written into confusion / counts
    (permutation_accumulators; mmskin_permutation_scores).  labels int64 [S]."""
    _need_gpu(logits, "permutation_scores")
    if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError(f"permutation_scores: logits must be a contiguous fp32 [rows, K] tensor, got {logits.dtype} {tuple(logits.shape)}")
    n, K = logits.shape
    if confusion is None or confusion.dim() != 4:
        raise ValueError("permutation_scores: confusion must be an int32 [R, G, K, K] device tensor")
    R, G = confusion.shape[:2]
    _dev_tensor(confusion, torch.int32, (R, G, K, K), "permutation_scores: confusion")
    _dev_tensor(counts, torch.int64, (R, G, 3 * K + 1), "permutation_scores: counts")
    if labels is None or labels.dim() != 1:
        raise ValueError("permutation_scores: labels must be an int64 [S] device tensor")
    S = labels.shape[0]
    _dev_tensor(labels, torch.int64, (S,), "permutation_scores: labels")
    call("mmskin_permutation_scores", ptr(logits), ptr(labels), R, G, S, K, int(row0), int(row0) + n, ptr(confusion), ptr(counts), stream())


def permutation_finalize(confusion, counts, baseline):
    """(metrics, importances fp64 [3, G, R], mean, std fp64 [3, G]) from the filled accumulators and baseline fp64 [3] on the
    device; the first axis is PERMUTATION_METRICS (mmskin_permutation_finalize)."""
    _need_gpu(confusion, "permutation_finalize")
    if confusion.dim() != 4:
        raise ValueError("permutation_finalize: confusion must be an int32 [R, G, K, K] device tensor")
    R, G, K = confusion.shape[:3]
    _dev_tensor(confusion, torch.int32, (R, G, K, K), "permutation_finalize: confusion")
    _dev_tensor(counts, torch.int64, (R, G, 3 * K + 1), "permutation_finalize: counts")
    _dev_tensor(baseline, torch.float64, (3,), "permutation_finalize: baseline")
    dev = confusion.device
    metrics, importances = (torch.empty((3, G, R), dtype=torch.float64, device=dev) for _ in range(2))
    mean, std = (torch.empty((3, G), dtype=torch.float64, device=dev) for _ in range(2))
    call("mmskin_permutation_finalize", ptr(confusion), ptr(counts), ptr(baseline), R, G, K, ptr(metrics), ptr(importances), ptr(mean),
         ptr(std), stream())
    return metrics, importances, mean, std


# ---------------------------------------------------------------------------------------------- bootstrap intervals of a fold's metrics
BOOTSTRAP_MAX_ROWS = 16384                                                                   # MMSKIN_BOOTSTRAP_MAX_* of mmskin.h
BOOTSTRAP_MAX_CLASSES = 64
BOOTSTRAP_MAX_RESAMPLES = 8192
BOOTSTRAP_PLAIN, BOOTSTRAP_STRATIFIED, BOOTSTRAP_POINT = 0, 1, 2                             # MMSKIN_BOOTSTRAP_PLAIN ...
BOOTSTRAP_METRICS = ("accuracy", "balanced_accuracy", "precision", "recall", "f1_score", "auc", "macro_auc")   # columns 0 .. 6
BOOTSTRAP_CLASS_METRICS = ("per_class_recall", "per_class_auc")                              # columns 7 .. 7 + K and 7 + K .. 7 + 2 K
BOOTSTRAP_SUMMARY = ("n_valid", "mean", "std", "low", "high")                                # the rows of a summary


def bootstrap_check_limits(what, N=None, K=None, B=None):
    """MMSkinError naming the limit that a row, class or replicate count breaks (the C entry points check the same)"""
    if N is not None and not 1 <= N <= BOOTSTRAP_MAX_ROWS:
        raise _lib.MMSkinError(f"{what}: {N} rows; a replicate's weights live in LDS, which holds 1 .. BOOTSTRAP_MAX_ROWS = {BOOTSTRAP_MAX_ROWS}")
    if K is not None and not 2 <= K <= BOOTSTRAP_MAX_CLASSES:
        raise _lib.MMSkinError(f"{what}: {K} classes; the kernels hold 2 .. BOOTSTRAP_MAX_CLASSES = {BOOTSTRAP_MAX_CLASSES}")
    if B is not None and not 1 <= B <= BOOTSTRAP_MAX_RESAMPLES:
        raise _lib.MMSkinError(f"{what}: {B} replicates; a metric column is sorted in LDS, which holds 1 .. BOOTSTRAP_MAX_RESAMPLES = "
                               f"{BOOTSTRAP_MAX_RESAMPLES}")


def bootstrap_quantiles(confidence):
    """the two quantiles of the percentile interval, as numpy forms them from the percentiles 100 a / 2 and 100 (1 - a / 2)"""
    a = 1.0 - float(confidence)
    return float(np.true_divide(100.0 * a / 2.0, 100)), float(np.true_divide(100.0 * (1.0 - a / 2.0), 100))


def bootstrap_tables(scores, labels, preds=None):
    """The per-call tables of a fold (mmskin.h): scores fp32 [N, K] and labels integer [N] in [0, K) on the device (no NaN, no label
    outside: the caller has dropped those rows), preds integer [N] or None for the first arg-max of each row.  Returns a dict:
    labels, preds int64 [N]; order, lo, hi int32 [K, N] (per class the rows in ascending order of their score, and each position's
    tie group); members int32 [N], class_start int32 [K + 1] (the rows grouped by label); N, K.  A device sort, not a kernel of ours:
    this runs once per call."""
    _need_gpu(scores, "bootstrap_tables")
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError(f"bootstrap_tables: scores must be an fp32 [N, K] tensor, got {scores.dtype} {tuple(scores.shape)}")
    N, K = scores.shape
    bootstrap_check_limits("bootstrap_tables", N=N, K=K)
    dev = scores.device
    if labels is None or tuple(labels.shape) != (N,) or labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.device != dev:
        raise ValueError(f"bootstrap_tables: labels must be an integer {(N,)} tensor on {dev}")
    labels = labels.detach().long().contiguous()
    if preds is None:
        preds = scores.argmax(dim=1)
    elif tuple(preds.shape) != (N,) or preds.dtype.is_floating_point or preds.dtype == torch.bool or preds.device != dev:
        raise ValueError(f"bootstrap_tables: preds must be an integer {(N,)} tensor on {dev}")
    preds = preds.detach().long().contiguous()
    vals, order = torch.sort(scores.detach().t().contiguous(), dim=1, stable=True)           # [K, N]
    at = torch.arange(N, device=dev, dtype=torch.int64).expand(K, N)
    edge = torch.ones((K, 1), dtype=torch.bool, device=dev)
    differs = vals[:, 1:] != vals[:, :-1]                                                    # position q + 1 opens a new tie group
    lo = torch.cummax(torch.where(torch.cat([edge, differs], dim=1), at, torch.zeros_like(at)), dim=1).values
    ends = torch.where(torch.cat([differs, edge], dim=1), at + 1, torch.full_like(at, N))
    hi = torch.cummin(ends.flip(1), dim=1).values.flip(1)
    members = torch.sort(labels, stable=True).indices
    class_start = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    class_start[1:] = torch.cumsum(torch.bincount(labels.clamp(0, K - 1), minlength=K), dim=0)
    i32 = lambda t: t.to(torch.int32).contiguous()
    return {"labels": labels, "preds": preds, "order": i32(order), "lo": i32(lo), "hi": i32(hi), "members": i32(members),
            "class_start": i32(class_start), "N": int(N), "K": int(K)}


def _bootstrap_range(B, b0, b1):
    b0 = int(b0)
    return b0, (B if b1 is None else int(b1))


def bootstrap_weights(seed, n_rows, n_resamples, device=None, b0=0, b1=None, tables=None):
    """w int32 [b1 - b0, N]: how often each row is drawn in the replicates [b0, b1) of a study of `n_resamples`
    (mmskin_bootstrap_weights).  Plain resampling needs no table; with `tables` (bootstrap_tables) the draws are stratified by
    label.  The weights depend on (seed, replicate, N) -- stratified: and the labels -- only."""
    N, B = int(n_rows), int(n_resamples)
    K = 2 if tables is None else tables["K"]
    bootstrap_check_limits("bootstrap_weights", N=N, K=K, B=B)
    if tables is not None and tables["N"] != N:
        raise ValueError(f"bootstrap_weights: the tables hold {tables['N']} rows, n_rows is {N}")
    b0, b1 = _bootstrap_range(B, b0, b1)
    if not torch.cuda.is_available():
        raise _lib.MMSkinError("bootstrap_weights needs a HIP device; there is no CPU fallback")
    dev = tables["labels"].device if tables is not None else (torch.device("cuda") if device is None else torch.device(device))
    with torch.cuda.device(dev):
        w = torch.empty((max(b1 - b0, 0), N), dtype=torch.int32, device=dev)
        if tables is None:
            call("mmskin_bootstrap_weights", int(seed) & (2 ** 64 - 1), BOOTSTRAP_PLAIN, N, K, B, None, None, None, b0, b1, ptr(w), stream())
        else:
            call("mmskin_bootstrap_weights", int(seed) & (2 ** 64 - 1), BOOTSTRAP_STRATIFIED, N, K, B, ptr(tables["labels"]),
                 ptr(tables["members"]), ptr(tables["class_start"]), b0, b1, ptr(w), stream())
    return w


def bootstrap_accumulators(B, K, device, fill=0):
    """(confusion int32 [B, K, K], counts int64 [B, 3 K]) for bootstrap_replicates to fill"""
    bootstrap_check_limits("bootstrap_accumulators", K=int(K), B=int(B))
    return (torch.full((B, K, K), fill, dtype=torch.int32, device=device), torch.full((B, 3 * K), fill, dtype=torch.int64, device=device))


def bootstrap_replicates(tables, seed, mode, confusion, counts, b0=0, b1=None):
    """The integers of replicates [b0, b1) written into their slices of confusion int32 [B, K, K] and counts int64 [B, 3 K] (pos,
    neg, wins2), one workgroup per replicate (mmskin_bootstrap_replicates).  mode: BOOTSTRAP_PLAIN, BOOTSTRAP_STRATIFIED, or
    BOOTSTRAP_POINT for the fold itself (all weights 1)."""
    N, K = tables["N"], tables["K"]
    _need_gpu(tables["labels"], "bootstrap_replicates")
    if confusion is None or confusion.dim() != 3:
        raise ValueError("bootstrap_replicates: confusion must be an int32 [B, K, K] device tensor")
    B = confusion.shape[0]
    bootstrap_check_limits("bootstrap_replicates", N=N, K=K, B=B)
    _dev_tensor(confusion, torch.int32, (B, K, K), "bootstrap_replicates: confusion")
    _dev_tensor(counts, torch.int64, (B, 3 * K), "bootstrap_replicates: counts")
    b0, b1 = _bootstrap_range(B, b0, b1)
    call("mmskin_bootstrap_replicates", int(seed) & (2 ** 64 - 1), int(mode), N, K, B, ptr(tables["labels"]), ptr(tables["preds"]),
         ptr(tables["members"]), ptr(tables["class_start"]), ptr(tables["order"]), ptr(tables["lo"]), ptr(tables["hi"]), b0, b1, ptr(confusion),
         ptr(counts), stream())


def bootstrap_finalize(confusion, counts, confidence=0.95):
    """(metrics fp64 [7 + 2 K, B], summary fp64 [5, 7 + 2 K]) on the device from the filled accumulators: the metric columns in the
    order BOOTSTRAP_METRICS, then K per-class recalls, then K per-class AUCs; the summary rows are BOOTSTRAP_SUMMARY
    (mmskin_bootstrap_finalize)."""
    _need_gpu(confusion, "bootstrap_finalize")
    if confusion.dim() != 3:
        raise ValueError("bootstrap_finalize: confusion must be an int32 [B, K, K] device tensor")
    B, K = confusion.shape[:2]
    bootstrap_check_limits("bootstrap_finalize", K=K, B=B)
    _dev_tensor(confusion, torch.int32, (B, K, K), "bootstrap_finalize: confusion")
    _dev_tensor(counts, torch.int64, (B, 3 * K), "bootstrap_finalize: counts")
    q_lo, q_hi = bootstrap_quantiles(confidence)
    M = 7 + 2 * K
    metrics = torch.empty((M, B), dtype=torch.float64, device=confusion.device)
    summary = torch.empty((5, M), dtype=torch.float64, device=confusion.device)
    call("mmskin_bootstrap_finalize", ptr(confusion), ptr(counts), B, K, q_lo, q_hi, ptr(metrics), ptr(summary), stream())
    return metrics, summary


def bootstrap_compare(metrics_a, metrics_b, confidence=0.95):
    """(delta fp64 [M, B] = a - b, summary fp64 [5, M] of delta, sign_counts int64 [M, 2] = the replicates with delta <= 0 and with
    delta >= 0) from two metric tables of bootstrap_finalize made with one seed (mmskin_bootstrap_compare)."""
    _need_gpu(metrics_a, "bootstrap_compare")
    if metrics_a.dim() != 2:
        raise ValueError("bootstrap_compare: the metric tables must be fp64 [M, B] device tensors")
    M, B = metrics_a.shape
    bootstrap_check_limits("bootstrap_compare", B=B)
    _dev_tensor(metrics_a, torch.float64, (M, B), "bootstrap_compare: metrics_a")
    _dev_tensor(metrics_b, torch.float64, (M, B), "bootstrap_compare: metrics_b")
    q_lo, q_hi = bootstrap_quantiles(confidence)
    dev = metrics_a.device
    delta = torch.empty((M, B), dtype=torch.float64, device=dev)
    summary = torch.empty((5, M), dtype=torch.float64, device=dev)
    sign_counts = torch.empty((M, 2), dtype=torch.int64, device=dev)
    call("mmskin_bootstrap_compare", ptr(metrics_a), ptr(metrics_b), B, M, q_lo, q_hi, ptr(delta), ptr(summary), ptr(sign_counts), stream())
    return delta, summary, sign_counts


# ---------------------------------------------------------------------------------------------- subgroup audit of a fold
SUBGROUP_MAX_ROWS = 8192                                                                     # MMSKIN_SUBGROUP_MAX_* of mmskin.h
SUBGROUP_MAX_GROUPS = 64
SUBGROUP_MAX_CELLS = 16384                                                                   # G K K
SUBGROUP_CLASS_METRICS = BOOTSTRAP_CLASS_METRICS + ("per_class_fpr", "per_class_predicted_rate")   # columns 7 + j K .. 7 + (j + 1) K
SUBGROUP_GAPS = ("lowest", "highest", "gap")                                                 # the blocks of a gap summary


def subgroup_metric_columns(K):
    return 7 + 4 * int(K)


def subgroup_check_limits(what, N=None, K=None, G=None, B=None):
    """MMSkinError naming the limit that a row, class, group or replicate count breaks (the C entry points check the same)"""
    if N is not None and not 1 <= N <= SUBGROUP_MAX_ROWS:
        raise _lib.MMSkinError(f"{what}: {N} rows; a replicate's weights live in LDS, which holds 1 .. SUBGROUP_MAX_ROWS = {SUBGROUP_MAX_ROWS}")
    bootstrap_check_limits(what, K=K, B=B)
    if G is not None and not 1 <= G <= SUBGROUP_MAX_GROUPS:
        raise _lib.MMSkinError(f"{what}: {G} groups; a row's group is a byte in LDS, which holds 1 .. SUBGROUP_MAX_GROUPS = {SUBGROUP_MAX_GROUPS}")
    if G is not None and K is not None and G * K * K > SUBGROUP_MAX_CELLS:
        raise _lib.MMSkinError(f"{what}: {G} groups of {K} classes are {G * K * K} confusion cells; LDS holds G K K <= SUBGROUP_MAX_CELLS = "
                               f"{SUBGROUP_MAX_CELLS}")


def subgroup_tables(scores, labels, groups, n_groups, preds=None):
    """The per-call tables of a grouped fold (mmskin.h): scores, labels and preds as for bootstrap_tables, groups integer [N] on the
    same device (an id outside [0, n_groups) puts the row in no group).  Returns bootstrap_tables' dict with order, lo, hi int32
    [K, N] taken over (group, score) -- per class the rows in ascending order of their group, then their score; a tie group ends
    where the group does -- plus groups int32 [N], group_start int32 [G + 1] and G.  Device sorts, once per call."""
    _need_gpu(scores, "subgroup_tables")
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError(f"subgroup_tables: scores must be an fp32 [N, K] tensor, got {scores.dtype} {tuple(scores.shape)}")
    N, K = scores.shape
    G = int(n_groups)
    subgroup_check_limits("subgroup_tables", N=N, K=K, G=G)
    dev = scores.device
    for name, t in (("labels", labels), ("groups", groups)) + ((("preds", preds),) if preds is not None else ()):
        if t is None or tuple(t.shape) != (N,) or t.dtype.is_floating_point or t.dtype == torch.bool or t.device != dev:
            raise ValueError(f"subgroup_tables: {name} must be an integer {(N,)} tensor on {dev}")
    labels = labels.detach().long().contiguous()
    preds = (scores.argmax(dim=1) if preds is None else preds.detach()).long().contiguous()
    groups = groups.detach().long()
    key = torch.where((groups >= 0) & (groups < G), groups, torch.full_like(groups, G))      # [N] in 0 .. G
    vals, order = torch.sort(scores.detach().t().contiguous(), dim=1, stable=True)           # [K, N] by score ...
    by_group = torch.sort(key[order], dim=1, stable=True)                                    # ... then, stably, by group
    order, vals, keys = torch.gather(order, 1, by_group.indices), torch.gather(vals, 1, by_group.indices), by_group.values
    at = torch.arange(N, device=dev, dtype=torch.int64).expand(K, N)
    edge = torch.ones((K, 1), dtype=torch.bool, device=dev)
    differs = (vals[:, 1:] != vals[:, :-1]) | (keys[:, 1:] != keys[:, :-1])                  # position q + 1 opens a new tie group
    lo = torch.cummax(torch.where(torch.cat([edge, differs], dim=1), at, torch.zeros_like(at)), dim=1).values
    ends = torch.where(torch.cat([differs, edge], dim=1), at + 1, torch.full_like(at, N))
    hi = torch.cummin(ends.flip(1), dim=1).values.flip(1)
    group_start = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    group_start[1:] = torch.cumsum(torch.bincount(key, minlength=G + 1)[:G], dim=0)
    members = torch.sort(labels, stable=True).indices
    class_start = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    class_start[1:] = torch.cumsum(torch.bincount(labels.clamp(0, K - 1), minlength=K), dim=0)
    i32 = lambda t: t.to(torch.int32).contiguous()
    return {"labels": labels, "preds": preds, "groups": i32(groups.clamp(-1, G)), "order": i32(order), "lo": i32(lo), "hi": i32(hi),
            "group_start": i32(group_start), "members": i32(members), "class_start": i32(class_start), "N": int(N), "K": int(K), "G": G}


def subgroup_accumulators(B, G, K, device, fill=0):
    """(confusion int32 [B, G, K, K], counts int64 [B, G, 3 K]) for subgroup_replicates to fill"""
    subgroup_check_limits("subgroup_accumulators", K=int(K), G=int(G), B=int(B))
    return (torch.full((B, G, K, K), fill, dtype=torch.int32, device=device), torch.full((B, G, 3 * K), fill, dtype=torch.int64, device=device))


def subgroup_replicates(tables, seed, mode, confusion, counts, b0=0, b1=None):
    """The per-group integers of replicates [b0, b1) written into their slices of confusion int32 [B, G, K, K] and counts int64
    [B, G, 3 K] (pos, neg, wins2 within the group), one workgroup per replicate (mmskin_subgroup_replicates).  The weights are
    those of bootstrap_weights for the same seed and mode, whatever the groups are."""
    N, K, G = tables["N"], tables["K"], tables["G"]
    _need_gpu(tables["labels"], "subgroup_replicates")
    if confusion is None or confusion.dim() != 4:
        raise ValueError("subgroup_replicates: confusion must be an int32 [B, G, K, K] device tensor")
    B = confusion.shape[0]
    subgroup_check_limits("subgroup_replicates", N=N, K=K, G=G, B=B)
    _dev_tensor(confusion, torch.int32, (B, G, K, K), "subgroup_replicates: confusion")
    _dev_tensor(counts, torch.int64, (B, G, 3 * K), "subgroup_replicates: counts")
    b0, b1 = _bootstrap_range(B, b0, b1)
    call("mmskin_subgroup_replicates", int(seed) & (2 ** 64 - 1), int(mode), N, K, G, B, ptr(tables["labels"]), ptr(tables["preds"]),
         ptr(tables["groups"]), ptr(tables["members"]), ptr(tables["class_start"]), ptr(tables["order"]), ptr(tables["lo"]), ptr(tables["hi"]),
         ptr(tables["group_start"]), b0, b1, ptr(confusion), ptr(counts), stream())


def subgroup_finalize(confusion, counts, confidence=0.95, min_rows=1):
    """(metrics fp64 [G, 7 + 4 K, B], summary fp64 [G, 5, 7 + 4 K]) on the device from the filled accumulators: per group the
    columns of bootstrap_finalize, then K false-positive rates and K predicted rates; a group below `min_rows` weighted rows in a
    replicate is NaN there (mmskin_subgroup_finalize)."""
    _need_gpu(confusion, "subgroup_finalize")
    if confusion.dim() != 4:
        raise ValueError("subgroup_finalize: confusion must be an int32 [B, G, K, K] device tensor")
    B, G, K = confusion.shape[:3]
    subgroup_check_limits("subgroup_finalize", K=K, G=G, B=B)
    _dev_tensor(confusion, torch.int32, (B, G, K, K), "subgroup_finalize: confusion")
    _dev_tensor(counts, torch.int64, (B, G, 3 * K), "subgroup_finalize: counts")
    if int(min_rows) < 1:
        raise ValueError(f"subgroup_finalize: min_rows must be >= 1, got {min_rows}")
    q_lo, q_hi = bootstrap_quantiles(confidence)
    M = subgroup_metric_columns(K)
    metrics = torch.empty((G, M, B), dtype=torch.float64, device=confusion.device)
    summary = torch.empty((G, 5, M), dtype=torch.float64, device=confusion.device)
    call("mmskin_subgroup_finalize", ptr(confusion), ptr(counts), B, G, K, int(min_rows), q_lo, q_hi, ptr(metrics), ptr(summary), stream())
    return metrics, summary


def subgroup_gaps(metrics, confidence=0.95):
    """(lowest, highest, gap fp64 [M, B], lowest_group int64 [M, G], summary fp64 [3, 5, M]) from the metrics fp64 [G, M, B] of
    subgroup_finalize: per column and replicate the extremes over the groups defined there and their difference
    (mmskin_subgroup_gaps)."""
    _need_gpu(metrics, "subgroup_gaps")
    if metrics.dim() != 3:
        raise ValueError("subgroup_gaps: metrics must be an fp64 [G, M, B] device tensor")
    G, M, B = metrics.shape
    subgroup_check_limits("subgroup_gaps", G=G, B=B)
    _dev_tensor(metrics, torch.float64, (G, M, B), "subgroup_gaps: metrics")
    q_lo, q_hi = bootstrap_quantiles(confidence)
    dev = metrics.device
    lowest, highest, gap = (torch.empty((M, B), dtype=torch.float64, device=dev) for _ in range(3))
    lowest_group = torch.empty((M, G), dtype=torch.int64, device=dev)
    summary = torch.empty((3, 5, M), dtype=torch.float64, device=dev)
    call("mmskin_subgroup_gaps", ptr(metrics), B, G, M, q_lo, q_hi, ptr(lowest), ptr(highest), ptr(gap), ptr(lowest_group), ptr(summary), stream())
    return lowest, highest, gap, lowest_group, summary


def subgroup_compare(metrics_a, metrics_b, confidence=0.95):
    """bootstrap_compare on two metric tables fp64 [M, B] of any width: mmskin_bootstrap_compare takes 7 + 2 * 64 columns a call, a
    subgroup table has up to 7 + 4 * 64, so the rows go through it in blocks.  Returns (delta, summary [5, M], sign_counts [M, 2])."""
    step = 7 + 2 * BOOTSTRAP_MAX_CLASSES
    M = metrics_a.shape[0]
    if M <= step:
        return bootstrap_compare(metrics_a, metrics_b, confidence)
    parts = [bootstrap_compare(metrics_a[m:m + step], metrics_b[m:m + step], confidence) for m in range(0, M, step)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts], dim=1), torch.cat([p[2] for p in parts])


# ---------------------------------------------------------------------------------------------- calibration of a fold's probabilities
CALIBRATION_MAX_ROWS = 1 << 24                                                               # MMSKIN_CALIBRATION_MAX_* of mmskin.h
CALIBRATION_MAX_CLASSES = 64
CALIBRATION_MAX_BINS = 64
CALIBRATION_CONF_SCALE_LOG2 = 30                                                             # q(p) = rint(p 2^30)
TEMPERATURE_MAX_CANDIDATES = 64
CALIBRATION_METRICS = ("ece", "mce", "classwise_ece", "confidence_gap", "brier", "nll")      # columns 0 .. 5
CALIBRATION_CLASS_METRICS = ("per_class_ece",)                                               # columns 6 .. 6 + K
CALIBRATION_BINNINGS = ("uniform", "quantile")


def calibration_check_limits(what, N=None, K=None, n_bins=None, R=None):
    """MMSkinError naming the limit that a row, class, bin or replicate count breaks (the C entry points check the same)"""
    if N is not None and not 1 <= N <= CALIBRATION_MAX_ROWS:
        raise _lib.MMSkinError(f"{what}: {N} rows; the codes are indexed in 31 bits, which holds 1 .. CALIBRATION_MAX_ROWS = "
                               f"{CALIBRATION_MAX_ROWS}")
    if K is not None and not 2 <= K <= CALIBRATION_MAX_CLASSES:
        raise _lib.MMSkinError(f"{what}: {K} classes; the kernels hold 2 .. CALIBRATION_MAX_CLASSES = {CALIBRATION_MAX_CLASSES}")
    if n_bins is not None and not 1 <= n_bins <= CALIBRATION_MAX_BINS:
        raise _lib.MMSkinError(f"{what}: {n_bins} bins; a table's cells live in LDS, which holds 1 .. CALIBRATION_MAX_BINS = "
                               f"{CALIBRATION_MAX_BINS}")
    if R is not None and not 1 <= R <= BOOTSTRAP_MAX_RESAMPLES:
        raise _lib.MMSkinError(f"{what}: {R} replicates; a metric column is sorted in LDS, which holds 1 .. BOOTSTRAP_MAX_RESAMPLES = "
                               f"{BOOTSTRAP_MAX_RESAMPLES}")


def _calibration_fold(what, probs, labels):
    _need_gpu(probs, what)
    if probs.dim() != 2 or probs.dtype != torch.float32 or not probs.is_contiguous():
        raise ValueError(f"{what}: probs must be a contiguous fp32 [N, K] tensor, got {probs.dtype} {tuple(probs.shape)}")
    N, K = probs.shape
    calibration_check_limits(what, N=N, K=K)
    _dev_tensor(labels, torch.int64, (N,), f"{what}: labels")
    return N, K


def calibration_confidences(probs):
    """fp32 [K + 1, N]: row 0 the top-label confidence (the row's maximum), row 1 + c the column of class c (torch or numpy)"""
    if isinstance(probs, np.ndarray):
        return np.concatenate([probs.max(axis=1)[None], probs.T], axis=0)
    return torch.cat([probs.max(dim=1).values[None], probs.t()], dim=0).contiguous()


def calibration_edges(probs, labels, n_bins, binning="uniform"):
    """fp32 [K + 1, n_bins + 1]: the bin edges of every table (mmskin.h), e_0 = 0 and e_n = 1.  "uniform": fp32(j / n_bins) for
    every table.  "quantile": per table, with its N confidences sorted ascending, e_j = sorted[ceil(j N / n_bins) - 1] for
    1 <= j < n_bins, so the right-closed bins hold about N / n_bins rows each; equal edges are allowed and leave empty bins.
    probs fp32 [N, K] as a tensor (a device sort) or a numpy array; labels are not read (the tables bin every row)."""
    n_bins = int(n_bins)
    N, K = probs.shape
    calibration_check_limits("calibration_edges", N=N, K=K, n_bins=n_bins)
    if binning not in CALIBRATION_BINNINGS:
        raise ValueError(f"calibration_edges: binning must be one of {CALIBRATION_BINNINGS}, got {binning!r}")
    host = isinstance(probs, np.ndarray)
    if binning == "uniform":
        row = (np.arange(n_bins + 1, dtype=np.float64) / n_bins).astype(np.float32)
        edges = np.ascontiguousarray(np.broadcast_to(row, (K + 1, n_bins + 1)))
        return edges if host else torch.from_numpy(edges).to(probs.device)
    at = -(-np.arange(1, n_bins, dtype=np.int64) * N // n_bins) - 1                             # ceil(j N / n_bins) - 1, in [0, N)
    conf = calibration_confidences(probs)
    if host:
        edges = np.empty((K + 1, n_bins + 1), dtype=np.float32)
        edges[:, 1:n_bins] = np.sort(conf, axis=1)[:, at]
    else:
        edges = torch.empty((K + 1, n_bins + 1), dtype=torch.float32, device=probs.device)
        edges[:, 1:n_bins] = torch.sort(conf, dim=1).values[:, torch.from_numpy(at).to(probs.device)]
    edges[:, 0], edges[:, n_bins] = 0.0, 1.0
    return edges


def calibration_codes(probs, labels, edges):
    """(bin uint8, q int32, hit uint8), each [K + 1, N]: the per-fold codes of every (table, row) (mmskin_calibration_codes)"""
    N, K = _calibration_fold("calibration_codes", probs, labels)
    if edges is None or edges.dim() != 2:
        raise ValueError("calibration_codes: edges must be an fp32 [K + 1, n_bins + 1] device tensor")
    n_bins = edges.shape[1] - 1
    calibration_check_limits("calibration_codes", n_bins=n_bins)
    _dev_tensor(edges, torch.float32, (K + 1, n_bins + 1), "calibration_codes: edges")
    dev = probs.device
    code, hit = (torch.empty((K + 1, N), dtype=torch.uint8, device=dev) for _ in range(2))
    q = torch.empty((K + 1, N), dtype=torch.int32, device=dev)
    call("mmskin_calibration_codes", ptr(probs), ptr(labels), N, K, ptr(edges), n_bins, ptr(code), ptr(q), ptr(hit), stream())
    return code, q, hit


def calibration_bins(codes, n_bins, weights=None, tables=None, b0=0):
    """tables int64 [R, K + 1, n_bins, 3] (count, hits, conf) from the codes of calibration_codes (mmskin_calibration_bins).
    weights None: the fold itself, R = 1.  weights int32 [r, N] (>= 0, each row summing below 2^31): one replicate per row,
    written into the slices [b0, b0 + r) of `tables` (allocated [r, ...] when None) and nowhere else."""
    code, q, hit = codes
    _need_gpu(code, "calibration_bins")
    T, N = code.shape
    K, n_bins = T - 1, int(n_bins)
    r = 1 if weights is None else (weights.shape[0] if weights.dim() == 2 else 0)
    calibration_check_limits("calibration_bins", N=N, K=K, n_bins=n_bins, R=r)
    _dev_tensor(code, torch.uint8, (T, N), "calibration_bins: bin")
    _dev_tensor(q, torch.int32, (T, N), "calibration_bins: q")
    _dev_tensor(hit, torch.uint8, (T, N), "calibration_bins: hit")
    if weights is not None:
        _dev_tensor(weights, torch.int32, (r, N), "calibration_bins: weights")
    if tables is None:
        tables, b0 = torch.empty((r, T, n_bins, 3), dtype=torch.int64, device=code.device), 0
    b0 = int(b0)
    if tables.dim() != 4 or not 0 <= b0 <= b0 + r <= tables.shape[0]:
        raise ValueError(f"calibration_bins: replicates [{b0}, {b0 + r}) are not a range of the tables {tuple(tables.shape)}")
    _dev_tensor(tables, torch.int64, (tables.shape[0], T, n_bins, 3), "calibration_bins: tables")
    call("mmskin_calibration_bins", N, K, n_bins, ptr(code), ptr(q), ptr(hit), ptr(weights), r, ptr(tables[b0:]), stream())
    return tables


def calibration_sums(probs, labels, weights=None):
    """fp64 [R, 2]: the weighted Brier and NLL sums of every replicate (mmskin_calibration_sums); weights None: the fold, R = 1"""
    N, K = _calibration_fold("calibration_sums", probs, labels)
    r = 1 if weights is None else (weights.shape[0] if weights.dim() == 2 else 0)
    calibration_check_limits("calibration_sums", R=r)
    if weights is not None:
        _dev_tensor(weights, torch.int32, (r, N), "calibration_sums: weights")
    dev = probs.device
    scratch = torch.empty(_lib.load().mmskin_calibration_sums_scratch_doubles(N, r), dtype=torch.float64, device=dev)
    sums = torch.empty((r, 2), dtype=torch.float64, device=dev)
    call("mmskin_calibration_sums", ptr(probs), ptr(labels), N, K, ptr(weights), r, ptr(scratch), ptr(sums), stream())
    return sums


def calibration_finalize(tables, sums, confidence=0.95):
    """(metrics fp64 [6 + K, R], summary fp64 [5, 6 + K]) on the device: the columns CALIBRATION_METRICS, then K per-class ECEs;
    the summary rows are BOOTSTRAP_SUMMARY (mmskin_calibration_finalize)."""
    _need_gpu(tables, "calibration_finalize")
    if tables.dim() != 4:
        raise ValueError("calibration_finalize: tables must be an int64 [R, K + 1, n_bins, 3] device tensor")
    R, T, n_bins = tables.shape[:3]
    K = T - 1
    calibration_check_limits("calibration_finalize", K=K, n_bins=n_bins, R=R)
    _dev_tensor(tables, torch.int64, (R, T, n_bins, 3), "calibration_finalize: tables")
    _dev_tensor(sums, torch.float64, (R, 2), "calibration_finalize: sums")
    q_lo, q_hi = bootstrap_quantiles(confidence)
    M = 6 + K
    metrics = torch.empty((M, R), dtype=torch.float64, device=tables.device)
    summary = torch.empty((5, M), dtype=torch.float64, device=tables.device)
    call("mmskin_calibration_finalize", ptr(tables), ptr(sums), R, K, n_bins, q_lo, q_hi, ptr(metrics), ptr(summary), stream())
    return metrics, summary


def _temperature_source(what, src):
    _need_gpu(src, what)
    if src.dim() != 2 or src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError(f"{what}: the scores must be a contiguous fp32 [N, K] tensor, got {src.dtype} {tuple(src.shape)}")
    N, K = src.shape
    calibration_check_limits(what, N=N, K=K)
    return N, K


def temperature_stats(src, labels, betas, from_probs=False):
    """fp64 [G, 3] on the device: per candidate beta = 1 / T the NLL sum of softmax(beta z) over the rows and its first and second
    derivative in beta (mmskin_temperature_stats).  src fp32 [N, K]: logits, or probabilities with from_probs (z = log p);
    betas: G <= TEMPERATURE_MAX_CANDIDATES positive floats on the host."""
    N, K = _temperature_source("temperature_stats", src)
    _dev_tensor(labels, torch.int64, (N,), "temperature_stats: labels")
    betas = np.ascontiguousarray(betas, dtype=np.float64).reshape(-1)
    G = len(betas)
    if not 1 <= G <= TEMPERATURE_MAX_CANDIDATES:
        raise _lib.MMSkinError(f"temperature_stats: {G} candidates; one launch holds 1 .. TEMPERATURE_MAX_CANDIDATES = "
                               f"{TEMPERATURE_MAX_CANDIDATES}")
    dev = src.device
    scratch = torch.empty(_lib.load().mmskin_temperature_scratch_doubles(N, G), dtype=torch.float64, device=dev)
    out = torch.empty((G, 3), dtype=torch.float64, device=dev)
    call("mmskin_temperature_stats", ptr(src), int(bool(from_probs)), ptr(labels), N, K, betas.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
         G, ptr(scratch), ptr(out), stream())
    return out


def temperature_apply(src, beta, from_probs=False):
    """fp32 [N, K] = softmax(beta z), z the logits `src` or log(src) with from_probs (mmskin_temperature_apply)"""
    N, K = _temperature_source("temperature_apply", src)
    out = torch.empty_like(src)
    call("mmskin_temperature_apply", ptr(src), int(bool(from_probs)), N, K, float(beta), ptr(out), stream())
    return out


# ---------------------------------------------------------------------------------------------- ROC / precision-recall curves of a fold
CURVES_MAX_CLASSES = 1024                                                                    # the limits of mmskin_ovr_auc_counts
CURVES_MAX_ROWS = 2 ** 31 - 1
CURVES_MAX_OPERATING_POINTS = 8                                                              # MMSKIN_CURVES_MAX_OPERATING_POINTS of mmskin.h


def curves_check_limits(what, N=None, C=None, n_spec=None, n_sens=None):
    """MMSkinError naming the limit that a row, class or operating-point count breaks (the C entry points check the same)"""
    if C is not None and not 2 <= C <= CURVES_MAX_CLASSES:
        raise _lib.MMSkinError(f"{what}: {C} classes; the kernels hold 2 .. CURVES_MAX_CLASSES = {CURVES_MAX_CLASSES}")
    if N is not None and not 1 <= N <= CURVES_MAX_ROWS:
        raise _lib.MMSkinError(f"{what}: {N} rows is outside 1 .. CURVES_MAX_ROWS = 2^31 - 1")
    for n, kind in ((n_spec, "specificities"), (n_sens, "sensitivities")):
        if n is not None and not 0 <= n <= CURVES_MAX_OPERATING_POINTS:
            raise _lib.MMSkinError(f"{what}: {n} {kind}; a summary holds 0 .. CURVES_MAX_OPERATING_POINTS = {CURVES_MAX_OPERATING_POINTS}")


def ovr_curves(probs, labels, out=None):
    """(thr fp32 [C, N], tp int32 [C, N], fp int32 [C, N], n_points int32 [C], counts int64 [2 C + 1] = pos, neg, nan) on the device
    (mmskin_ovr_curves): per class the distinct scores, descending, with the true and false positives at each; slots at and past
    n_points[c] are zero.  probs fp32 [N, C] contiguous, labels int64 [N].  out: the five tensors to write into, or None."""
    _need_gpu(probs, "ovr_curves")
    if probs.dim() != 2 or probs.dtype != torch.float32 or not probs.is_contiguous():
        raise ValueError(f"ovr_curves: probs must be a contiguous fp32 [N, C] tensor, got {probs.dtype} {tuple(probs.shape)}")
    N, C = probs.shape
    curves_check_limits("ovr_curves", N=N, C=C)
    _dev_tensor(labels, torch.int64, (N,), "ovr_curves: labels")
    dev = probs.device
    if out is None:
        out = (torch.empty((C, N), dtype=torch.float32, device=dev), torch.empty((C, N), dtype=torch.int32, device=dev),
               torch.empty((C, N), dtype=torch.int32, device=dev), torch.empty(C, dtype=torch.int32, device=dev),
               torch.empty(2 * C + 1, dtype=torch.int64, device=dev))
    thr, tp, fp, n_points, counts = out
    _dev_tensor(thr, torch.float32, (C, N), "ovr_curves: thr")
    _dev_tensor(tp, torch.int32, (C, N), "ovr_curves: tp")
    _dev_tensor(fp, torch.int32, (C, N), "ovr_curves: fp")
    _dev_tensor(n_points, torch.int32, (C,), "ovr_curves: n_points")
    _dev_tensor(counts, torch.int64, (2 * C + 1,), "ovr_curves: counts")
    scratch = torch.empty(_lib.load().mmskin_ovr_curves_scratch_ints(N, C), dtype=torch.int32, device=dev)
    call("mmskin_ovr_curves", ptr(probs), ptr(labels), N, C, ptr(scratch), ptr(thr), ptr(tp), ptr(fp), ptr(n_points), ptr(counts), stream())
    return thr, tp, fp, n_points, counts


def ovr_curves_summary(curves, specificities=(), sensitivities=()):
    """fp64 [C, 5 + 3 (A + B)] on the device from the tensors of ovr_curves (mmskin_ovr_curves_summary): auc, average_precision,
    youden_j / threshold / index, then (sensitivity, threshold, index) per requested specificity and (specificity, threshold, index)
    per requested sensitivity; the requests are host sequences of floats."""
    thr, tp, fp, n_points, counts = curves
    _need_gpu(thr, "ovr_curves_summary")
    if thr.dim() != 2:
        raise ValueError("ovr_curves_summary: thr must be an fp32 [C, N] device tensor")
    C, N = thr.shape
    spec = np.ascontiguousarray(specificities, dtype=np.float64).reshape(-1)
    sens = np.ascontiguousarray(sensitivities, dtype=np.float64).reshape(-1)
    curves_check_limits("ovr_curves_summary", N=N, C=C, n_spec=len(spec), n_sens=len(sens))
    _dev_tensor(thr, torch.float32, (C, N), "ovr_curves_summary: thr")
    _dev_tensor(tp, torch.int32, (C, N), "ovr_curves_summary: tp")
    _dev_tensor(fp, torch.int32, (C, N), "ovr_curves_summary: fp")
    _dev_tensor(n_points, torch.int32, (C,), "ovr_curves_summary: n_points")
    _dev_tensor(counts, torch.int64, (2 * C + 1,), "ovr_curves_summary: counts")
    dev = thr.device
    requests = torch.from_numpy(np.concatenate([spec, sens, [0.0]])).to(dev)                     # one copy; never empty
    S = _lib.load().mmskin_ovr_curves_summary_columns(len(spec), len(sens))
    summary = torch.empty((C, S), dtype=torch.float64, device=dev)
    call("mmskin_ovr_curves_summary", ptr(thr), ptr(tp), ptr(fp), ptr(n_points), ptr(counts), N, C, ptr(requests), len(spec),
         ptr(requests[len(spec):]), len(sens), ptr(summary), stream())
    return summary


# ---------------------------------------------------------------------------------------------- per-sample predictive uncertainty
UNCERTAINTY_MAX_PASSES = 4096                                                                # MMSKIN_UNCERTAINTY_MAX_* of mmskin.h
UNCERTAINTY_MAX_CLASSES = 64
UNCERTAINTY_MAX_ROWS = 1 << 24
UNCERTAINTY_STATS = ("confidence", "margin", "predictive_entropy", "expected_entropy", "mutual_information", "variation_ratio",
                     "predicted_std")                                                        # columns 0 .. 6 of stats
RISK_COVERAGE_MAX_ROWS = BOOTSTRAP_MAX_ROWS
RISK_COVERAGE_SUMMARY = ("aurc", "optimal_aurc", "e_aurc", "error_auroc", "error_rate", "n", "n_wrong", "n_distinct")
VIEWS_DIHEDRAL, VIEWS_FLIPS = 0xFF, 0x55                                                     # all 8 views; views 0, 2, 4, 6


def view_ids(view_mask):
    """the view ids of an 8-bit mask, ascending: the order of the slabs mmskin_dihedral_views writes"""
    return [v for v in range(8) if (int(view_mask) >> v) & 1]


def dihedral_views(src, view_mask, out=None):
    """[V, B, C, H, W], one slab per set bit of `view_mask` in ascending view id (mmskin_dihedral_views): view v is
    torch.rot90(src, v & 3, (2, 3)), flipped along W when v & 4.  src: a contiguous [B, C, H, W] device tensor of 1-, 2- or 4-byte
    elements (copied bit for bit).  The library refuses an empty mask and a quarter-turn view of a non-square plane."""
    _need_gpu(src, "dihedral_views")
    if src.dim() != 4 or not src.is_contiguous() or src.element_size() not in (1, 2, 4):
        raise ValueError(f"dihedral_views: src must be a contiguous [B, C, H, W] tensor of 1-, 2- or 4-byte elements, got {src.dtype} "
                         f"{tuple(src.shape)}")
    view_mask = int(view_mask)
    V = len(view_ids(view_mask & 0xFF))
    B, C, H, W = src.shape
    if out is None:
        out = torch.empty((V, B, C, H, W), dtype=src.dtype, device=src.device)
    _dev_tensor(out, src.dtype, (V, B, C, H, W), "dihedral_views: out")
    call("mmskin_dihedral_views", ptr(src), ptr(out), B, C, H, W, src.element_size(), view_mask, stream())
    return out


def uncertainty_check_limits(what, T=None, C=None, N=None):
    """MMSkinError naming the limit that a pass, class or row count breaks (the C entry points check the same)"""
    if T is not None and not 1 <= T <= UNCERTAINTY_MAX_PASSES:
        raise _lib.MMSkinError(f"{what}: T = {T} passes; one call holds 1 .. UNCERTAINTY_MAX_PASSES = {UNCERTAINTY_MAX_PASSES}")
    if C is not None and not 2 <= C <= UNCERTAINTY_MAX_CLASSES:
        raise _lib.MMSkinError(f"{what}: C = {C} classes; the kernel holds one class per lane, 2 .. UNCERTAINTY_MAX_CLASSES = "
                               f"{UNCERTAINTY_MAX_CLASSES}")
    if N is not None and not 1 <= N <= UNCERTAINTY_MAX_ROWS:
        raise _lib.MMSkinError(f"{what}: N = {N} rows is outside 1 .. UNCERTAINTY_MAX_ROWS = 2^24")


def uncertainty_reduce(logits):
    """(mean_prob fp64 [N, C], prob_std fp64 [N, C], votes int32 [N, C], pred int32 [N], stats fp64 [N, 7]) on the device from the
    logits fp32 [T, N, C] of T passes (mmskin_uncertainty_reduce); the columns of stats are UNCERTAINTY_STATS.  The classes of a row
    must be contiguous; the pass and row strides are taken from the tensor, so a slice of a larger block is read in place."""
    _need_gpu(logits, "uncertainty_reduce")
    if logits.dim() != 3 or logits.dtype != torch.float32:
        raise ValueError(f"uncertainty_reduce: logits must be an fp32 [T, N, C] tensor, got {logits.dtype} {tuple(logits.shape)}")
    T, N, C = logits.shape
    uncertainty_check_limits("uncertainty_reduce", T=T, C=C, N=N)
    if logits.stride(2) != 1 and C > 1:
        raise ValueError(f"uncertainty_reduce: the classes of a row must be contiguous, got strides {logits.stride()}")
    dev = logits.device
    mean_prob, prob_std = (torch.empty((N, C), dtype=torch.float64, device=dev) for _ in range(2))
    votes = torch.empty((N, C), dtype=torch.int32, device=dev)
    pred = torch.empty(N, dtype=torch.int32, device=dev)
    stats = torch.empty((N, 7), dtype=torch.float64, device=dev)
    call("mmskin_uncertainty_reduce", ptr(logits), logits.stride(0) if T > 1 else N * logits.stride(1), logits.stride(1) if N > 1 else C, T, N,
         C, ptr(mean_prob), ptr(prob_std), ptr(votes), ptr(pred), ptr(stats), stream())
    return mean_prob, prob_std, votes, pred, stats


def risk_coverage_check_limits(what, N):
    if not 1 <= N <= RISK_COVERAGE_MAX_ROWS:
        raise _lib.MMSkinError(f"{what}: N = {N} rows; the ranking is held in LDS, which holds 1 .. BOOTSTRAP_MAX_ROWS = {RISK_COVERAGE_MAX_ROWS}")


def risk_coverage(score, wrong):
    """counts int32 [N, 4] = (n_lt, n_eq, e_lt, e_eq) per row (mmskin_risk_coverage): the rows with a smaller and with an equal
    score (itself included) and the wrong rows among each.  score fp64 [N] (larger = less sure, no NaN), wrong uint8 [N]."""
    _need_gpu(score, "risk_coverage")
    N = score.shape[0] if score.dim() == 1 else 0
    risk_coverage_check_limits("risk_coverage", N)
    _dev_tensor(score, torch.float64, (N,), "risk_coverage: score")
    _dev_tensor(wrong, torch.uint8, (N,), "risk_coverage: wrong")
    counts = torch.empty((N, 4), dtype=torch.int32, device=score.device)
    call("mmskin_risk_coverage", ptr(score), ptr(wrong), N, ptr(counts), stream())
    return counts


def risk_coverage_summary(counts, wrong):
    """fp64 [8] on the device, the values RISK_COVERAGE_SUMMARY, from the counts of risk_coverage (mmskin_risk_coverage_summary)"""
    _need_gpu(counts, "risk_coverage_summary")
    N = counts.shape[0] if counts.dim() == 2 else 0
    risk_coverage_check_limits("risk_coverage_summary", N)
    _dev_tensor(counts, torch.int32, (N, 4), "risk_coverage_summary: counts")
    _dev_tensor(wrong, torch.uint8, (N,), "risk_coverage_summary: wrong")
    out = torch.empty(8, dtype=torch.float64, device=counts.device)
    call("mmskin_risk_coverage_summary", ptr(counts), ptr(wrong), N, ptr(out), stream())
    return out
