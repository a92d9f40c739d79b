"""Softmax attention over the C ABI: the one route decision (attention_route), the three entry points that ask it (attention,
attention_blhd, attention_packed), the autograd Functions of the five kernel families, and DaViT's window / channel attention and Swin's
shifted-window attention (entry points of their own, outside the route) on the same packed-qkv caller.  The route table is written out once, in DESIGN.md ("The attention route"); tests/attention_route_cases.py holds
it as data."""
import ctypes
import os

import torch

from . import _lib
from ._autograd import _dropout_state, _dtype_code, _f32c, _need_gpu, _needs_grad, get_linear_dtype, no_second_order
from ._lib import call, ptr, stream

# the kernel families: fused bf16 forward (csrc/flash_attn.hip), fused forward + backward (flash_attn_bwd.hip), one wave per head,
# one workgroup per head with the probabilities kept, batched GEMMs + row softmax
FLASH, FLASH_TRAIN, ROWS, BLOCK, LONG = "FLASH", "FLASH_TRAIN", "ROWS", "BLOCK", "LONG"


def _rows_ok(L, Dh):
    """shapes of the one-wave-per-head attention kernels (mmskin_attention_rows_*, mmskin_window_attention_*)"""
    return L <= 64 and Dh in (32, 64)


def attention_route(layout, B, H, L, Dh, dtype, on_device, grad, extras, mode, flash_bwd,
                    contiguous=True, unit_stride=True, same_shape=True, same_dtype=True, aligned=True):
    """Which kernel family serves an attention call, and whether it reads the caller's tensors in place (True) or permuted contiguous
    [B, H, L, Dh] copies (False) -> (family, in_place).  Plain values only, nothing is launched or loaded: layout 'bhld' / 'blhd' /
    'packed'; dtype of q (of qkv); grad: a gradient flows through q, k, v or the bias; extras: mask, bias or causal present; mode: the
    Linear operand mode; flash_bwd: MMSKIN_FLASH_BWD ('0' keeps the unfused fp32 chain for trainable attention).  The rest describes
    the tensors: contiguous (the packed tensor), unit_stride (last dim of q, k, v), same_shape / same_dtype (q, k, v), aligned
    (16 bytes: every pointer and the batch / token / head strides of the views).  The table: DESIGN.md, "The attention route"."""
    # the fused kernels' grid is (query tiles, batch * heads): batch * heads <= 65535 (flash_attn.hip ARG_CHECK); larger launches (DaViT
    # window attention on >= 342 images: 64 windows x 3 heads each) take the rows / unfused kernels instead of raising
    fused = mode == "bf16" and Dh in (32, 64) and on_device and same_shape and B * H <= 65535
    flash = fused and not grad and same_dtype and unit_stride and dtype in (torch.float32, torch.bfloat16)
    in_place = layout == "bhld"
    if not in_place:
        if (layout == "packed" and on_device and dtype == torch.float32 and contiguous and not extras and _rows_ok(L, Dh)
                and not flash):
            return ROWS, True
        if flash and aligned:
            return FLASH, True
        # the copies are contiguous, and fp32 where q was bf16 (bf16 views only exist on the inference lane)
        flash = fused and not grad and (dtype == torch.bfloat16 or (same_dtype and dtype == torch.float32))
    if fused and grad and flash_bwd != "0" and L > 64:      # shorter sequences have the one-wave-per-head fp32 kernels
        return FLASH_TRAIN, in_place
    if flash:
        return FLASH, in_place
    # the one-workgroup-per-head kernel keeps L x L scores in LDS and walks the feature dimension serially: long sequences
    # and long feature dimensions (DaViT's channel attention: feature = tokens) go through the batched-GEMM path
    if extras or L * L * 4 > 64 * 1024 or Dh > 256:
        return LONG, in_place
    return (ROWS if _rows_ok(L, Dh) else BLOCK), in_place


def _aligned16(*ts):
    """16 bytes: every pointer, and every stride but the last"""
    per16 = 16 // ts[0].element_size()
    return all(t.data_ptr() % 16 == 0 and all(s % per16 == 0 for s in t.stride()[:-1]) for t in ts)


def _route(layout, B, H, L, Dh, q, k, v, mask_add, bias, causal):
    """attention_route for the tensors of one call.  k and v None: q is the packed tensor -- its three views share its strides and sit
    a multiple of stride(2) apart, so they are aligned exactly when its pointer and first four strides are."""
    if k is None:
        unit_stride, same_shape, same_dtype, aligned = q.stride(-1) == 1, True, True, _aligned16(q)
    else:
        unit_stride = q.stride(-1) == 1 and k.stride(-1) == 1 and v.stride(-1) == 1
        same_shape, same_dtype = q.shape == k.shape == v.shape, q.dtype == k.dtype == v.dtype
        aligned = layout == "bhld" or _aligned16(q, k, v)
    return attention_route(layout, B, H, L, Dh, q.dtype, q.is_cuda, _needs_grad(q, k, v, bias), mask_add is not None or bias is not None or causal,
                           get_linear_dtype(), os.environ.get("MMSKIN_FLASH_BWD", "1"), q.is_contiguous(), unit_stride, same_shape, same_dtype,
                           aligned)


def _i64x3(a, b, c):
    return (ctypes.c_int64 * 3)(int(a), int(b), int(c))


def _strides(order, *ts):
    """the (batch, head, token) strides of every tensor, in the kernels' int64 array; order: where those dims sit in the tensors"""
    return (ctypes.c_int64 * (3 * len(ts)))(*[t.stride(i) for t in ts for i in order])


def _qkv_ptrs(t):
    """q, k, v pointers inside a packed fp32 tensor [..., 3, H, Dh] -- or d(q), d(k), d(v) inside its gradient tensor"""
    base, step = t.data_ptr(), t.shape[-2] * t.shape[-1] * 4
    return ctypes.c_void_p(base), ctypes.c_void_p(base + step), ctypes.c_void_p(base + 2 * step)


@no_second_order
class AttentionRowsFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(Dh)) v on [B, H, L, Dh] tensors, optional dropout on the probabilities: one wave per head, the row
    log-sum-exp kept instead of the [B, H, L, L] probabilities (L <= 64, Dh 32 / 64)."""

    @staticmethod
    def forward(ctx, q, k, v, drop_p, seed, offset):
        _need_gpu(q, "attention")
        q, k, v = _f32c(q), _f32c(k), _f32c(v)
        B, H, L, Dh = q.shape
        o = torch.empty_like(q)
        lse = torch.empty((B, H, L), device=q.device, dtype=torch.float32)
        ctx.rng = (float(drop_p), int(seed), int(offset))
        st = _i64x3(H * L * Dh, L * Dh, Dh)
        call("mmskin_attention_rows_forward", ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, H, L, Dh, st, st, Dh ** -0.5, *ctx.rng, stream())
        ctx.save_for_backward(q, k, v, o, lse)
        return o

    @staticmethod
    def backward(ctx, dO):
        q, k, v, o, lse = ctx.saved_tensors
        B, H, L, Dh = q.shape
        dO = _f32c(dO)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        st = _i64x3(H * L * Dh, L * Dh, Dh)
        call("mmskin_attention_rows_backward", ptr(dO), ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), ptr(dq), ptr(dk), ptr(dv), B, H, L, Dh,
             st, st, Dh ** -0.5, *ctx.rng, stream())
        return dq, dk, dv, None, None, None


@no_second_order
class AttentionBlockFn(torch.autograd.Function):
    """The same on one workgroup per head, the [B, H, L, L] probabilities kept for the backward (L x L scores in LDS, Dh <= 256)."""

    @staticmethod
    def forward(ctx, q, k, v, drop_p, seed, offset):
        _need_gpu(q, "attention")
        q, k, v = _f32c(q), _f32c(k), _f32c(v)
        B, H, L, Dh = q.shape
        o = torch.empty_like(q)
        p = torch.empty((B, H, L, L), device=q.device, dtype=torch.float32)
        ctx.rng = (float(drop_p), int(seed), int(offset))
        call("mmskin_attention_forward", ptr(q), ptr(k), ptr(v), ptr(o), ptr(p), B, H, L, Dh, *ctx.rng, stream())
        ctx.save_for_backward(q, k, v, p)
        return o

    @staticmethod
    def backward(ctx, dO):
        q, k, v, p = ctx.saved_tensors
        B, H, L, Dh = q.shape
        dO = _f32c(dO)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        call("mmskin_attention_backward", ptr(dO), ptr(q), ptr(k), ptr(v), ptr(p), ptr(dq), ptr(dk), ptr(dv), B, H, L,
             Dh, *ctx.rng, stream())
        return dq, dk, dv, None, None, None


@no_second_order
class AttentionPackedFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(Dh)) v straight on the packed [B, L, 3, H, Dh] output of a fused qkv Linear -> [B, L, H, Dh] (token-major,
    what the output projection reads); the backward writes d(qkv) in the packed layout.  No permute / contiguous copies in either
    direction (timm Attention.forward / DaViT WindowAttention with gradients: window attention of 49 tokens, Dh 32)."""

    @staticmethod
    def forward(ctx, qkv, drop_p, seed, offset):
        _need_gpu(qkv, "attention_packed")
        qkv = _f32c(qkv)
        B, L, three, H, Dh = qkv.shape
        o = torch.empty((B, L, H, Dh), device=qkv.device, dtype=torch.float32)
        lse = torch.empty((B, H, L), device=qkv.device, dtype=torch.float32)
        ctx.rng = (float(drop_p), int(seed), int(offset))
        qs, os_ = _i64x3(L * 3 * H * Dh, Dh, 3 * H * Dh), _i64x3(L * H * Dh, Dh, H * Dh)
        call("mmskin_attention_rows_forward", *_qkv_ptrs(qkv), ptr(o), ptr(lse), B, H, L, Dh, qs, os_, Dh ** -0.5, *ctx.rng, stream())
        ctx.save_for_backward(qkv, o, lse)
        return o

    @staticmethod
    def backward(ctx, dO):
        qkv, o, lse = ctx.saved_tensors
        B, L, three, H, Dh = qkv.shape
        dO = _f32c(dO)
        dqkv = torch.empty_like(qkv)
        qs, os_ = _i64x3(L * 3 * H * Dh, Dh, 3 * H * Dh), _i64x3(L * H * Dh, Dh, H * Dh)
        call("mmskin_attention_rows_backward", ptr(dO), *_qkv_ptrs(qkv), ptr(o), ptr(lse), *_qkv_ptrs(dqkv), B, H, L, Dh,
             qs, os_, Dh ** -0.5, *ctx.rng, stream())
        return dqkv, None, None, None


@no_second_order
class WindowAttentionFn(torch.autograd.Function):
    """Window attention on the packed qkv of an image-major token grid, qkv [B, Hp, Wp, 3, H, Dh] -> [B, Hp, Wp, H, Dh]: every ws x ws
    window attends over its own tokens where they sit (mmskin_window_attention_*), so timm's window_partition / window_reverse
    (davit.py SpatialBlock.forward) cost no copy in either direction."""

    @staticmethod
    def forward(ctx, qkv, ws, drop_p, seed, offset):
        _need_gpu(qkv, "window_attention")
        qkv = _f32c(qkv)
        B, Hp, Wp, three, H, Dh = qkv.shape
        nwy, nwx = Hp // ws, Wp // ws
        o = torch.empty((B, Hp, Wp, H, Dh), device=qkv.device, dtype=torch.float32)
        lse = torch.empty((B * nwy * nwx, H, ws * ws), device=qkv.device, dtype=torch.float32)
        ctx.rng = (float(drop_p), int(seed), int(offset))
        ctx.geom = (B, nwy, nwx, ws, H, Dh)
        call("mmskin_window_attention_forward", *_qkv_ptrs(qkv), ptr(o), ptr(lse), *ctx.geom, 3 * H * Dh, Dh, H * Dh, Dh, Dh ** -0.5,
             *ctx.rng, stream())
        ctx.save_for_backward(qkv, o, lse)
        return o

    @staticmethod
    def backward(ctx, dO):
        qkv, o, lse = ctx.saved_tensors
        B, nwy, nwx, ws, H, Dh = ctx.geom
        dO = _f32c(dO)
        dqkv = torch.empty_like(qkv)
        call("mmskin_window_attention_backward", ptr(dO), *_qkv_ptrs(qkv), ptr(o), ptr(lse), *_qkv_ptrs(dqkv), *ctx.geom,
             3 * H * Dh, Dh, H * Dh, Dh, Dh ** -0.5, *ctx.rng, stream())
        return dqkv, None, None, None, None


def window_attention_ok(qkv, ws):
    """shapes mmskin_window_attention_* takes: fp32 packed qkv [B, Hp, Wp, 3, H, Dh] on the GPU, Hp / Wp multiples of ws, ws*ws <= 64, Dh 32 / 64"""
    return (qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 6 and qkv.shape[3] == 3 and qkv.is_contiguous()
            and qkv.shape[1] % ws == 0 and qkv.shape[2] % ws == 0 and _rows_ok(ws * ws, qkv.shape[5]))


def window_attention(qkv, ws, dropout_p=0.0, training=False):
    """softmax(q k^T / sqrt(Dh)) v inside every ws x ws window of the token grid; qkv [B, Hp, Wp, 3, H, Dh] -> [B, Hp, Wp, H, Dh]."""
    B, Hp, Wp, _, H, Dh = qkv.shape
    p = dropout_p if training else 0.0
    nw = B * (Hp // ws) * (Wp // ws)
    seed, offset = _dropout_state(p, nw * H * (ws * ws) ** 2)
    return WindowAttentionFn.apply(qkv, ws, p, seed, offset)


@no_second_order
class SwinWindowAttentionFn(torch.autograd.Function):
    """Shifted-window attention of the Swin Transformer on the packed qkv of an image-major token grid, qkv [B, Hp, Wp, 3, H, Dh] and
    bias_table [(2 ws - 1)^2, H] -> [B, Hp, Wp, H, Dh]: the cyclic shift, the window partition, the relative-position bias gather and the
    -100 region mask of timm's SwinTransformerBlock._attn / WindowAttention are index arithmetic of mmskin_swin_attention_*; the backward
    writes d(qkv) packed and the table gradient through a fixed-order fp64 reduction."""

    @staticmethod
    def forward(ctx, qkv, bias_table, ws, shift, drop_p, seed, offset):
        _need_gpu(qkv, "swin_window_attention")
        if qkv.dim() != 6 or qkv.shape[3] != 3:
            raise _lib.MMSkinError(f"mmskin.swin_window_attention: qkv {tuple(qkv.shape)} is not [B, Hp, Wp, 3, H, Dh]")
        qkv, bias_table = _f32c(qkv), _f32c(bias_table)
        B, Hp, Wp, three, H, Dh = qkv.shape
        if ws < 1 or tuple(bias_table.shape) != ((2 * ws - 1) ** 2, H) or not bias_table.is_cuda:
            raise _lib.MMSkinError(f"mmskin.swin_window_attention: bias table {tuple(bias_table.shape)}, expected {((2 * ws - 1) ** 2, H)} on the GPU")
        ctx.rng = (float(drop_p), int(seed), int(offset))
        ctx.geom = (B, Hp, Wp, int(ws), *_shift_yx(shift), H, Dh, 3 * H * Dh, Dh, H * Dh, Dh, Dh ** -0.5)
        o = torch.empty((B, Hp, Wp, H, Dh), device=qkv.device, dtype=torch.float32)
        lse = torch.empty((B * (Hp // ws) * (Wp // ws), H, ws * ws), device=qkv.device, dtype=torch.float32)
        call("mmskin_swin_attention_forward", *_qkv_ptrs(qkv), ptr(bias_table), ptr(o), ptr(lse), *ctx.geom, *ctx.rng, stream())
        ctx.save_for_backward(qkv, bias_table, o, lse)
        return o

    @staticmethod
    def backward(ctx, dO):
        qkv, bias_table, o, lse = ctx.saved_tensors
        B, Hp, Wp, ws, _, _, H = ctx.geom[:7]
        dO = _f32c(dO)
        dqkv = torch.empty_like(qkv)
        dtable = workspace = None
        if ctx.needs_input_grad[1]:
            dtable = torch.empty_like(bias_table)
            workspace = torch.empty(_lib.load().mmskin_swin_attention_workspace_bytes(B, Hp, Wp, ws, H), device=qkv.device, dtype=torch.uint8)
        call("mmskin_swin_attention_backward", ptr(dO), *_qkv_ptrs(qkv), ptr(bias_table), ptr(o), ptr(lse), *_qkv_ptrs(dqkv), ptr(dtable),
             ptr(workspace), *ctx.geom, *ctx.rng, stream())
        return dqkv, dtable, None, None, None, None, None


def _shift_yx(shift):
    """one shift for both axes, or timm's per-axis (shift_y, shift_x)"""
    return (int(shift), int(shift)) if isinstance(shift, int) else (int(shift[0]), int(shift[1]))


def swin_window_attention_ok(qkv, bias_table, ws, shift):
    """shapes mmskin_swin_attention_* takes: fp32 packed qkv [B, Hp, Wp, 3, H, Dh] and table [(2 ws - 1)^2, H] on the GPU, Hp / Wp
    multiples of ws, ws*ws <= 64, 0 <= shift < ws (one int, or one per axis), Dh 32 / 64"""
    return (qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 6 and qkv.shape[3] == 3 and qkv.is_contiguous() and ws >= 1
            and qkv.shape[1] % ws == 0 and qkv.shape[2] % ws == 0 and _rows_ok(ws * ws, qkv.shape[5]) and all(0 <= s < ws for s in _shift_yx(shift))
            and bias_table.is_cuda and bias_table.dtype == torch.float32 and tuple(bias_table.shape) == ((2 * ws - 1) ** 2, qkv.shape[4]))


def swin_window_attention(qkv, bias_table, ws, shift, dropout_p=0.0, training=False):
    """softmax(q k^T / sqrt(Dh) + relative-position bias + shift mask) v inside every ws x ws window of the token grid rolled by
    (-shift, -shift) -- or by (-shift[0], -shift[1]) -- and written back un-rolled; qkv [B, Hp, Wp, 3, H, Dh], bias_table [(2 ws - 1)^2, H] -> [B, Hp, Wp, H, Dh]."""
    p = dropout_p if training else 0.0
    seed, offset = _dropout_state(p, qkv.numel() // (3 * qkv.shape[-1]) * (ws * ws) if qkv.dim() == 6 else 0)
    return SwinWindowAttentionFn.apply(qkv, bias_table, ws, shift, p, seed, offset)


@no_second_order
class ChannelAttentionFn(torch.autograd.Function):
    """DaViT channel attention on the packed qkv of a fused Linear, qkv [B, N, 3, G, 32] -> [B, N, G, 32] (token-major, what the output
    projection reads): A = softmax(scale q^T k) over each group's 32 channels, x = (A v^T)^T (timm davit.py ChannelAttention.forward).
    No permute / contiguous copies; the backward writes d(qkv) in the packed layout."""

    @staticmethod
    def forward(ctx, qkv, scale):
        _need_gpu(qkv, "channel_attention")
        qkv = _f32c(qkv)
        B, N, three, G, Dh = qkv.shape
        x = torch.empty((B, N, G, Dh), device=qkv.device, dtype=torch.float32)
        attn = torch.empty((B * G, Dh, Dh), device=qkv.device, dtype=torch.float32)
        ctx.scale = float(scale)
        ns = _lib.load().mmskin_channel_attention_scratch_floats(B, G, N)
        scratch = torch.empty(ns, device=qkv.device, dtype=torch.float32) if ns else None
        call("mmskin_channel_attention_forward", *_qkv_ptrs(qkv), ptr(x), ptr(attn), ptr(scratch), B, G, N, Dh,
             3 * G * Dh, N * 3 * G * Dh, G * Dh, N * G * Dh, ctx.scale, stream())
        ctx.save_for_backward(qkv, attn)
        return x

    @staticmethod
    def backward(ctx, dO):
        qkv, attn = ctx.saved_tensors
        B, N, three, G, Dh = qkv.shape
        dO = _f32c(dO)
        dqkv = torch.empty_like(qkv)
        ns = _lib.load().mmskin_channel_attention_scratch_floats(B, G, N)
        scratch = torch.empty(ns, device=qkv.device, dtype=torch.float32) if ns else None
        call("mmskin_channel_attention_backward", ptr(dO), *_qkv_ptrs(qkv), ptr(attn), *_qkv_ptrs(dqkv), ptr(scratch), B, G, N, Dh,
             3 * G * Dh, N * 3 * G * Dh, G * Dh, N * G * Dh, ctx.scale, stream())
        return dqkv, None


def channel_attention_ok(qkv):
    """shapes mmskin_channel_attention_* takes: fp32 packed qkv [B, N, 3, G, 32] on the GPU"""
    return qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 5 and qkv.shape[2] == 3 and qkv.shape[4] == 32 and qkv.is_contiguous()


def channel_attention(qkv, scale):
    return ChannelAttentionFn.apply(qkv, scale)


def _bmm(a, b, c, batch, M, N, K, sam, sak, sab, sbn, sbk, sbb, ldc, scb):
    call("mmskin_bmm", ptr(a), ptr(b), ptr(c), batch, M, N, K, sam, sak, sab, sbn, sbk, sbb, ldc, scb, stream())


@no_second_order
class LongAttentionFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(Dh) + mask) v for sequences whose score matrix does not fit one workgroup's LDS
    (BERT: L = 512): strided batched GEMMs + a row-softmax kernel, the probabilities kept for backward.
    q, k, v [B, H, L, Dh]; mask_add [B, L] additive key mask or None; dropout on the probabilities when drop_p > 0."""

    @staticmethod
    def forward(ctx, q, k, v, mask_add, drop_p, seed, offset, bias=None, causal=False):
        _need_gpu(q, "attention")
        q, k, v = _f32c(q), _f32c(k), _f32c(v)
        B, H, L, Dh = q.shape
        BH = B * H
        scores = torch.empty((B, H, L, L), device=q.device, dtype=torch.float32)
        _bmm(q, k, scores, BH, L, L, Dh, Dh, 1, L * Dh, Dh, 1, L * Dh, L, L * L)
        probs = torch.empty_like(scores)
        m = _f32c(mask_add) if mask_add is not None else None
        bs = _f32c(bias) if bias is not None else None                              # [H, L, L], shared by the batch
        call("mmskin_softmax_forward", ptr(scores), ptr(m), ptr(bs), ptr(probs), BH * L, L, H * L, 1.0 / Dh ** 0.5, int(causal), stream())
        ctx.has_bias = bias is not None
        del scores
        dmask = None
        pd = probs
        if drop_p > 0.0:
            pd = torch.empty_like(probs)
            dmask = torch.empty(probs.shape, device=q.device, dtype=torch.uint8)
            call("mmskin_attn_dropout_forward", ptr(probs), ptr(pd), ptr(dmask), probs.numel(), L, float(drop_p), int(seed), int(offset), stream())
        o = torch.empty_like(q)
        _bmm(pd, v, o, BH, L, Dh, L, L, 1, L * L, 1, Dh, L * Dh, Dh, L * Dh)          # o[i][d] = sum_j pd[i][j] v[j][d]
        ctx.save_for_backward(q, k, v, probs, pd if drop_p > 0.0 else None, dmask)
        ctx.drop_p = float(drop_p)
        return o

    @staticmethod
    def backward(ctx, dO):
        q, k, v, probs, pd, dmask = ctx.saved_tensors
        B, H, L, Dh = q.shape
        BH = B * H
        dO = _f32c(dO)
        pdrop = pd if pd is not None else probs
        dv = torch.empty_like(v)
        _bmm(pdrop, dO, dv, BH, L, Dh, L, 1, L, L * L, 1, Dh, L * Dh, Dh, L * Dh)        # dv[j][d] = sum_i pd[i][j] dO[i][d]
        dp = torch.empty_like(probs)
        _bmm(dO, v, dp, BH, L, L, Dh, Dh, 1, L * Dh, Dh, 1, L * Dh, L, L * L)           # dp[i][j] = sum_d dO[i][d] v[j][d]
        if dmask is not None:
            dp2 = torch.empty_like(dp)
            call("mmskin_dropout_backward", ptr(dp), ptr(dmask), ptr(dp2), dp.numel(), ctx.drop_p, stream())
            dp = dp2
        ds = torch.empty_like(dp)
        call("mmskin_softmax_backward", ptr(dp), ptr(probs), ptr(ds), BH * L, L, 1.0 / Dh ** 0.5, stream())
        del dp
        dq, dk = torch.empty_like(q), torch.empty_like(k)
        _bmm(ds, k, dq, BH, L, Dh, L, L, 1, L * L, 1, Dh, L * Dh, Dh, L * Dh)            # dq[i][d] = sum_j ds[i][j] k[j][d]
        _bmm(ds, q, dk, BH, L, Dh, L, 1, L, L * L, 1, Dh, L * Dh, Dh, L * Dh)            # dk[j][d] = sum_i ds[i][j] q[i][d]
        dbias = None
        if ctx.has_bias and ctx.needs_input_grad[7]:       # d/d(bias) = d/d(scaled scores) summed over the batch = ds / scale
            dbias = torch.empty((H, L, L), device=q.device, dtype=torch.float32)
            call("mmskin_colsum", ptr(ds), ptr(dbias), B, H * L * L, stream())
            dbias.mul_(Dh ** 0.5)
        return dq, dk, dv, None, None, None, None, dbias, None


def _flash_forward(q, k, v, out, lse, dims, order, mask_add, bias, causal, p, seed, offset):
    """The one caller of the fused forward (csrc/flash_attn.hip): q, k, v fp32 or bf16 with (batch, head, token) at dims `order`, out
    in their dtype and layout; lse [B, H, L] (kept for the fused backward) or None.  -> the fp32 mask and bias it read."""
    B, H, L, Dh = dims
    if bias is not None and tuple(bias.shape) != (H, L, L):
        raise _lib.MMSkinError(f"mmskin.attention: bias must be [H, L, L] = {(H, L, L)}, got {tuple(bias.shape)}")
    if mask_add is not None and tuple(mask_add.shape) != (B, L):
        raise _lib.MMSkinError(f"mmskin.attention: mask_add must be [B, L] = {(B, L)}, got {tuple(mask_add.shape)}")
    m = _f32c(mask_add) if mask_add is not None else None
    bs = _f32c(bias) if bias is not None else None
    call("mmskin_flash_attention_forward", ptr(q), ptr(k), ptr(v), ptr(m), ptr(bs), ptr(out), ptr(lse), B, H, L, Dh,
         _strides(order, q, k, v, out), _dtype_code(q), 1.0 / Dh ** 0.5, int(causal), float(p), int(seed), int(offset), stream())
    return m, bs


@no_second_order
class FlashAttnFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(Dh) + bias + mask) v with gradients, fused (forward with the row log-sum-exp kept, backward recomputing the
    probabilities: csrc/flash_attn_bwd.hip): q, k, v [B, H, L, Dh] fp32 (rounded to bf16 operands inside), mask_add [B, L] or None,
    bias [H, L, L] or None (its gradient is the sum of dS over the batch), dropout on the probabilities."""

    @staticmethod
    def forward(ctx, q, k, v, mask_add, bias, causal, p, seed, offset):
        q, k, v = _f32c(q), _f32c(k), _f32c(v)
        B, H, L, Dh = q.shape
        out = torch.empty_like(q)
        lse = torch.empty((B, H, L), device=q.device, dtype=torch.float32)
        m, bs = _flash_forward(q, k, v, out, lse, (B, H, L, Dh), (0, 1, 2), mask_add, bias, causal, p, seed, offset)
        ctx.save_for_backward(q, k, v, out, lse, m, bs)
        ctx.cfg = (bool(causal), float(p), int(seed), int(offset))
        return out

    @staticmethod
    def backward(ctx, dO):
        q, k, v, out, lse, m, bs = ctx.saved_tensors
        causal, p, seed, offset = ctx.cfg
        B, H, L, Dh = q.shape
        dO = _f32c(dO)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
        delta = torch.empty((B, H, L), device=q.device, dtype=torch.float32)
        bT = bs.transpose(1, 2).contiguous() if bs is not None else None
        ds = torch.empty((B, H, L, L), device=q.device, dtype=torch.float32) if bs is not None and ctx.needs_input_grad[4] else None
        call("mmskin_flash_attention_backward", ptr(q), ptr(k), ptr(v), ptr(out), ptr(dO), ptr(lse), ptr(m), ptr(bs), ptr(bT), ptr(delta),
             ptr(dq), ptr(dk), ptr(dv), ptr(ds), B, H, L, Dh, _strides((0, 1, 2), q, q, q, q, q), 1.0 / Dh ** 0.5, int(causal), p, seed,
             offset, stream())
        dbias = None
        if ds is not None:       # d(bias) = dS summed over the batch (deterministic column sum, as the unfused path does)
            dbias = torch.empty((H, L, L), device=q.device, dtype=torch.float32)
            call("mmskin_colsum", ptr(ds), ptr(dbias), B, H * L * L, stream())
        return dq, dk, dv, None, dbias, None, None, None, None


def _run(family, q, k, v, mask_add, bias, causal, p, seed, offset):
    """one kernel family on [B, H, L, Dh] tensors"""
    if family == FLASH_TRAIN:
        return FlashAttnFn.apply(q, k, v, mask_add, bias, causal, p, seed, offset)
    if family == FLASH:
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out = torch.empty_like(q)
        _flash_forward(q, k, v, out, None, q.shape, (0, 1, 2), mask_add, bias, causal, p, seed, offset)
        return out
    if family == LONG:
        return LongAttentionFn.apply(q, k, v, mask_add, p, seed, offset, bias, causal)
    return (AttentionRowsFn if family == ROWS else AttentionBlockFn).apply(q, k, v, p, seed, offset)


def _run_blhd(family, in_place, q, k, v, mask_add, bias, causal, p, seed, offset):
    """the same on [B, L, H, Dh] views -> [B, L, H, Dh] contiguous: FLASH on the views themselves, anything else on permuted copies"""
    if in_place:
        B, L, H, Dh = q.shape
        out = torch.empty((B, L, H, Dh), device=q.device, dtype=q.dtype)
        _flash_forward(q, k, v, out, None, (B, H, L, Dh), (0, 2, 1), mask_add, bias, causal, p, seed, offset)
        return out
    if q.dtype == torch.bfloat16:     # bf16 views only exist on the inference lane; off the fused kernel's shapes go through fp32
        q, k, v = q.float(), k.float(), v.float()
    o = _run(family, q.permute(0, 2, 1, 3).contiguous(), k.permute(0, 2, 1, 3).contiguous(), v.permute(0, 2, 1, 3).contiguous(),
             mask_add, bias, causal, p, seed, offset)
    return o.permute(0, 2, 1, 3).contiguous()


def attention(q, k, v, dropout_p=0.0, training=False, mask_add=None, bias=None, causal=False):
    """softmax(q k^T / sqrt(Dh) + bias + mask_add) v on [B, H, L, Dh] tensors, dropout on the probabilities when training."""
    B, H, L, Dh = q.shape
    family, _ = _route("bhld", B, H, L, Dh, q, k, v, mask_add, bias, causal)
    p = dropout_p if training else 0.0
    return _run(family, q, k, v, mask_add, bias, causal, p, *_dropout_state(p, B * H * L * L))


def attention_blhd(q, k, v, dropout_p=0.0, training=False, mask_add=None, bias=None, causal=False):
    """Attention on token-major views: q, k, v [B, L, H, Dh] (any strides with a contiguous last dim, e.g. slices of the
    [B, L, 3, H, Dh] output of a fused qkv Linear) -> [B, L, H, Dh] contiguous."""
    B, L, H, Dh = q.shape
    family, in_place = _route("blhd", B, H, L, Dh, q, k, v, mask_add, bias, causal)
    p = dropout_p if training else 0.0
    return _run_blhd(family, in_place, q, k, v, mask_add, bias, causal, p, *_dropout_state(p, B * H * L * L))


def attention_packed(qkv, dropout_p=0.0, training=False, mask_add=None, bias=None, causal=False):
    """Attention on the packed output of a fused qkv Linear, qkv [B, L, 3, H, Dh] -> [B, L, H, Dh]."""
    B, L, _, H, Dh = qkv.shape
    family, in_place = _route("packed", B, H, L, Dh, qkv, None, None, mask_add, bias, causal)
    p = dropout_p if training else 0.0
    seed, offset = _dropout_state(p, B * H * L * L)
    if family == ROWS and in_place:
        return AttentionPackedFn.apply(qkv, p, seed, offset)
    return _run_blhd(family, in_place, qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], mask_add, bias, causal, p, seed, offset)
