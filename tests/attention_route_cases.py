"""The attention route table of mmskin/attention.py (attention_route) as data, and the tensors and the fp64 reference the route tests
share.  No GPU needed to import: tests/test_cpu_attention_routes.py asks attention_route for every row, tests/test_gpu_attention_routes.py
runs the rows marked gpu through the public entry points.

A row is (id, arguments of attention_route, which of mask / bias / causal is present, runs on the GPU, (family, in place)).  The comment
behind a row names the condition it stands on.  The expectations were read off the three nested routers as they stood in ops.py before
attention_route existed (attention_packed -> attention_blhd -> attention with _rows_ok / _flash_ok / _flash_train_ok)."""
import math

import torch

FLASH, FLASH_TRAIN, ROWS, BLOCK, LONG = "FLASH", "FLASH_TRAIN", "ROWS", "BLOCK", "LONG"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def row(cid, layout, B, H, L, Dh, expect, mode="fp32", grad=True, extras=None, dtype=F32, flash_bwd="1", gpu=True, **views):
    """views: on_device / contiguous / unit_stride / same_shape / same_dtype / aligned where they differ from True"""
    args = dict(layout=layout, B=B, H=H, L=L, Dh=Dh, dtype=dtype, on_device=True, grad=grad, extras=extras is not None, mode=mode,
                flash_bwd=flash_bwd)
    args.update(views)
    return cid, args, extras, gpu, expect


ROUTE_CASES = [
    # ---- [B, H, L, Dh], fp32 mode: LONG, then ROWS, then BLOCK
    row("bhld-f32-L64-D32", "bhld", 2, 2, 64, 32, (ROWS, True)),                   # L <= 64 at its edge, Dh 32
    row("bhld-f32-L65-D32", "bhld", 2, 2, 65, 32, (BLOCK, True)),                  # L <= 64 fails by one token
    row("bhld-f32-L64-D64", "bhld", 2, 2, 64, 64, (ROWS, True)),                   # Dh 64
    row("bhld-f32-L64-D48", "bhld", 2, 2, 64, 48, (BLOCK, True)),                  # Dh in {32, 64} fails
    row("bhld-f32-L128-D32", "bhld", 2, 2, 128, 32, (BLOCK, True)),                # L * L * 4 = 65536: not above
    row("bhld-f32-L129-D32", "bhld", 2, 2, 129, 32, (LONG, True)),                 # L * L * 4 > 65536
    row("bhld-f32-L8-D256", "bhld", 2, 2, 8, 256, (BLOCK, True)),                  # Dh > 256 fails at its edge
    row("bhld-f32-L8-D257", "bhld", 2, 2, 8, 257, (LONG, True)),                   # Dh > 256
    row("bhld-f32-mask", "bhld", 2, 2, 16, 32, (LONG, True), extras="mask"),       # a key mask alone
    row("bhld-f32-bias", "bhld", 2, 2, 16, 32, (LONG, True), extras="bias"),       # a bias alone
    row("bhld-f32-causal", "bhld", 2, 2, 16, 32, (LONG, True), extras="causal"),   # causal alone
    row("bhld-f32-nograd-L64", "bhld", 2, 2, 64, 32, (ROWS, True), grad=False),    # fp32 mode: gradients do not move the route
    row("bhld-f32-nograd-L65", "bhld", 2, 2, 65, 32, (BLOCK, True), grad=False),
    row("bhld-f32-cpu", "bhld", 2, 2, 16, 32, (ROWS, True), gpu=False, on_device=False),   # the route does not look at the device off the fused kernels (the Function raises)
    # ---- [B, H, L, Dh], bf16 mode without gradients: FLASH first
    row("bhld-bf16-nograd-L64-D32", "bhld", 2, 2, 64, 32, (FLASH, True), "bf16", False),   # FLASH has no minimum L
    row("bhld-bf16-nograd-L65-D64", "bhld", 2, 2, 65, 64, (FLASH, True), "bf16", False),
    row("bhld-bf16-nograd-L64-D48", "bhld", 2, 2, 64, 48, (BLOCK, True), "bf16", False),   # Dh in {32, 64} fails: the fp32 list
    row("bhld-bf16-nograd-L129-D48", "bhld", 2, 2, 129, 48, (LONG, True), "bf16", False),
    row("bhld-bf16-nograd-mask", "bhld", 2, 2, 16, 32, (FLASH, True), "bf16", False, "mask"),      # FLASH takes mask, bias and causal itself
    row("bhld-bf16-nograd-bias", "bhld", 2, 2, 16, 32, (FLASH, True), "bf16", False, "bias"),
    row("bhld-bf16-nograd-causal", "bhld", 2, 2, 16, 32, (FLASH, True), "bf16", False, "causal"),
    row("bhld-bf16-nograd-f16", "bhld", 2, 2, 16, 32, (ROWS, True), "bf16", False, dtype=F16),     # dtype fp32 or bf16 fails
    row("bhld-bf16-nograd-strided", "bhld", 2, 2, 16, 32, (ROWS, True), "bf16", False, contiguous=False, unit_stride=False),   # unit last stride fails
    row("bhld-bf16-nograd-cpu", "bhld", 2, 2, 16, 32, (ROWS, True), "bf16", False, gpu=False, on_device=False),                # on device fails
    row("bhld-bf16-nograd-shapes", "bhld", 2, 2, 16, 32, (ROWS, True), "bf16", False, gpu=False, same_shape=False),            # equal shapes fails (never launched: the kernels take one L)
    row("bhld-bf16-nograd-dtypes", "bhld", 2, 2, 16, 32, (ROWS, True), "bf16", False, gpu=False, same_dtype=False),            # equal dtypes fails
    row("bhld-bf16-nograd-BH65535", "bhld", 21845, 3, 2, 32, (FLASH, True), "bf16", False),        # B * H <= 65535 at its edge
    row("bhld-bf16-nograd-BH65536", "bhld", 16384, 4, 2, 32, (ROWS, True), "bf16", False),         # the grid limit: one pair too many
    # ---- [B, H, L, Dh], bf16 mode with gradients: FLASH_TRAIN first
    row("bhld-bf16-grad-L65-D64", "bhld", 2, 2, 65, 64, (FLASH_TRAIN, True), "bf16"),              # L > 64 at its edge
    row("bhld-bf16-grad-L64-D64", "bhld", 2, 2, 64, 64, (ROWS, True), "bf16"),                     # L > 64 fails: the one-wave-per-head kernels
    row("bhld-bf16-grad-L65-D32", "bhld", 2, 2, 65, 32, (FLASH_TRAIN, True), "bf16"),
    row("bhld-bf16-grad-L65-D48", "bhld", 2, 2, 65, 48, (BLOCK, True), "bf16"),                    # Dh in {32, 64} fails
    row("bhld-bf16-grad-L65-bwd0", "bhld", 2, 2, 65, 64, (BLOCK, True), "bf16", flash_bwd="0"),    # MMSKIN_FLASH_BWD=0: the unfused fp32 chain
    row("bhld-bf16-grad-L129-bwd0", "bhld", 2, 2, 129, 64, (LONG, True), "bf16", flash_bwd="0"),
    row("bhld-bf16-grad-mask-L65", "bhld", 2, 2, 65, 32, (FLASH_TRAIN, True), "bf16", extras="mask"),
    row("bhld-bf16-grad-bias-L65", "bhld", 2, 2, 65, 32, (FLASH_TRAIN, True), "bf16", extras="bias"),
    row("bhld-bf16-grad-causal-L65", "bhld", 2, 2, 65, 32, (FLASH_TRAIN, True), "bf16", extras="causal"),
    row("bhld-bf16-grad-mask-L16", "bhld", 2, 2, 16, 32, (LONG, True), "bf16", extras="mask"),     # below the FLASH_TRAIN minimum a mask means LONG
    row("bhld-bf16-grad-BH65535", "bhld", 21845, 3, 65, 32, (FLASH_TRAIN, True), "bf16", gpu=False),   # B * H <= 65535 at its edge (hundreds of MB: CPU only)
    row("bhld-bf16-grad-BH65536", "bhld", 16384, 4, 65, 32, (BLOCK, True), "bf16", gpu=False),     # the grid limit with gradients
    # ---- [B, L, H, Dh] views: FLASH in place when aligned, else the list above on permuted contiguous copies
    row("blhd-bf16-nograd-aligned", "blhd", 2, 2, 65, 64, (FLASH, True), "bf16", False, contiguous=False),
    row("blhd-bf16-nograd-misaligned", "blhd", 2, 2, 65, 64, (FLASH, False), "bf16", False, aligned=False),    # 16-byte alignment fails: still FLASH, through copies
    row("blhd-bf16-nograd-bf16views", "blhd", 2, 2, 65, 64, (FLASH, True), "bf16", False, dtype=BF16, contiguous=False),
    row("blhd-bf16-nograd-bf16views-D48", "blhd", 2, 2, 16, 48, (BLOCK, False), "bf16", False, dtype=BF16, contiguous=False),    # bf16 views off the fused shapes: widened to fp32
    row("blhd-bf16-nograd-bf16views-L129-D48", "blhd", 2, 2, 129, 48, (LONG, False), "bf16", False, dtype=BF16, contiguous=False),
    row("blhd-bf16-nograd-bias", "blhd", 2, 2, 65, 32, (FLASH, True), "bf16", False, "bias", contiguous=False),
    row("blhd-bf16-grad-L65", "blhd", 2, 2, 65, 64, (FLASH_TRAIN, False), "bf16", contiguous=False),
    row("blhd-bf16-grad-L64", "blhd", 2, 2, 64, 64, (ROWS, False), "bf16", contiguous=False),
    row("blhd-f32-L64", "blhd", 2, 2, 64, 32, (ROWS, False), contiguous=False),
    row("blhd-f32-L65", "blhd", 2, 2, 65, 32, (BLOCK, False), contiguous=False),
    row("blhd-f32-mask", "blhd", 2, 2, 16, 32, (LONG, False), extras="mask", contiguous=False),
    # ---- packed [B, L, 3, H, Dh]: ROWS in place, else the [B, L, H, Dh] rule on the three views
    row("packed-f32-L49-D32", "packed", 2, 2, 49, 32, (ROWS, True)),                               # DaViT / CAFormer window attention with gradients
    row("packed-f32-L64-D64", "packed", 2, 2, 64, 64, (ROWS, True)),                               # L <= 64 at its edge
    row("packed-f32-L65-D32", "packed", 2, 2, 65, 32, (BLOCK, False)),                             # L <= 64 fails
    row("packed-f32-L16-D48", "packed", 2, 2, 16, 48, (BLOCK, False)),                             # Dh in {32, 64} fails
    row("packed-f32-nograd-L49", "packed", 2, 2, 49, 32, (ROWS, True), grad=False),
    row("packed-f32-slice", "packed", 2, 2, 49, 32, (ROWS, False), contiguous=False),              # a non-contiguous slice: the rows kernels through copies
    row("packed-f32-mask", "packed", 2, 2, 16, 32, (LONG, False), extras="mask"),
    row("packed-f32-bias", "packed", 2, 2, 16, 32, (LONG, False), extras="bias"),
    row("packed-f32-causal", "packed", 2, 2, 16, 32, (LONG, False), extras="causal"),
    row("packed-f32-cpu", "packed", 2, 2, 16, 32, (ROWS, False), gpu=False, on_device=False),      # on device fails: the views, then the Function raises
    row("packed-bf16-nograd-L49", "packed", 2, 2, 49, 32, (FLASH, True), "bf16", False),           # the FLASH predicate holds on the views: not ROWS
    row("packed-bf16-nograd-slice", "packed", 2, 2, 49, 32, (FLASH, True), "bf16", False, contiguous=False),
    row("packed-bf16-nograd-strided", "packed", 2, 2, 49, 32, (FLASH, False), "bf16", False, gpu=False, contiguous=False, unit_stride=False, aligned=False),   # no unit last stride: neither in place, FLASH on the copies
    row("packed-bf16-grad-L49", "packed", 2, 2, 49, 32, (ROWS, True), "bf16"),                     # gradients fail FLASH, L <= 64 fails FLASH_TRAIN
    row("packed-bf16-grad-L65", "packed", 2, 2, 65, 32, (FLASH_TRAIN, False), "bf16"),
    row("packed-bf16-grad-L65-bwd0", "packed", 2, 2, 65, 32, (BLOCK, False), "bf16", flash_bwd="0"),
    row("packed-bf16-nograd-bf16-L16-D32", "packed", 2, 2, 16, 32, (FLASH, True), "bf16", False, dtype=BF16),
    row("packed-bf16-nograd-bf16-L16-D48", "packed", 2, 2, 16, 48, (BLOCK, False), "bf16", False, dtype=BF16),    # bf16 tensor off the fused shapes
    row("packed-bf16-nograd-BH65535", "packed", 21845, 3, 2, 32, (FLASH, True), "bf16", False),    # B * H <= 65535 at its edge
    row("packed-bf16-nograd-BH65536", "packed", 16384, 4, 2, 32, (ROWS, True), "bf16", False),     # the grid limit: the rows kernels in place
]

GPU_CASES = [c for c in ROUTE_CASES if c[3]]


def case_id(case):
    return case[0]


def entry_points(family, grad, bias_grad):
    """the C entry points a family runs, forward then backward, in order"""
    fwd = {FLASH: ["mmskin_flash_attention_forward"], FLASH_TRAIN: ["mmskin_flash_attention_forward"], ROWS: ["mmskin_attention_rows_forward"],
           BLOCK: ["mmskin_attention_forward"], LONG: ["mmskin_bmm", "mmskin_softmax_forward", "mmskin_bmm"]}[family]
    if not grad:
        return fwd
    bwd = {FLASH_TRAIN: ["mmskin_flash_attention_backward"], ROWS: ["mmskin_attention_rows_backward"], BLOCK: ["mmskin_attention_backward"],
           LONG: ["mmskin_bmm", "mmskin_bmm", "mmskin_softmax_backward", "mmskin_bmm", "mmskin_bmm"]}[family]
    return fwd + bwd + (["mmskin_colsum"] if bias_grad else [])


def make_inputs(case):
    """The tensors of a row on the CPU: (qkv [B, L, 3, H, Dh] holding values the row's dtype represents exactly, mask_add, bias, causal, dO
    [B, L, H, Dh]).  Every layout is cut from the same packed tensor."""
    cid, a, extras, _, _ = case
    B, H, L, Dh = a["B"], a["H"], a["L"], a["Dh"]
    g = torch.Generator().manual_seed(L * 131 + Dh * 7 + H)
    qkv = torch.randn(B, L, 3, H, Dh, generator=g)
    if a["dtype"] != F32:
        qkv = qkv.to(a["dtype"]).float()
    dO = torch.randn(B, L, H, Dh, generator=g)
    mask = bias = None
    if extras == "mask":
        mask = torch.zeros(B, L)
        mask[0, L // 2:] = -10000.0
        mask[-1, L - 3:] = float("-inf")
    if extras == "bias":
        bias = torch.randn(H, L, L, generator=g)
    return qkv, mask, bias, extras == "causal", dO


def device_tensors(case, qkv, dev):
    """qkv on the device in the layout, dtype and memory format the row describes -> (entry point name, its tensor arguments, a function
    that returns d(qkv) [B, L, 3, H, Dh] after a backward pass).  The leaves require gradients when the row does."""
    cid, a, _, _, _ = case
    B, H, L, Dh = a["B"], a["H"], a["L"], a["Dh"]
    t = qkv.to(a["dtype"])
    leaf = lambda x: x.to(dev, copy=True).requires_grad_(a["grad"])
    if a["layout"] == "packed":
        if a.get("contiguous", True):
            x = leaf(t)
            return "attention_packed", [x], lambda: x.grad
        wide = leaf(torch.cat([t, t], 3))                      # [B, L, 3, 2H, Dh]: the first H heads are a strided slice
        return "attention_packed", [wide[:, :, :, :H]], lambda: wide.grad[:, :, :, :H]
    if a["layout"] == "blhd" and a.get("aligned", True):
        x = leaf(t)
        return "attention_blhd", [x[:, :, 0], x[:, :, 1], x[:, :, 2]], lambda: x.grad
    if a["layout"] == "blhd":                                  # contiguous [B, L, H, Dh], each one element past a 16-byte boundary
        xs = [leaf(t[:, :, i].contiguous()) for i in range(3)]
        pad = torch.zeros(1, dtype=t.dtype, device=dev)
        views = [torch.cat([pad, x.flatten(), pad])[1:1 + x.numel()].view(B, L, H, Dh) for x in xs]
        assert all(v.data_ptr() % 16 != 0 for v in views)
        return "attention_blhd", views, lambda: torch.stack([x.grad for x in xs], 2)
    if a.get("unit_stride", True):
        xs = [leaf(t[:, :, i].permute(0, 2, 1, 3).contiguous()) for i in range(3)]
        return "attention", xs, lambda: torch.stack([x.grad.permute(0, 2, 1, 3) for x in xs], 2)
    xs = []
    for i in range(3):                                         # every second element of a [B, H, L, 2 Dh] tensor
        two = torch.zeros(B, H, L, 2 * Dh, dtype=t.dtype)
        two[..., ::2] = t[:, :, i].permute(0, 2, 1, 3)
        xs.append(leaf(two))
    return "attention", [x[..., ::2] for x in xs], lambda: torch.stack([x.grad[..., ::2].permute(0, 2, 1, 3) for x in xs], 2)


def reference(qkv, mask, bias, causal, dO, rounded=False):
    """fp64 attention on the CPU -> (out [B, L, H, Dh], d(qkv), d(bias) or None).  rounded: the forward with exactly what the fused bf16
    kernel rounds (q, k, v and the un-normalised probabilities relative to the row maximum) -- (out, None, None)."""
    rb = (lambda t: t.bfloat16().double()) if rounded else (lambda t: t)
    x = qkv.double().requires_grad_(not rounded)
    b = bias.double().requires_grad_(not rounded) if bias is not None else None
    q, k, v = (rb(x[:, :, i]).permute(0, 2, 1, 3) for i in range(3))
    L, Dh = q.shape[2], q.shape[3]
    s = q @ k.transpose(-1, -2) / math.sqrt(Dh)
    if b is not None:
        s = s + b[None]
    if mask is not None:
        s = s + mask.double()[:, None, None, :]
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(L, L, dtype=torch.bool), 1), float("-inf"))
    if rounded:
        e = torch.exp(s - s.amax(-1, keepdim=True))
        return ((rb(e.float()) @ v) / e.sum(-1, keepdim=True)).permute(0, 2, 1, 3).detach(), None, None
    out = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3)
    out.backward(dO.double())
    return out.detach(), x.grad, (b.grad if b is not None else None)
