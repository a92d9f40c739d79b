"""Swin Transformer image encoders on the HIP ops -- timm 1.0.x `swin_{tiny,small,base}_patch4_window7_224` (swin_transformer.py) as the
reference's generic timm branch builds them (loadImageModelClassifier.py:117-152: create_model(name) + reset_classifier(0)); the
reference's training script sweeps "swin-tiny" among its backbones (train_pad_20.py:516).

timm's `SwinTransformer` module tree / state_dict keys: patch_embed.{proj,norm}, layers.S.downsample.{norm,reduction} (stages 1-3; stage 0
has an Identity), layers.S.blocks.D.{norm1, attn.{relative_position_bias_table, qkv, proj}, norm2, mlp.{fc1, fc2}}, norm, head.
`relative_position_index` and `attn_mask` are non-persistent buffers in timm: no key, and here no tensor either.  Activations stay an
image-major token grid [B, H, W, C] throughout: the 4x4/4 patch embedding is patch columns + one Linear, and the token mixer -- window
attention over the cyclically shifted grid with the learned relative-position bias and the -100 region mask -- is ONE fused op on the
packed qkv where the tokens sit (ops.swin_window_attention, fp32 in both Linear dtypes): no roll, no window partition / reverse, no index
or mask tensor.  Patch merging is a strided gather, a LayerNorm and a Linear.  Stochastic depth (timm's Swin default drop_path_rate 0.1,
linear per-block schedule) draws a per-sample keep mask with torch on the device.  Swin-V2 and the window-12 / 384 models have no plan.
PARITY UNPINNED against timm (absent); pinned against a CPU restatement in the tests.
"""
import os
import sys

import torch
import torch.nn as nn

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_PKG, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from mmskin import ops  # noqa: E402

SWIN_CONFIGS = {   # name: (embed_dim, depths, heads); head width 32 everywhere
    "swin_tiny_patch4_window7_224": (96, (2, 2, 6, 2), (3, 6, 12, 24)),
    "swin_small_patch4_window7_224": (96, (2, 2, 18, 2), (3, 6, 12, 24)),
    "swin_base_patch4_window7_224": (128, (2, 2, 18, 2), (4, 8, 16, 32)),
}


def _layernorm(mod, x2d):
    return ops.layernorm(x2d, mod.weight, mod.bias, mod.eps)


class DropPath(nn.Module):
    """stochastic depth per sample (timm DropPath, scale_by_keep): parameter-less; the mask is drawn by torch on the device"""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def active(self):
        return self.training and self.drop_prob > 0.0

    def forward(self, x):                          # [B, ...]
        if not self.active():
            return x
        keep = 1.0 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        return x * (mask / keep)

    def extra_repr(self):
        return f"drop_prob={self.drop_prob:.3f}"


class _PatchEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, 4, 4)
        self.norm = nn.LayerNorm(dim)

    def forward(self, x):                          # NCHW image -> [B, H / 4, W / 4, dim]
        B, _, H, W = x.shape
        y = ops.linear(ops.patch_cols(x, 4, 4, 0), self.proj.weight.flatten(1), self.proj.bias)
        return _layernorm(self.norm, y).reshape(B, H // 4, W // 4, -1)


class _WindowAttention(nn.Module):
    """parameters only: the attention runs in the block, on the token grid"""

    def __init__(self, dim, heads, ws):
        super().__init__()
        self.num_heads = heads
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * ws - 1) ** 2, heads))
        self.qkv = nn.Linear(dim, dim * 3)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)


class _Mlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1 = nn.Linear(dim, dim * 4)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(dim * 4, dim)

    def forward(self, x, residual=None):           # [residual +] fc2(gelu(fc1(x)))
        return ops.mlp(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, residual=residual)


class _SwinBlock(nn.Module):
    def __init__(self, dim, heads, ws, shift, drop_path):
        super().__init__()
        self.window_size, self.shift_size = ws, shift            # shift: (rows, columns), each 0 or ws // 2
        self.norm1 = nn.LayerNorm(dim)
        self.attn = _WindowAttention(dim, heads, ws)
        self.drop_path1 = DropPath(drop_path)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = _Mlp(dim)
        self.drop_path2 = DropPath(drop_path)

    def forward(self, x):                          # [B, H, W, C]
        B, H, W, C = x.shape
        a, heads = self.attn, self.attn.num_heads
        x2 = x.reshape(B * H * W, C)
        # qkv and proj are per-token Linears: they run on the un-rolled image-major grid, and the attention kernel finds each shifted
        # window's tokens where they sit
        qkv = ops.linear(_layernorm(self.norm1, x2), a.qkv.weight, a.qkv.bias).reshape(B, H, W, 3, heads, C // heads)
        o = ops.swin_window_attention(qkv, a.relative_position_bias_table, self.window_size, self.shift_size).reshape(B * H * W, C)
        if self.drop_path1.active():               # the branch alone, masked per sample, then the skip connection
            x2 = ops.add(x2, self.drop_path1(ops.linear(o, a.proj.weight, a.proj.bias).reshape(B, H * W, C)).reshape(B * H * W, C))
            x2 = ops.add(x2, self.drop_path2(self.mlp(_layernorm(self.norm2, x2)).reshape(B, H * W, C)).reshape(B * H * W, C))
        else:                                      # the skip connections ride on the output passes of proj and fc2
            x2 = ops.linear(o, a.proj.weight, a.proj.bias, residual=x2)
            x2 = self.mlp(_layernorm(self.norm2, x2), residual=x2)
        return x2.reshape(B, H, W, C)


class _PatchMerging(nn.Module):
    def __init__(self, dim, out_dim):
        super().__init__()
        self.norm = nn.LayerNorm(4 * dim)
        self.reduction = nn.Linear(4 * dim, out_dim, bias=False)

    def forward(self, x):                          # [B, H, W, C] -> [B, H / 2, W / 2, out_dim]
        B, H, W, C = x.shape
        # timm's channel order: (column parity, row parity, C).  A strided gather; not the hot path.
        x = x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5).reshape(B * (H // 2) * (W // 2), 4 * C)
        return ops.linear(_layernorm(self.norm, x), self.reduction.weight).reshape(B, H // 2, W // 2, -1)


class _Stage(nn.Module):
    def __init__(self, dim, out_dim, resolution, depth, downsample, heads, window, drop_path):
        super().__init__()
        self.downsample = _PatchMerging(dim, out_dim) if downsample else nn.Identity()
        # timm _calc_window_shift, per axis: an axis no longer than the window takes the whole axis as its window and is not shifted
        win = tuple(r if r <= window else window for r in resolution)
        if win[0] != win[1]:
            raise NotImplementedError(f"Swin stage of {resolution[0]} x {resolution[1]} tokens needs a {win[0]} x {win[1]} window: "
                                      "only square windows have MI355X kernels")
        ws = win[0]
        if ws * ws > 64 or resolution[0] % ws or resolution[1] % ws:
            raise NotImplementedError(f"Swin stage of {resolution[0]} x {resolution[1]} tokens with window {ws}: the MI355X kernels take "
                                      "windows of at most 64 tokens that tile the stage exactly (no padding)")
        shifts = [(0, 0) if i % 2 == 0 else tuple(0 if r <= ws else ws // 2 for r in resolution) for i in range(depth)]
        self.blocks = nn.Sequential(*[_SwinBlock(out_dim, heads, ws, shifts[i], drop_path[i]) for i in range(depth)])

    def forward(self, x):
        return self.blocks(self.downsample(x))


class _Head(nn.Module):
    """timm ClassifierHead after reset_classifier(0): average pool over the token grid, Identity fc -- no parameters"""

    def __init__(self):
        super().__init__()
        self.global_pool = nn.Identity()
        self.drop = nn.Dropout(0.0)
        self.fc = nn.Identity()
        self.flatten = nn.Identity()


class HipSwinTransformer(nn.Module):
    def __init__(self, name="swin_tiny_patch4_window7_224", img_size=224, window_size=7, drop_path_rate=0.1):
        super().__init__()
        key = name.split(".")[0]
        if key not in SWIN_CONFIGS:
            raise NotImplementedError(f"image encoder '{name}' has no MI355X kernels (available: {sorted(SWIN_CONFIGS)})")
        dim, depths, heads = SWIN_CONFIGS[key]
        img = (int(img_size), int(img_size)) if isinstance(img_size, int) else (int(img_size[0]), int(img_size[1]))
        if img[0] % 32 or img[1] % 32:
            raise ValueError(f"Swin needs an input height and width divisible by 32 (got {img})")
        self.img_size, self.window_size = img, int(window_size)
        self.num_features = dim * 8
        self.patch_embed = _PatchEmbed(dim)
        dpr = [r.tolist() for r in torch.linspace(0, drop_path_rate, sum(depths)).split(depths)]     # timm's linear schedule
        layers, cin = [], dim
        for i in range(4):
            cout = dim * 2 ** i
            res = (img[0] // 4 // 2 ** i, img[1] // 4 // 2 ** i)
            layers.append(_Stage(cin, cout, res, depths[i], i > 0, heads[i], self.window_size, dpr[i]))
            cin = cout
        self.layers = nn.Sequential(*layers)
        self.norm = nn.LayerNorm(self.num_features)
        self.head = _Head()                       # reset_classifier(0)
        for m in self.modules():                  # timm SwinTransformer.init_weights (the bias tables: _WindowAttention)
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward_features(self, image):            # -> [B, H / 32, W / 32, C], after the final norm
        x = image.float()
        if tuple(x.shape[2:]) != self.img_size:   # the windows and shifts of every stage were fixed by img_size, as in timm
            raise ValueError(f"this Swin encoder was built for {self.img_size[0]} x {self.img_size[1]} images (got {tuple(x.shape[2:])})")
        x = self.layers(self.patch_embed(x))
        B, H, W, C = x.shape
        return _layernorm(self.norm, x.reshape(B * H * W, C)).reshape(B, H, W, C)

    def forward(self, image):                     # reset_classifier(0): norm -> average pool -> Identity
        x = self.forward_features(image)
        B, H, W, C = x.shape
        return ops.token_mean(x.reshape(B, H * W, C), 0)
