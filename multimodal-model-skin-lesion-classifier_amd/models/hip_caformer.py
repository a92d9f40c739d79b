"""CAFormer image encoders on the HIP ops -- timm 1.0.x `caformer_*` (metaformer.py) as the reference's generic timm branch builds it
(loadImageModelClassifier.py:117-152: create_model(name) + reset_classifier(0)); the reference's training driver uses
`caformer_b36.sail_in22k_ft_in1k`.

timm's `MetaFormer` module tree / state_dict keys: stem.{conv,norm}, stages.S.downsample.{norm,conv} (S >= 1), stages.S.blocks.D.*
with norm1 / token_mixer / [res_scale1] / norm2 / mlp / [res_scale2], head.norm.  Stages 0-1 mix tokens with SepConv (1x1 expand,
StarReLU, depthwise 7x7, 1x1 project; the MLP's 1x1 convolutions are Conv2d), stages 2-3 with multi-head attention (head dim 32) and
per-channel residual scales.  Every norm is a LayerNorm without bias (eps 1e-6) except head.norm.  Activations stay in token (NHWC)
layout throughout: 1x1 convolutions are Linear layers over the `weight.flatten(1)` views, channel LayerNorms are row LayerNorms, the
stem and downsample convolutions are patch columns + one Linear, and the StarReLU + depthwise 7x7 pair runs as one kernel each way
(ops.dw7_star).  PARITY UNPINNED against timm (absent); pinned against a CPU restatement in the tests.
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
from mmskin.nn import HipLayerNormNoBias  # noqa: E402

CAFORMER_CONFIGS = {   # name: (depths, dims)
    "caformer_s18": ((3, 3, 9, 3), (64, 128, 320, 512)),
    "caformer_s36": ((3, 12, 18, 3), (64, 128, 320, 512)),
    "caformer_m36": ((3, 12, 18, 3), (96, 192, 384, 576)),
    "caformer_b36": ((3, 12, 18, 3), (128, 256, 512, 768)),
}
EPS = 1e-6
HEAD_DIM = 32


def _ln(dim):
    return HipLayerNormNoBias(dim, eps=EPS)


class _StarReLU(nn.Module):
    """timm StarReLU parameters: scale * relu(x)^2 + bias (applied inside the fused kernels)."""

    def __init__(self):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(1))
        self.bias = nn.Parameter(torch.zeros(1))


class _Scale(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(dim))


class _SepConv(nn.Module):
    def __init__(self, dim):
        super().__init__()
        mid = 2 * dim
        self.pwconv1 = nn.Conv2d(dim, mid, 1, bias=False)
        self.act1 = _StarReLU()
        self.dwconv = nn.Conv2d(mid, mid, 7, padding=3, groups=mid, bias=False)
        self.pwconv2 = nn.Conv2d(mid, dim, 1, bias=False)

    def forward(self, h, B, H, W, residual):      # h [B*H*W, C] -> residual + pwconv2(dw7(act1(pwconv1(h))))
        z = ops.linear(h, self.pwconv1.weight.flatten(1)).reshape(B, H, W, -1)
        u = ops.dw7_star(z, self.dwconv.weight, self.act1.scale, self.act1.bias)
        return ops.linear(u.reshape(B * H * W, -1), self.pwconv2.weight.flatten(1), residual=residual)


class _Attention(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.num_heads = dim // HEAD_DIM
        self.qkv = nn.Linear(dim, 3 * dim, bias=False)
        self.proj = nn.Linear(dim, dim, bias=False)

    def forward(self, h, B, L):                   # h [B*L, C] -> proj(softmax(q k^T / sqrt(32)) v)
        C = h.shape[1]
        qkv = ops.linear(h, self.qkv.weight).reshape(B, L, 3, self.num_heads, HEAD_DIM)
        o = ops.attention_packed(qkv)                 # [B, L, heads, 32], token-major
        return ops.linear(o.reshape(B * L, C), self.proj.weight)


class _Mlp(nn.Module):
    def __init__(self, dim, conv):
        super().__init__()
        self.fc1 = nn.Conv2d(dim, 4 * dim, 1, bias=False) if conv else nn.Linear(dim, 4 * dim, bias=False)
        self.act = _StarReLU()
        self.fc2 = nn.Conv2d(4 * dim, dim, 1, bias=False) if conv else nn.Linear(4 * dim, dim, bias=False)

    def forward(self, h, residual=None):        # [residual +] fc2(StarReLU(fc1(h)))
        return ops.mlp(h, self.fc1.weight.flatten(1), None, self.fc2.weight.flatten(1), None, residual=residual,
                       star_relu=(self.act.scale, self.act.bias))


class _ConvBlock(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm1 = _ln(dim)
        self.token_mixer = _SepConv(dim)
        self.norm2 = _ln(dim)
        self.mlp = _Mlp(dim, conv=True)

    def forward(self, x):                         # [B, H, W, C]
        B, H, W, C = x.shape
        x2 = x.reshape(B * H * W, C)
        x2 = self.token_mixer(self.norm1(x2), B, H, W, residual=x2)
        return self.mlp(self.norm2(x2), residual=x2).reshape(B, H, W, C)


class _AttnBlock(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm1 = _ln(dim)
        self.token_mixer = _Attention(dim)
        self.res_scale1 = _Scale(dim)
        self.norm2 = _ln(dim)
        self.mlp = _Mlp(dim, conv=False)
        self.res_scale2 = _Scale(dim)

    def forward(self, x):                         # x = res_scale1 * x + attn(norm1(x)); x = res_scale2 * x + mlp(norm2(x))
        B, H, W, C = x.shape
        x2 = x.reshape(B * H * W, C)
        x2 = ops.scale_add(self.token_mixer(self.norm1(x2), B, H * W), x2, self.res_scale1.scale)
        x2 = ops.scale_add(self.mlp(self.norm2(x2)), x2, self.res_scale2.scale)
        return x2.reshape(B, H, W, C)


class _Stem(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.conv = nn.Conv2d(3, dim, 7, 4, 2)
        self.norm = _ln(dim)


class _Downsample(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.norm = _ln(cin)
        self.conv = nn.Conv2d(cin, cout, 3, 2, 1)


class _Stage(nn.Module):
    def __init__(self, cin, cout, depth, attention, downsample):
        super().__init__()
        self.downsample = _Downsample(cin, cout) if downsample else nn.Identity()
        blk = _AttnBlock if attention else _ConvBlock
        self.blocks = nn.Sequential(*[blk(cout) for _ in range(depth)])


class _Head(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm = nn.LayerNorm(dim, eps=EPS)     # timm LayerNorm2d with bias, over channels


class HipCAFormer(nn.Module):
    def __init__(self, name="caformer_s18"):
        super().__init__()
        key = name.split(".")[0]
        if key not in CAFORMER_CONFIGS:
            raise NotImplementedError(f"image encoder '{name}' has no MI355X kernels (available: {sorted(CAFORMER_CONFIGS)})")
        depths, dims = CAFORMER_CONFIGS[key]
        self.num_features = dims[-1]
        self.stem = _Stem(dims[0])
        stages, cin = [], dims[0]
        for i in range(4):
            stages.append(_Stage(cin, dims[i], depths[i], attention=i >= 2, downsample=i > 0))
            cin = dims[i]
        self.stages = nn.Sequential(*stages)
        self.head = _Head(dims[-1])
        for m in self.modules():              # timm MetaFormer._init_weights
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward_features(self, image):                                   # -> [B, H/32, W/32, C]
        x = image.float()
        B = x.shape[0]
        H, W = (x.shape[2] - 3) // 4 + 1, (x.shape[3] - 3) // 4 + 1       # 7x7 / 4, pad 2
        x = ops.linear(ops.patch_cols(x, 7, 4, 2), self.stem.conv.weight.flatten(1), self.stem.conv.bias)
        x = self.stem.norm(x).reshape(B, H, W, -1)
        for stage in self.stages:
            if not isinstance(stage.downsample, nn.Identity):
                ds = stage.downsample
                B, H, W, C = x.shape
                x = ds.norm(x.reshape(B * H * W, C)).reshape(B, H, W, C)
                p = ops.patch_cols(x, 3, 2, 1, channels_last=True)                                  # columns ordered (c, kh, kw)
                x = ops.linear(p, ds.conv.weight.flatten(1), ds.conv.bias).reshape(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, -1)
            x = stage.blocks(x)
        return x

    def forward(self, image):                                            # reset_classifier(0): avg pool -> head.norm -> flatten
        x = self.forward_features(image)
        B, H, W, C = x.shape
        pooled = ops.token_mean(x.reshape(B, H * W, C), 0)
        return ops.layernorm(pooled, self.head.norm.weight, self.head.norm.bias, EPS)
