"""CoaT-Lite image encoders on the HIP ops -- timm 1.0.x `coat_lite_*` (coat.py) as the reference's generic timm branch builds it
(loadImageModelClassifier.py:117-152: create_model(name) + reset_classifier(0)); the reference's training drivers use
`coat_lite_small.in1k`.

timm's `CoaT` module tree / state_dict keys: patch_embed{1..4}.{proj,norm}, cls_token{1..4}, cpe{1..4}.proj, crpe{1..4}.conv_list.{0,1,2},
serial_blocks{1..4}.D.{cpe, norm1, factoratt_crpe.{qkv, proj, crpe}, norm2, mlp.{fc1, fc2}}, norm4, head_drop, head.  A stage's blocks
share ONE cpe and ONE crpe module (the alias keys of timm checkpoints load with strict=True; parameters() yields each tensor once).
Activations stay token-major [B, 1 + H * W, C] with the class token at row 0: the patch embeddings are patch columns + one Linear, the
position encoding runs on the image rows in place (ops.conv_pos_enc_tokens), and the token mixer -- factorized attention with the
convolutional relative position encoding -- is one fused op on the packed qkv (ops.factor_attention, fp32 in both Linear dtypes).
The full `coat_*` models (parallel blocks) have no plan.  PARITY UNPINNED against timm (absent); pinned against a CPU restatement in
the tests.
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

COAT_CONFIGS = {   # name: (embed_dims, serial_depths, mlp_ratios)
    "coat_lite_tiny": ((64, 128, 256, 320), (2, 2, 2, 2), (8, 8, 4, 4)),
    "coat_lite_mini": ((64, 128, 320, 512), (2, 2, 2, 2), (8, 8, 4, 4)),
    "coat_lite_small": ((64, 128, 320, 512), (3, 4, 6, 3), (8, 8, 4, 4)),
    "coat_lite_medium": ((128, 256, 320, 512), (3, 6, 10, 8), (4, 4, 4, 4)),
}
NUM_HEADS = 8
CRPE_WINDOW = {3: 2, 5: 3, 7: 3}      # window: heads
EPS = 1e-6


def _layernorm(mod, x2d):
    return ops.layernorm(x2d, mod.weight, mod.bias, mod.eps)


class _PatchEmbed(nn.Module):
    def __init__(self, patch, cin, dim):
        super().__init__()
        self.patch = patch
        self.proj = nn.Conv2d(cin, dim, patch, patch)
        self.norm = nn.LayerNorm(dim)             # eps 1e-5 (timm PatchEmbed with norm_layer=nn.LayerNorm)

    def forward(self, x, channels_last):          # NCHW image or NHWC token grid -> [B * H * W, dim], (H, W)
        H, W = (x.shape[1], x.shape[2]) if channels_last else (x.shape[2], x.shape[3])
        cols = ops.patch_cols(x, self.patch, self.patch, 0, channels_last=channels_last)
        y = ops.linear(cols, self.proj.weight.flatten(1), self.proj.bias)
        return _layernorm(self.norm, y), (H // self.patch, W // self.patch)


class _ConvPosEnc(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(dim, dim, 3, 1, 1, groups=dim)

    def forward(self, x, size):                   # [B, 1 + H * W, C]: class row unchanged, image rows x + dwconv3(x) + bias
        return ops.conv_pos_enc_tokens(x, size[0], size[1], self.proj.weight, self.proj.bias)


class _ConvRelPosEnc(nn.Module):
    """parameters only: the convolutions run inside ops.factor_attention"""

    def __init__(self, head_chs):
        super().__init__()
        self.conv_list = nn.ModuleList(
            [nn.Conv2d(n * head_chs, n * head_chs, k, padding=k // 2, groups=n * head_chs) for k, n in CRPE_WINDOW.items()])


class _FactorAttnConvRelPosEnc(nn.Module):
    def __init__(self, dim, shared_crpe):
        super().__init__()
        self.qkv = nn.Linear(dim, dim * 3)
        self.proj = nn.Linear(dim, dim)
        self.crpe = shared_crpe

    def forward(self, h, B, size, residual):      # h [B * N, C] -> residual + proj(attention)
        C = h.shape[1]
        N = 1 + size[0] * size[1]
        qkv = ops.linear(h, self.qkv.weight, self.qkv.bias).reshape(B, N, 3, NUM_HEADS, C // NUM_HEADS)
        convs = self.crpe.conv_list
        att = ops.factor_attention(qkv, size[0], size[1], [c.weight for c in convs], [c.bias for c in convs])    # [B, N, C], token-major
        return ops.linear(att.reshape(B * N, C), self.proj.weight, self.proj.bias, residual=residual)


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x, residual=None):          # [residual +] fc2(gelu(fc1(x)))
        return ops.mlp(x, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, residual=residual)


class _SerialBlock(nn.Module):
    def __init__(self, dim, mlp_ratio, shared_cpe, shared_crpe):
        super().__init__()
        self.cpe = shared_cpe
        self.norm1 = nn.LayerNorm(dim, eps=EPS)
        self.factoratt_crpe = _FactorAttnConvRelPosEnc(dim, shared_crpe)
        self.norm2 = nn.LayerNorm(dim, eps=EPS)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))

    def forward(self, x, size):                   # [B, N, C]
        B, N, C = x.shape
        x2 = self.cpe(x, size).reshape(B * N, C)
        x2 = self.factoratt_crpe(_layernorm(self.norm1, x2), B, size, residual=x2)
        return self.mlp(_layernorm(self.norm2, x2), residual=x2).reshape(B, N, C)


class HipCoaT(nn.Module):
    def __init__(self, name="coat_lite_small"):
        super().__init__()
        key = name.split(".")[0]
        if key not in COAT_CONFIGS:
            raise NotImplementedError(f"image encoder '{name}' has no MI355X kernels (available: {sorted(COAT_CONFIGS)})")
        dims, depths, ratios = COAT_CONFIGS[key]
        self.num_features = dims[-1]
        cin = 3
        for i in range(4):                        # registration order = timm's = state_dict / parameters() order
            setattr(self, f"patch_embed{i + 1}", _PatchEmbed(4 if i == 0 else 2, cin, dims[i]))
            cin = dims[i]
        for i in range(4):
            setattr(self, f"cls_token{i + 1}", nn.Parameter(torch.zeros(1, 1, dims[i])))
        for i in range(4):
            setattr(self, f"cpe{i + 1}", _ConvPosEnc(dims[i]))
        for i in range(4):
            setattr(self, f"crpe{i + 1}", _ConvRelPosEnc(dims[i] // NUM_HEADS))
        for i in range(4):
            cpe, crpe = getattr(self, f"cpe{i + 1}"), getattr(self, f"crpe{i + 1}")
            setattr(self, f"serial_blocks{i + 1}", nn.ModuleList([_SerialBlock(dims[i], ratios[i], cpe, crpe) for _ in range(depths[i])]))
        self.norm2 = self.norm3 = None            # timm: only with return_interm_layers
        self.norm4 = nn.LayerNorm(dims[3], eps=EPS)
        self.head_drop = nn.Dropout(0.0)
        self.head = nn.Identity()                 # reset_classifier(0)
        for i in range(4):                        # timm CoaT.__init__ / _init_weights
            nn.init.trunc_normal_(getattr(self, f"cls_token{i + 1}"), std=0.02)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def forward_features(self, image):            # -> [B, 1 + H/32 * W/32, C_4], before norm4
        x = image.float()
        B = x.shape[0]
        if x.shape[2] % 32 or x.shape[3] % 32:
            raise ValueError(f"CoaT-Lite needs an input height and width divisible by 32 (got {tuple(x.shape[2:])})")
        for i in range(1, 5):
            tok, size = getattr(self, f"patch_embed{i}")(x, channels_last=i > 1)
            C = tok.shape[1]
            x = torch.cat((getattr(self, f"cls_token{i}").expand(B, -1, -1), tok.reshape(B, size[0] * size[1], C)), dim=1)
            for blk in getattr(self, f"serial_blocks{i}"):
                x = blk(x, size)
            if i < 4:
                x = x[:, 1:].reshape(B, size[0], size[1], C)       # image tokens as an NHWC grid for the next patch embedding
        return x

    def forward(self, image):                     # reset_classifier(0), global_pool 'token': norm4(x)[:, 0]
        x = self.forward_features(image)
        return _layernorm(self.norm4, x[:, 0].contiguous())      # a row LayerNorm: only the class rows are needed
