"""CPU restatement of timm 1.0.x CAFormer (metaformer.py) in timm's NCHW formulation with timm's module names, after
reset_classifier(0): the yardstick for models/hip_caformer.py (timm is absent: parity unpinned against timm itself).

The stem and downsample convolutions are written as F.unfold + F.linear, so tests/bf16_emulation.py rounds exactly the GEMMs the HIP
path rounds in bf16-operand mode (it rounds F.linear and unpadded kernel = stride convolutions: here the 1x1 convolutions).  In that
mode the HIP path also runs attention over more than 64 tokens on the fused bf16 kernels; `bf16_attention()` makes the restatement
round q, k, v and the probabilities (and their gradients) to bf16 there, which tests/bf16_emulation.py does not do."""
import contextlib

import torch
import torch.nn as nn
import torch.nn.functional as F

CONFIGS = {
    "caformer_s18": ((3, 3, 9, 3), (64, 128, 320, 512)),
    "caformer_s36": ((3, 12, 18, 3), (64, 128, 320, 512)),
    "caformer_m36": ((3, 12, 18, 3), (96, 192, 384, 576)),
    "caformer_b36": ((3, 12, 18, 3), (128, 256, 512, 768)),
}
EPS = 1e-6


class StarReLU(nn.Module):
    def __init__(self):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(1))
        self.bias = nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return self.scale * F.relu(x) ** 2 + self.bias


class Scale(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(dim))

    def forward(self, x):                 # channels last
        return x * self.scale


class LayerNormNoBias(nn.Module):         # over the last dim
    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        return F.layer_norm(x, (x.shape[-1],), self.weight, None, EPS)


class LayerNorm2dNoBias(LayerNormNoBias):  # over channels of NCHW
    def forward(self, x):
        return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), self.weight, None, EPS).permute(0, 3, 1, 2)


def _conv_as_linear(x, conv, k, stride, pad):
    B, _, H, W = x.shape
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cols = F.unfold(x, k, padding=pad, stride=stride).transpose(1, 2)          # [B, L, C*k*k], columns (c, ky, kx)
    y = F.linear(cols, conv.weight.flatten(1), conv.bias)
    return y.transpose(1, 2).reshape(B, -1, OH, OW)


class Stem(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.conv = nn.Conv2d(3, dim, 7, 4, 2)
        self.norm = LayerNorm2dNoBias(dim)

    def forward(self, x):
        return self.norm(_conv_as_linear(x, self.conv, 7, 4, 2))


class Downsampling(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.norm = LayerNorm2dNoBias(cin)
        self.conv = nn.Conv2d(cin, cout, 3, 2, 1)

    def forward(self, x):
        return _conv_as_linear(self.norm(x), self.conv, 3, 2, 1)


class SepConv(nn.Module):
    def __init__(self, dim):
        super().__init__()
        mid = 2 * dim
        self.pwconv1 = nn.Conv2d(dim, mid, 1, bias=False)
        self.act1 = StarReLU()
        self.dwconv = nn.Conv2d(mid, mid, 7, padding=3, groups=mid, bias=False)
        self.pwconv2 = nn.Conv2d(mid, dim, 1, bias=False)

    def forward(self, x):
        return self.pwconv2(self.dwconv(self.act1(self.pwconv1(x))))


class _RoundBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


_BF16_ATTENTION = [False]


@contextlib.contextmanager
def bf16_attention():
    _BF16_ATTENTION[0] = True
    try:
        yield
    finally:
        _BF16_ATTENTION[0] = False


class Attention(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.num_heads = dim // 32
        self.qkv = nn.Linear(dim, 3 * dim, bias=False)
        self.proj = nn.Linear(dim, dim, bias=False)

    def forward(self, x):                 # [B, H, W, C]
        B, H, W, C = x.shape
        N = H * W
        qkv = self.qkv(x.reshape(B, N, C)).reshape(B, N, 3, self.num_heads, 32).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        rb = _BF16_ATTENTION[0] and N > 64
        if rb:
            q, k, v = _RoundBf16.apply(q), _RoundBf16.apply(k), _RoundBf16.apply(v)
        a = ((q @ k.transpose(-2, -1)) * 32 ** -0.5).softmax(-1)
        if rb:
            a = _RoundBf16.apply(a)
        o = (a @ v).transpose(1, 2).reshape(B, N, C)
        return self.proj(o).reshape(B, H, W, C)


class Mlp(nn.Module):
    def __init__(self, dim, conv):
        super().__init__()
        self.fc1 = nn.Conv2d(dim, 4 * dim, 1, bias=False) if conv else nn.Linear(dim, 4 * dim, bias=False)
        self.act = StarReLU()
        self.fc2 = nn.Conv2d(4 * dim, dim, 1, bias=False) if conv else nn.Linear(4 * dim, dim, bias=False)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class ConvBlock(nn.Module):             # NCHW, no res_scale
    def __init__(self, dim):
        super().__init__()
        self.norm1 = LayerNorm2dNoBias(dim)
        self.token_mixer = SepConv(dim)
        self.norm2 = LayerNorm2dNoBias(dim)
        self.mlp = Mlp(dim, conv=True)

    def forward(self, x):
        x = x + self.token_mixer(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class AttnBlock(nn.Module):             # NHWC
    def __init__(self, dim):
        super().__init__()
        self.norm1 = LayerNormNoBias(dim)
        self.token_mixer = Attention(dim)
        self.res_scale1 = Scale(dim)
        self.norm2 = LayerNormNoBias(dim)
        self.mlp = Mlp(dim, conv=False)
        self.res_scale2 = Scale(dim)

    def forward(self, x):
        x = self.res_scale1(x) + self.token_mixer(self.norm1(x))
        return self.res_scale2(x) + self.mlp(self.norm2(x))


class Stage(nn.Module):
    def __init__(self, cin, cout, depth, attention, downsample):
        super().__init__()
        self.downsample = Downsampling(cin, cout) if downsample else nn.Identity()
        self.attention = attention
        blk = AttnBlock if attention else ConvBlock
        self.blocks = nn.Sequential(*[blk(cout) for _ in range(depth)])

    def forward(self, x):                 # NCHW in and out
        x = self.downsample(x)
        if self.attention:
            return self.blocks(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
        return self.blocks(x)


class Head(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.norm = nn.LayerNorm(dim, eps=EPS)


class OracleCAFormer(nn.Module):
    def __init__(self, name="caformer_s18"):
        super().__init__()
        depths, dims = CONFIGS[name.split(".")[0]]
        self.num_features = dims[-1]
        self.stem = Stem(dims[0])
        stages, cin = [], dims[0]
        for i in range(4):
            stages.append(Stage(cin, dims[i], depths[i], attention=i >= 2, downsample=i > 0))
            cin = dims[i]
        self.stages = nn.Sequential(*stages)
        self.head = Head(dims[-1])

    def forward(self, x):
        x = self.stages(self.stem(x.float()))
        return self.head.norm(x.mean((2, 3)))
