"""CPU restatement of timm 1.0.x CoaT-Lite (coat.py, `coat_lite_*`: serial blocks only) with timm's module names, after
reset_classifier(0): the yardstick for models/hip_coat.py (timm is absent: parity unpinned against timm itself).

The patch embeddings are kernel = stride convolutions without padding, which tests/bf16_emulation.py rounds like the F.linear calls:
every GEMM the HIP path rounds in bf16-operand mode.  The attention and the depthwise convolutions are fp32 on both sides."""
import torch
import torch.nn as nn
import torch.nn.functional as F

CONFIGS = {   # name: (embed_dims, serial_depths, mlp_ratios)
    "coat_lite_tiny": ((64, 128, 256, 320), (2, 2, 2, 2), (8, 8, 4, 4)),
    "coat_lite_mini": ((64, 128, 320, 512), (2, 2, 2, 2), (8, 8, 4, 4)),
    "coat_lite_small": ((64, 128, 320, 512), (3, 4, 6, 3), (8, 8, 4, 4)),
    "coat_lite_medium": ((128, 256, 320, 512), (3, 6, 10, 8), (4, 4, 4, 4)),
}
NUM_HEADS = 8
CRPE_WINDOW = {3: 2, 5: 3, 7: 3}


class ConvRelPosEnc(nn.Module):
    def __init__(self, head_chs, num_heads, window):
        super().__init__()
        self.conv_list = nn.ModuleList()
        self.head_splits = []
        for cur_window, cur_split in window.items():
            self.conv_list.append(nn.Conv2d(cur_split * head_chs, cur_split * head_chs, cur_window, padding=cur_window // 2,
                                            groups=cur_split * head_chs))
            self.head_splits.append(cur_split)
        self.channel_splits = [x * head_chs for x in self.head_splits]

    def forward(self, q, v, size):
        B, num_heads, N, C = q.shape
        H, W = size
        q_img = q[:, :, 1:, :]
        v_img = v[:, :, 1:, :]
        v_img = v_img.transpose(-1, -2).reshape(B, num_heads * C, H, W)
        v_img_list = torch.split(v_img, self.channel_splits, dim=1)
        conv_v_img = torch.cat([conv(x) for conv, x in zip(self.conv_list, v_img_list)], dim=1)
        conv_v_img = conv_v_img.reshape(B, num_heads, C, H * W).transpose(-1, -2)
        return F.pad(q_img * conv_v_img, (0, 0, 1, 0, 0, 0))


class FactorAttnConvRelPosEnc(nn.Module):
    def __init__(self, dim, num_heads, shared_crpe):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3)
        self.proj = nn.Linear(dim, dim)
        self.crpe = shared_crpe

    def forward(self, x, size):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        k_softmax = k.softmax(dim=2)
        factor_att = k_softmax.transpose(-1, -2) @ v
        factor_att = q @ factor_att
        crpe = self.crpe(q, v, size=size)
        x = self.scale * factor_att + crpe
        return self.proj(x.transpose(1, 2).reshape(B, N, C))


class ConvPosEnc(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(dim, dim, 3, 1, 1, groups=dim)

    def forward(self, x, size):
        B, N, C = x.shape
        H, W = size
        cls_token, img_tokens = x[:, :1], x[:, 1:]
        feat = img_tokens.transpose(1, 2).view(B, C, H, W)
        x = self.proj(feat) + feat
        return torch.cat((cls_token, x.flatten(2).transpose(1, 2)), dim=1)


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class SerialBlock(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, shared_cpe, shared_crpe):
        super().__init__()
        self.cpe = shared_cpe
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.factoratt_crpe = FactorAttnConvRelPosEnc(dim, num_heads, shared_crpe)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    def forward(self, x, size):
        x = self.cpe(x, size)
        x = x + self.factoratt_crpe(self.norm1(x), size)
        return x + self.mlp(self.norm2(x))


class PatchEmbed(nn.Module):
    def __init__(self, patch, cin, dim):
        super().__init__()
        self.proj = nn.Conv2d(cin, dim, patch, patch)
        self.norm = nn.LayerNorm(dim)          # timm PatchEmbed(norm_layer=nn.LayerNorm): eps 1e-5

    def forward(self, x):
        x = self.proj(x)
        return self.norm(x.flatten(2).transpose(1, 2)), (x.shape[2], x.shape[3])


class OracleCoaT(nn.Module):
    def __init__(self, name="coat_lite_tiny"):
        super().__init__()
        dims, depths, ratios = CONFIGS[name.split(".")[0]]
        self.num_features = dims[-1]
        cin = 3
        for i in range(4):
            setattr(self, f"patch_embed{i + 1}", PatchEmbed(4 if i == 0 else 2, cin, dims[i]))
            cin = dims[i]
        for i in range(4):
            setattr(self, f"cls_token{i + 1}", nn.Parameter(torch.zeros(1, 1, dims[i])))
        for i in range(4):
            setattr(self, f"cpe{i + 1}", ConvPosEnc(dims[i]))
        for i in range(4):
            setattr(self, f"crpe{i + 1}", ConvRelPosEnc(dims[i] // NUM_HEADS, NUM_HEADS, CRPE_WINDOW))
        for i in range(4):
            cpe, crpe = getattr(self, f"cpe{i + 1}"), getattr(self, f"crpe{i + 1}")
            setattr(self, f"serial_blocks{i + 1}",
                    nn.ModuleList([SerialBlock(dims[i], NUM_HEADS, ratios[i], cpe, crpe) for _ in range(depths[i])]))
        self.norm2 = self.norm3 = None
        self.norm4 = nn.LayerNorm(dims[3], eps=1e-6)
        self.head_drop = nn.Dropout(0.0)
        self.head = nn.Identity()
        for i in range(4):
            nn.init.trunc_normal_(getattr(self, f"cls_token{i + 1}"), std=0.02)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        x = x.float()
        B = x.shape[0]
        for i in range(1, 5):
            x, size = getattr(self, f"patch_embed{i}")(x)
            x = torch.cat((getattr(self, f"cls_token{i}").expand(B, -1, -1), x), dim=1)
            for blk in getattr(self, f"serial_blocks{i}"):
                x = blk(x, size)
            if i < 4:
                x = x[:, 1:].reshape(B, size[0], size[1], -1).permute(0, 3, 1, 2).contiguous()
        return self.head(self.head_drop(self.norm4(x)[:, 0]))      # global_pool 'token'
