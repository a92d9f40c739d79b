"""CPU restatement of timm 1.0.x Swin Transformer (swin_transformer.py, `swin_*_patch4_window7_224`) with timm's module names, after
reset_classifier(0): the yardstick for models/hip_swin.py and for the shifted-window attention kernels (timm is absent: parity unpinned
against timm itself).  Written the timm way -- explicit torch.roll, window_partition / window_reverse, the relative_position_index buffer and
an img_mask-built attn_mask (both non-persistent buffers: no state_dict key).

The patch embedding is a kernel = stride convolution without padding, which tests/bf16_emulation.py rounds like the F.linear calls: every
GEMM the HIP path rounds in bf16-operand mode.  The attention is fp32 on both sides."""
import torch
import torch.nn as nn
import torch.nn.functional as F

CONFIGS = {   # name: (embed_dim, depths, heads)
    "swin_tiny_patch4_window7_224": (96, (2, 2, 6, 2), (3, 6, 12, 24)),
    "swin_small_patch4_window7_224": (96, (2, 2, 18, 2), (3, 6, 12, 24)),
    "swin_base_patch4_window7_224": (128, (2, 2, 18, 2), (4, 8, 16, 32)),
}


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def window_partition(x, ws):                                 # [B, H, W, C] -> [nW * B, ws0, ws1, C]
    B, H, W, C = x.shape
    x = x.view(B, H // ws[0], ws[0], W // ws[1], ws[1], C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws[0], ws[1], C)


def window_reverse(windows, ws, H, W):                       # [nW * B, ws0, ws1, C] -> [B, H, W, C]
    C = windows.shape[-1]
    x = windows.view(-1, H // ws[0], W // ws[1], ws[0], ws[1], C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, H, W, C)


def relative_position_index(win_h, win_w):
    coords = torch.stack(torch.meshgrid(torch.arange(win_h), torch.arange(win_w), indexing="ij")).flatten(1)     # [2, L]
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()                                 # [L, L, 2]
    rel[:, :, 0] += win_h - 1
    rel[:, :, 1] += win_w - 1
    rel[:, :, 0] *= 2 * win_w - 1
    return rel.sum(-1)


def attention_mask(H, W, ws, shift, dtype=torch.float32):
    """timm SwinTransformerBlock.get_attn_mask: [nW, L, L] of 0 / -100, or None without a shift"""
    if not any(shift):
        return None
    img_mask = torch.zeros((1, H, W, 1), dtype=dtype)
    cnt = 0
    for h in ((0, -ws[0]), (-ws[0], -shift[0]), (-shift[0], None)):
        for w in ((0, -ws[1]), (-ws[1], -shift[1]), (-shift[1], None)):
            img_mask[:, h[0]:h[1], w[0]:w[1], :] = cnt
            cnt += 1
    mask_windows = window_partition(img_mask, ws).view(-1, ws[0] * ws[1])
    attn_mask = mask_windows.unsqueeze(1) - mask_windows.unsqueeze(2)
    return attn_mask.masked_fill(attn_mask != 0, -100.0).masked_fill(attn_mask == 0, 0.0)


def shifted_window_attention_fp64(qkv, table, ws, shift):
    """timm SwinTransformerBlock._attn around WindowAttention.forward, without the qkv / proj Linears, in the dtype of its inputs:
    qkv [B, Hp, Wp, 3, H, Dh] (the qkv Linear applied per token, which commutes with roll and partition), table [(2 ws - 1)^2, H]
    -> [B, Hp, Wp, H * Dh].  shift: one int, or timm's per-axis pair."""
    B, Hp, Wp, _, H, Dh = qkv.shape
    ws, shift = _pair(ws), _pair(shift)
    L = ws[0] * ws[1]
    x = qkv.reshape(B, Hp, Wp, 3 * H * Dh)
    if any(shift):
        x = torch.roll(x, shifts=(-shift[0], -shift[1]), dims=(1, 2))
    xw = window_partition(x, ws).view(-1, L, 3, H, Dh).permute(2, 0, 3, 1, 4)                # [3, nW * B, H, L, Dh]
    q, k, v = xw.unbind(0)
    attn = (q * Dh ** -0.5) @ k.transpose(-2, -1)
    bias = table[relative_position_index(*ws).view(-1)].view(L, L, -1).permute(2, 0, 1).contiguous()
    attn = attn + bias.unsqueeze(0)
    mask = attention_mask(Hp, Wp, ws, shift, qkv.dtype)
    if mask is not None:
        nW = mask.shape[0]
        attn = attn.view(-1, nW, H, L, L) + mask.unsqueeze(1).unsqueeze(0)
        attn = attn.view(-1, H, L, L)
    attn = attn.softmax(dim=-1)
    o = (attn @ v).transpose(1, 2).reshape(-1, ws[0], ws[1], H * Dh)
    o = window_reverse(o, ws, Hp, Wp)
    if any(shift):
        o = torch.roll(o, shifts=shift, dims=(1, 2))
    return o


class WindowAttention(nn.Module):
    def __init__(self, dim, num_heads, window_size):
        super().__init__()
        self.num_heads, self.window_size = num_heads, window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size[0] - 1) * (2 * window_size[1] - 1), num_heads))
        self.qkv = nn.Linear(dim, dim * 3)
        self.attn_drop = nn.Dropout(0.0)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(0.0)
        self.softmax = nn.Softmax(dim=-1)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.drop1 = nn.Dropout(0.0)
        self.norm = nn.Identity()
        self.fc2 = nn.Linear(hidden, dim)
        self.drop2 = nn.Dropout(0.0)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class DropPath(nn.Module):
    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1.0 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        return x * mask / keep


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, resolution, num_heads, window_size, shift, drop_path):
        super().__init__()
        # timm _calc_window_shift: an axis no longer than the window takes the whole axis as its window and is not shifted
        self.window_size = tuple(r if r <= w else w for r, w in zip(resolution, window_size))
        self.shift_size = tuple(0 if r <= w else s for r, w, s in zip(resolution, self.window_size, shift))
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, num_heads, self.window_size)
        self.drop_path1 = DropPath(drop_path)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim, dim * 4)
        self.drop_path2 = DropPath(drop_path)

    def forward(self, x):                                    # [B, H, W, C]
        B, H, W, C = x.shape
        a = self.attn
        qkv = a.qkv(self.norm1(x)).reshape(B, H, W, 3, a.num_heads, C // a.num_heads)
        o = shifted_window_attention_fp64(qkv, a.relative_position_bias_table, self.window_size, self.shift_size)
        x = x + self.drop_path1(a.proj(o))
        x = x.reshape(B, -1, C)
        x = x + self.drop_path2(self.mlp(self.norm2(x)))
        return x.reshape(B, H, W, C)


class PatchMerging(nn.Module):
    def __init__(self, dim, out_dim):
        super().__init__()
        self.norm = nn.LayerNorm(4 * dim)
        self.reduction = nn.Linear(4 * dim, out_dim, bias=False)

    def forward(self, x):
        B, H, W, C = x.shape
        x = x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5).flatten(3)
        return self.reduction(self.norm(x))


class SwinTransformerStage(nn.Module):
    def __init__(self, dim, out_dim, resolution, depth, downsample, num_heads, window_size, drop_path):
        super().__init__()
        self.downsample = PatchMerging(dim, out_dim) if downsample else nn.Identity()
        ws = _pair(window_size)
        shift = tuple(w // 2 for w in ws)
        self.blocks = nn.Sequential(*[SwinTransformerBlock(out_dim, resolution, num_heads, ws, (0, 0) if i % 2 == 0 else shift, drop_path[i])
                                      for i in range(depth)])

    def forward(self, x):
        return self.blocks(self.downsample(x))


class PatchEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, 4, 4)
        self.norm = nn.LayerNorm(dim)

    def forward(self, x):
        return self.norm(self.proj(x).permute(0, 2, 3, 1))   # output_fmt NHWC


class ClassifierHead(nn.Module):
    """timm ClassifierHead after reset_classifier(0): average pool over the NHWC grid, no fc"""

    def __init__(self):
        super().__init__()
        self.global_pool = nn.Identity()
        self.drop = nn.Dropout(0.0)
        self.fc = nn.Identity()
        self.flatten = nn.Identity()

    def forward(self, x):
        return x.mean(dim=(1, 2))


class OracleSwin(nn.Module):
    def __init__(self, name="swin_tiny_patch4_window7_224", img_size=224, window_size=7, drop_path_rate=0.0):
        super().__init__()
        dim, depths, heads = CONFIGS[name.split(".")[0]]
        img = _pair(img_size)
        self.num_features = dim * 8
        self.patch_embed = PatchEmbed(dim)
        dpr = [r.tolist() for r in torch.linspace(0, drop_path_rate, sum(depths)).split(depths)]
        layers, cin = [], dim
        for i in range(4):
            cout = dim * 2 ** i
            res = (img[0] // 4 // 2 ** i, img[1] // 4 // 2 ** i)
            layers.append(SwinTransformerStage(cin, cout, res, depths[i], i > 0, heads[i], window_size, dpr[i]))
            cin = cout
        self.layers = nn.Sequential(*layers)
        self.norm = nn.LayerNorm(self.num_features)
        self.head = ClassifierHead()
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def forward(self, x):
        x = self.layers(self.patch_embed(x.float()))
        return self.head(self.norm(x))


def brute_force_shifted_window_attention(qkv, table, ws, shift):
    """The same attention without a roll: token (y, x) has rolled coordinates ((y - shift_y) mod Hp, (x - shift_x) mod Wp); it attends to
    the tokens whose rolled coordinates fall in its window, with the table entry of their relative position inside the window and -100
    between tokens of different region ids (the three slices per axis of the rolled image, an unshifted axis being one region)."""
    B, Hp, Wp, _, H, Dh = qkv.shape
    sy, sx = _pair(shift)
    ys, xs = torch.meshgrid(torch.arange(Hp), torch.arange(Wp), indexing="ij")
    ry, rx = ((ys - sy) % Hp).flatten(), ((xs - sx) % Wp).flatten()              # rolled coordinates of every token
    win = (ry // ws) * (Wp // ws) + rx // ws

    def region(r, n, s):
        return torch.zeros_like(r) if s == 0 else (r >= n - ws).long() + (r >= n - s).long()

    rid = region(ry, Hp, sy) * 3 + region(rx, Wp, sx)
    rel = (ry[:, None] % ws - ry[None, :] % ws + ws - 1) * (2 * ws - 1) + (rx[:, None] % ws - rx[None, :] % ws + ws - 1)    # [N, N]
    same = win[:, None] == win[None, :]
    q, k, v = qkv.reshape(B, Hp * Wp, 3, H, Dh).permute(2, 0, 3, 1, 4).unbind(0)                                              # [B, H, N, Dh]
    logits = (q * Dh ** -0.5) @ k.transpose(-2, -1) + table[rel.clamp(0, table.shape[0] - 1)].permute(2, 0, 1)
    logits = logits + torch.where(rid[:, None] != rid[None, :], -100.0, 0.0).to(qkv.dtype)
    logits = logits.masked_fill(~same, float("-inf"))
    return (logits.softmax(-1) @ v).transpose(1, 2).reshape(B, Hp, Wp, H * Dh)
