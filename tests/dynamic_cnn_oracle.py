"""Plain-torch CPU restatement of the reference's NAS model `DynamicCNN` (models/dynamicMultimodalmodel.py of the reference), written from
its behaviour, and the cases the CPU and GPU tests of the HIP drop-in share.  tests/golden/dynamic_cnn.json, recorded from the reference's
own class by tests/golden/gen_dynamic_cnn_golden.py, pins this restatement (keys, shapes, seeded initialisation, logits).

The model: a trunk `conv_block` of [Conv2d(k, pad k // 2, no bias) -> GroupNorm(8, C) -> ReLU] x layers_per_block per entry of `filters`,
each block followed by MaxPool2d(2, 2) when use_pooling, then AdaptiveAvgPool2d(1); a metadata MLP `text_fc`; Linear + LayerNorm
projections of both into common_dim; four MultiheadAttention modules on length-1 sequences that always run; and one of four heads chosen
by `attention_mecanism`."""
import torch
import torch.nn as nn

BRANCHES = ("no-metadata", "concatenation", "crossattention", "metablock")

# trunk cases of the plan tests: (filters, layers_per_block, use_pooling, (N, H, W))
TRUNK_CASES = (
    ((64, 128), 2, True, (2, 32, 32)),
    ((64, 128), 1, False, (2, 32, 32)),
    ((64, 128, 256), 2, True, (3, 36, 44)),    # 36 -> 18 -> 9 -> 4: an odd map is floored; H != W; ragged N
)
# the two configurations the fixture records (seed 1234, one forward at N = 2, 3 x 32 x 32)
GOLDEN_SEED = 1234
GOLDEN_CONFIGS = {
    "pooled-l2-concatenation": dict(config=dict(filters=[64, 128], layers_per_block=2, use_pooling=True, num_layers_text_fc=1,
                                                neurons_per_layer_size_of_text_fc=32, num_layers_fc_module=1,
                                                neurons_per_layer_size_of_fc_module=48),
                                    num_classes=6, attention_mecanism="concatenation", common_dim=64, vocab_size=20, text_encoder_dim_output=40),
    "unpooled-l1-metablock": dict(config=dict(filters=[64, 128], layers_per_block=1, use_pooling=False, num_layers_text_fc=2,
                                              neurons_per_layer_size_of_text_fc=24, num_layers_fc_module=2,
                                              neurons_per_layer_size_of_fc_module=32),
                                  num_classes=5, attention_mecanism="metablock", common_dim=64, vocab_size=20, text_encoder_dim_output=40),
}
# the full-model GPU test: every branch at N = 4, 3 x 32 x 32
MODEL_KW = dict(config=dict(filters=[64, 128], layers_per_block=2, use_pooling=True, num_layers_text_fc=1,
                            neurons_per_layer_size_of_text_fc=64, num_layers_fc_module=1, neurons_per_layer_size_of_fc_module=128),
                num_classes=6, common_dim=64, num_heads=8, vocab_size=20, text_encoder_dim_output=64)


def trunk_id(case):
    filters, layers, pool, (n, h, w) = case
    return "f%s-l%d-p%d-%dx%dx%d" % ("_".join(map(str, filters)), layers, int(pool), n, h, w)


def golden_inputs(vocab_size, n=2, hw=32):
    g = torch.Generator().manual_seed(GOLDEN_SEED + 1)
    return torch.randn(n, 3, hw, hw, generator=g), torch.randn(n, vocab_size, generator=g)


def make_trunk(filters, layers_per_block, use_pooling, kernel_size=3, in_channels=3):
    layers, cin = [], in_channels
    for f in filters:
        for _ in range(layers_per_block):
            layers += [nn.Conv2d(cin, f, kernel_size=kernel_size, padding=kernel_size // 2, bias=False), nn.GroupNorm(8, f), nn.ReLU()]
            cin = f
        if use_pooling:
            layers.append(nn.MaxPool2d(2, 2))
    return nn.Sequential(*layers)


class OracleTrunk(nn.Module):
    """conv_block followed by the global average: what the plan computes, [N, filters[-1]]"""

    def __init__(self, filters, layers_per_block, use_pooling):
        super().__init__()
        self.conv_block = make_trunk(filters, layers_per_block, use_pooling)

    def forward(self, x):
        return self.conv_block(x).mean(dim=(2, 3))


class OracleMetaBlock(nn.Module):
    def __init__(self, V_dim, U_dim):
        super().__init__()
        self.fb = nn.Sequential(nn.Linear(U_dim, V_dim), nn.LayerNorm(V_dim))
        self.gb = nn.Sequential(nn.Linear(U_dim, V_dim), nn.LayerNorm(V_dim))

    def forward(self, V, U):
        return torch.sigmoid(torch.tanh(V * self.fb(U)) + self.gb(U))


class OracleDynamicCNN(nn.Module):
    def __init__(self, config, in_channels=3, num_classes=10, attention_mecanism="concatenation", text_model_name="one-hot-encoder", n=2,
                 device="cpu", num_heads=8, common_dim=512, vocab_size=85, text_encoder_dim_output=512):
        super().__init__()
        self.attention_mecanism = attention_mecanism
        k = int(config.get("kernel_size", 3))
        n_text, w_text = int(config.get("num_layers_text_fc", 2)), int(config.get("neurons_per_layer_size_of_text_fc", 512))
        n_fc, w_fc = int(config.get("num_layers_fc_module", 2)), int(config.get("neurons_per_layer_size_of_fc_module", 1024))
        filters = config.get("filters", [64, 128, 256])
        # modules are created in the reference's order: the seeded default initialisation consumes the generator in that order
        self.conv_block = make_trunk(filters, int(config.get("layers_per_block", 2)), config.get("use_pooling", True), k, in_channels)
        self.global_pool = nn.AdaptiveAvgPool2d((1, 1))
        self.image_encoder = nn.Sequential(self.conv_block, self.global_pool)
        c_out = filters[-1]
        text = [nn.Linear(vocab_size, w_text), nn.ReLU()]
        for _ in range(n_text):
            text += [nn.Linear(w_text, w_text), nn.ReLU()]
        text.append(nn.Linear(w_text, text_encoder_dim_output))
        self.text_fc = nn.Sequential(*text)
        self.image_projector = nn.Linear(c_out, common_dim)
        self.text_projector = nn.Linear(text_encoder_dim_output, common_dim)
        self.ln_img = nn.LayerNorm(common_dim)
        self.ln_txt = nn.LayerNorm(common_dim)
        self.image_self_attention = nn.MultiheadAttention(common_dim, num_heads)
        self.text_self_attention = nn.MultiheadAttention(common_dim, num_heads)
        self.image_cross_attention = nn.MultiheadAttention(common_dim, num_heads)
        self.text_cross_attention = nn.MultiheadAttention(common_dim, num_heads)
        in_common = attention_mecanism == "att-intramodal+residual+cross-attention-metadados+metablock"
        self.meta_block = OracleMetaBlock(common_dim if in_common else c_out, common_dim if in_common else text_encoder_dim_output)
        fc = [nn.Linear(common_dim * (1 if attention_mecanism == "no-metadata" else n), w_fc), nn.LayerNorm(w_fc), nn.ReLU(), nn.Dropout(0.3)]
        for _ in range(n_fc):
            fc += [nn.Linear(w_fc, w_fc), nn.ReLU()]
        fc.append(nn.Linear(w_fc, num_classes))
        self.fc_fusion = nn.Sequential(*fc)
        self.fc_visual_only = nn.Linear(c_out, num_classes)

    def forward(self, image, text_metadata):
        img_feat = self.image_encoder(image).flatten(1)
        img_proj = self.ln_img(self.image_projector(img_feat))
        txt_feat = self.text_fc(text_metadata)
        txt_proj = self.ln_txt(self.text_projector(txt_feat))
        img_seq, txt_seq = img_proj.unsqueeze(0), txt_proj.unsqueeze(0)
        img_att, _ = self.image_self_attention(img_seq, img_seq, img_seq)
        txt_att, _ = self.text_self_attention(txt_seq, txt_seq, txt_seq)
        img_cross, _ = self.image_cross_attention(img_att, txt_att, txt_att)
        txt_cross, _ = self.text_cross_attention(txt_att, img_att, img_att)
        if self.attention_mecanism == "no-metadata":
            return self.fc_fusion(img_proj)
        if self.attention_mecanism in ("concatenation", "crossattention"):
            return self.fc_fusion(torch.cat([img_cross.squeeze(0), txt_cross.squeeze(0)], dim=1))
        if self.attention_mecanism == "metablock":
            return self.fc_visual_only(self.meta_block(img_feat, txt_feat))
        raise ValueError(f"Attention mechanism '{self.attention_mecanism}' not supported.")


def tensor_sums(state_dict):
    """name -> [sum, sum of |.|] in float64: what the fixture records of a seeded initialisation"""
    return {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in state_dict.items()}
