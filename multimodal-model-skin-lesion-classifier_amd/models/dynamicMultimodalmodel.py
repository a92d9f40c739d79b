"""DynamicCNN on the HIP path -- drop-in for the reference's models/dynamicMultimodalmodel.py (the model its NAS scripts search over and
train: nas/optimization_train_process_pad_20*.py, nas/train_pad_20_optimized_model.py).

Same constructor, attribute names, state_dict keys / order and seeded default initialisation.  The trunk `conv_block`
([Conv2d -> GroupNorm(8, C) -> ReLU] x layers per filter, optional MaxPool2d(2, 2) per block) and `global_pool` run as ONE plan
(mmskin.backbone.HipDynamicCNNFeatures, csrc/dynamic_cnn.hip) that already returns the pooled [N, C] features; the head runs on the
Linear / LayerNorm / attention / MetaBlock kernels the other models use.

Supported trunks: kernel_size 3, every filter a multiple of 64 (at most 1024), filters[0] == 64; anything else raises
mmskin MMSkinError at the first forward (plan creation).  The LSTM controller and the search loop of the NAS scripts are host code
and stay in PyTorch.
"""
import os
import sys

import torch.nn as nn

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
for _p in (_PKG, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from metablock import MetaBlock  # noqa: E402
from mmskin import ops  # noqa: E402
from mmskin.backbone import HipDynamicCNNFeatures  # noqa: E402
from mmskin.nn import FusedAway, HipDropout, HipLayerNorm, HipLinear, HipMultiheadAttention  # noqa: E402


class DynamicCNN(nn.Module):
    def __init__(
        self,
        config: dict,
        in_channels: int = 3,
        num_classes: int = 10,
        attention_mecanism: str = "concatenation",
        text_model_name: str = "one-hot-encoder",
        n: int = 2,
        device: str = "cpu",
        num_heads: int = 8,
        common_dim: int = 512,
        vocab_size: int = 85,
        text_encoder_dim_output: int = 512
    ):
        super().__init__()
        self.config = config
        self.device = device
        self.text_encoder_dim_output = text_encoder_dim_output
        self.common_dim = common_dim
        self.attention_mecanism = attention_mecanism
        self.text_model_name = text_model_name
        self.num_heads = num_heads
        self.num_classes = num_classes
        self.n = n

        self.k = int(config.get("kernel_size", 3))
        self.num_layers_text_fc = int(config.get("num_layers_text_fc", 2))
        self.neurons_text = int(config.get("neurons_per_layer_size_of_text_fc", 512))
        self.num_layers_fc = int(config.get("num_layers_fc_module", 2))
        self.neurons_fc = int(config.get("neurons_per_layer_size_of_fc_module", 1024))

        # trunk: conv_block + global_pool in one plan; image_encoder.0 IS conv_block, so both key families alias as in the reference
        filters = config.get("filters", [64, 128, 256])
        self.conv_block = HipDynamicCNNFeatures(filters, int(config.get("layers_per_block", 2)), config.get("use_pooling", True),
                                                kernel_size=self.k, in_channels=in_channels)
        self.layers = list(self.conv_block.children())
        self.in_channels = filters[-1]
        self.global_pool = FusedAway("AdaptiveAvgPool2d((1, 1)) (inside the conv_block plan)")
        self.image_encoder = nn.Sequential(self.conv_block, self.global_pool)
        self.cnn_dim_output = filters[-1]

        text_layers = [HipLinear(vocab_size, self.neurons_text, fuse_relu=True), FusedAway("ReLU")]
        for _ in range(self.num_layers_text_fc):
            text_layers.extend([HipLinear(self.neurons_text, self.neurons_text, fuse_relu=True), FusedAway("ReLU")])
        text_layers.append(HipLinear(self.neurons_text, text_encoder_dim_output))
        self.text_fc = nn.Sequential(*text_layers)

        self.image_projector = HipLinear(self.cnn_dim_output, self.common_dim)
        self.text_projector = HipLinear(text_encoder_dim_output, self.common_dim)
        self.ln_img = HipLayerNorm(self.common_dim)
        self.ln_txt = HipLayerNorm(self.common_dim)

        mha = lambda: HipMultiheadAttention(embed_dim=self.common_dim, num_heads=self.num_heads, batch_first=False)
        self.image_self_attention = mha()
        self.text_self_attention = mha()
        self.image_cross_attention = mha()
        self.text_cross_attention = mha()

        in_common = self.attention_mecanism in ["att-intramodal+residual+cross-attention-metadados+metablock"]
        self.meta_block = MetaBlock(V_dim=self.common_dim if in_common else self.cnn_dim_output,
                                    U_dim=self.common_dim if in_common else self.text_encoder_dim_output)

        self.fc_fusion = self._build_fc_fusion(n=1 if attention_mecanism == "no-metadata" else self.n)
        self.fc_visual_only = HipLinear(self.cnn_dim_output, self.num_classes)

    # Linear-LayerNorm-ReLU-Dropout, num_layers_fc x (Linear-ReLU), Linear: the reference's indices, so the keys match
    def _build_fc_fusion(self, n=1):
        layers = [HipLinear(self.common_dim * n, self.neurons_fc), HipLayerNorm(self.neurons_fc, fuse_relu=True), FusedAway("ReLU"),
                  HipDropout(0.3)]
        for _ in range(self.num_layers_fc):
            layers.extend([HipLinear(self.neurons_fc, self.neurons_fc, fuse_relu=True), FusedAway("ReLU")])
        layers.append(HipLinear(self.neurons_fc, self.num_classes))
        return nn.Sequential(*layers)

    def forward(self, image, text_metadata):
        image = image.to(self.device)

        img_feat = self.image_encoder(image)             # (B, C): the plan's output is already pooled and flat
        img_feat = img_feat.view(img_feat.size(0), -1)
        img_proj = self.ln_img(self.image_projector(img_feat))
        img_seq = img_proj.unsqueeze(0)                  # (1, B, D)

        txt_feat = self.text_fc(text_metadata)           # (B, D_txt)
        txt_proj = self.ln_txt(self.text_projector(txt_feat))
        txt_seq = txt_proj.unsqueeze(0)

        # as in the reference, the four attentions run whatever the branch; a branch that ignores them leaves their parameters
        # without a gradient
        img_att, _ = self.image_self_attention(img_seq, img_seq, img_seq)
        txt_att, _ = self.text_self_attention(txt_seq, txt_seq, txt_seq)
        img_cross, _ = self.image_cross_attention(img_att, txt_att, txt_att)
        txt_cross, _ = self.text_cross_attention(txt_att, img_att, img_att)
        img_pooled = img_cross.squeeze(0)
        txt_pooled = txt_cross.squeeze(0)

        if self.attention_mecanism == "no-metadata":
            return self.fc_fusion(img_proj)
        elif self.attention_mecanism == "concatenation":
            return self.fc_fusion(ops.concat2(img_pooled, txt_pooled))
        elif self.attention_mecanism == "crossattention":
            return self.fc_fusion(ops.concat2(img_pooled, txt_pooled))
        elif self.attention_mecanism == "metablock":
            return self.fc_visual_only(self.meta_block(img_feat, txt_feat))
        else:
            raise ValueError(f"Attention mechanism '{self.attention_mecanism}' not supported.")
