"""Swin Transformer encoders through the reference's generic timm branch (loadImageModelClassifier.py:117-152): module tree, state_dict,
parameter counts, freezing modes, init and the stochastic-depth schedule against the CPU restatement in tests/swin_oracle.py -- and that
restatement's shifted-window attention (roll, partition, index buffer, img_mask) against a formulation that never rolls, which pins the
reference the kernels of csrc/swin_attn.hip are held to.  No GPU needed."""
import pytest
import torch

from swin_oracle import OracleSwin, brute_force_shifted_window_attention, shifted_window_attention_fp64

# the published 28 288 354 / 49 606 258 / 87 768 224 minus the 1000-way head (768 * 1000 + 1000; 1024 * 1000 + 1000)
COUNTS = {"swin_tiny_patch4_window7_224": 27_519_354, "swin_small_patch4_window7_224": 48_837_258, "swin_base_patch4_window7_224": 86_743_224}
FEATURES = {"swin_tiny_patch4_window7_224": 768, "swin_small_patch4_window7_224": 768, "swin_base_patch4_window7_224": 1024}


def _encoder(name, mode):
    from models.loadImageModelClassifier import loadModels
    return loadModels.loadModelImageEncoder(name, 512, mode)


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_swin_matches_timm_layout(name):
    model, dim = _encoder(name, "unfrozen_weights")
    ref = OracleSwin(name)
    assert dim == ref.num_features == model.num_features == FEATURES[name]
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    assert got["layers.0.blocks.1.attn.relative_position_bias_table"] == (169, model.layers[0].blocks[1].attn.num_heads)
    assert got["layers.1.downsample.reduction.weight"] == (2 * got["patch_embed.norm.weight"][0], 4 * got["patch_embed.norm.weight"][0])
    assert "layers.1.downsample.reduction.bias" not in got and not any("relative_position_index" in k or "attn_mask" in k for k in got)
    assert not any(k.startswith("layers.0.downsample") for k in got)
    assert sum(p.numel() for p in model.parameters()) == COUNTS[name]
    assert sum(p.numel() for p in ref.parameters()) == COUNTS[name]
    assert [k for k, _ in model.named_parameters()] == [k for k, _ in ref.named_parameters()]
    assert [k for k, _ in model.named_children()] == [k for k, _ in ref.named_children()] == ["patch_embed", "layers", "norm", "head"]
    for a, b in ((model.layers[1], ref.layers[1]), (model.layers[1].blocks[1], ref.layers[1].blocks[1]), (model.layers[1].downsample, ref.layers[1].downsample)):
        assert [k for k, _ in a.named_children() if not k.startswith("drop")] == \
               [k for k, _ in b.named_children() if not k.startswith("drop")]
    assert [(b.window_size, b.shift_size) for b in model.layers[0].blocks] == [(7, (0, 0)), (7, (3, 3))]
    assert [(b.window_size, b.shift_size) for b in model.layers[3].blocks] == [(7, (0, 0)), (7, (0, 0))]       # 7 x 7 tokens: one window, no shift
    assert [(b.window_size, b.shift_size) for b in ref.layers[3].blocks] == [((7, 7), (0, 0)), ((7, 7), (0, 0))]
    assert model.norm.eps == model.layers[2].blocks[0].norm1.eps == model.patch_embed.norm.eps == 1e-5
    model.load_state_dict(ref.state_dict(), strict=True)


def test_swin_tag_suffix_and_other_sizes():
    from models.hip_swin import HipSwinTransformer
    model, dim = _encoder("swin_tiny_patch4_window7_224.ms_in1k", "frozen_weights")
    assert dim == 768
    m = HipSwinTransformer("swin_tiny_patch4_window7_224", img_size=128, window_size=4)
    assert [(b.window_size, b.shift_size) for b in m.layers[2].blocks[:2]] == [(4, (0, 0)), (4, (2, 2))]
    assert [(b.window_size, b.shift_size) for b in m.layers[3].blocks] == [(4, (0, 0)), (4, (0, 0))]
    assert m.layers[0].blocks[0].attn.relative_position_bias_table.shape == (49, 3)
    m.load_state_dict(OracleSwin("swin_tiny_patch4_window7_224", img_size=128, window_size=4).state_dict(), strict=True)
    m = HipSwinTransformer("swin_tiny_patch4_window7_224", img_size=(224, 448))         # 7 x 14 tokens at stage 3: columns shift, rows do not
    assert [(b.window_size, b.shift_size) for b in m.layers[3].blocks] == [(7, (0, 0)), (7, (0, 3))]
    ref = OracleSwin("swin_tiny_patch4_window7_224", img_size=(224, 448))
    assert [(b.window_size, b.shift_size) for b in ref.layers[3].blocks] == [((7, 7), (0, 0)), ((7, 7), (0, 3))]
    with pytest.raises(NotImplementedError):
        HipSwinTransformer("swin_tiny_patch4_window7_224", img_size=224, window_size=9)      # 81 tokens per window
    with pytest.raises(NotImplementedError):
        HipSwinTransformer("swin_tiny_patch4_window7_224", img_size=224, window_size=8)      # 28 x 28 tokens are not a multiple of 8


def test_swin_freezing_modes():
    name = "swin_tiny_patch4_window7_224"
    for mode in ("partial", "frozen_weights"):      # reference :135-140: no `stages` / `blocks`; the last child is the parameter-less head
        model, dim = _encoder(name, mode)
        assert dim == 768
        assert not any(p.requires_grad for p in model.parameters()), mode
    model, _ = _encoder(name, "unfrozen_weights")
    assert all(p.requires_grad for p in model.parameters())
    model, _ = _encoder(name, "last_layer_unfrozen_weights")
    assert {k for k, p in model.named_parameters() if p.requires_grad} == {"norm.weight", "norm.bias"}
    assert not hasattr(model, "stages") and not hasattr(model, "blocks") and not list(model.head.parameters())


def test_swin_init_follows_timm():
    model, _ = _encoder("swin_tiny_patch4_window7_224", "unfrozen_weights")
    sd = model.state_dict()
    tables = torch.cat([v.flatten() for k, v in sd.items() if k.endswith("relative_position_bias_table")])
    assert 0.015 < float(tables.std()) < 0.025 and float(tables.abs().max()) <= 2.0
    assert float(sd["layers.1.blocks.0.attn.qkv.bias"].abs().max()) == 0.0
    assert float(sd["layers.2.blocks.3.mlp.fc2.bias"].abs().max()) == 0.0
    assert 0.015 < float(sd["layers.2.blocks.3.mlp.fc1.weight"].std()) < 0.025
    assert 0.015 < float(sd["layers.2.downsample.reduction.weight"].std()) < 0.025


@pytest.mark.parametrize("name", ["swin_large_patch4_window12_384", "swinv2_tiny_window8_256", "swin_base_patch4_window12_384.ms_in22k"])
def test_swin_without_plan_raises(name):
    from models.hip_swin import HipSwinTransformer
    with pytest.raises(NotImplementedError, match="swin_tiny_patch4_window7_224"):
        _encoder(name, "frozen_weights")
    with pytest.raises(NotImplementedError):
        HipSwinTransformer(name)


def test_multimodal_model_with_swin_tiny():
    from models import multimodalIntraInterModal as M
    model = M.MultimodalModel(num_classes=6, num_heads=8, device="cpu", cnn_model_name="swin_tiny_patch4_window7_224",
                              text_model_name="one-hot-encoder", vocab_size=20, unfreeze_weights="unfrozen_weights",
                              attention_mecanism="att-intramodal+residual+cross-attention-metadados")
    assert model.cnn_dim_output == 768


def test_drop_path_follows_the_linear_schedule():
    from models.hip_swin import DropPath, HipSwinTransformer
    for rate in (0.1, 0.3):
        m = HipSwinTransformer("swin_tiny_patch4_window7_224", drop_path_rate=rate)
        blocks = [b for stage in m.layers for b in stage.blocks]
        probs = [b.drop_path1.drop_prob for b in blocks]
        assert len(blocks) == 12 and all(isinstance(b.drop_path1, DropPath) and isinstance(b.drop_path2, DropPath) for b in blocks)
        assert probs == [b.drop_path2.drop_prob for b in blocks]
        assert probs[0] == 0.0 and abs(probs[-1] - rate) < 1e-7
        assert all(abs(p - rate * i / 11) < 1e-6 for i, p in enumerate(probs))
        assert not list(blocks[3].drop_path1.parameters()) and not list(blocks[3].drop_path1.buffers())
    assert HipSwinTransformer("swin_tiny_patch4_window7_224").layers[3].blocks[1].drop_path2.drop_prob == pytest.approx(0.1)     # timm's Swin default
    x = torch.ones(64, 3, 5)
    dp = DropPath(0.25).train()
    y = dp(x)
    kept = torch.tensor(1.0) / 0.75
    assert bool(((y == 0) | (y == kept)).all()) and 0 < int((y[:, 0, 0] == 0).sum()) < 64
    assert bool((y == y[:, :1, :1]).all())          # one draw per sample
    assert torch.equal(dp.eval()(x), x) and torch.equal(DropPath(0.0).train()(x), x)


@pytest.mark.parametrize("Hp,Wp,ws,shift", [(14, 14, 7, 3), (8, 12, 4, 2), (7, 21, 7, 3), (7, 14, 7, (0, 3)), (14, 14, 7, 0)])
def test_oracle_attention_equals_a_formulation_that_never_rolls(Hp, Wp, ws, shift):
    """timm's way (roll, partition, relative_position_index, img_mask -> attn_mask, reverse, roll back) against: every token attends to
    the tokens whose rolled coordinates fall in its window, -100 across region ids.  fp64, to 1e-12."""
    g = torch.Generator().manual_seed(Hp * 100 + Wp)
    B, H, Dh = 2, 2, 8
    qkv = torch.randn(B, Hp, Wp, 3, H, Dh, generator=g, dtype=torch.float64)
    table = torch.randn((2 * ws - 1) ** 2, H, generator=g, dtype=torch.float64)
    a = shifted_window_attention_fp64(qkv, table, ws, shift)
    b = brute_force_shifted_window_attention(qkv, table, ws, shift)
    assert a.shape == b.shape == (B, Hp, Wp, H * Dh)
    assert float((a - b).abs().max()) <= 1e-12, float((a - b).abs().max())
    if shift:       # the mask matters: without it the wrapped regions mix
        c = brute_force_shifted_window_attention(qkv, table, ws, 0)
        assert float((a - c).abs().max()) > 1e-3


def test_swin_attention_workspace_bytes_is_host_arithmetic():
    """per-window partial table gradients [windows][(2 ws - 1)^2][H] floats + the fp64 reducer's 64 rows of doubles, each on a 256-byte
    boundary; -1 for a geometry the kernels refuse (no device needed)"""
    from mmskin import _lib
    lib = _lib.load()
    for B, Hp, Wp, ws, H in ((64, 56, 56, 7, 3), (2, 14, 14, 7, 6), (1, 8, 12, 4, 1), (3, 8, 8, 8, 2)):
        T, nwin = (2 * ws - 1) ** 2, B * (Hp // ws) * (Wp // ws)
        size = lib.mmskin_swin_attention_workspace_bytes(B, Hp, Wp, ws, H)
        assert size % 256 == 0 and size >= 4 * nwin * T * H + 8 * lib.mmskin_col_reduce_scratch_doubles(T * H)
        assert size < 4 * nwin * T * H + 8 * 64 * T * H + 512
        assert lib.mmskin_swin_attention_workspace_bytes(B + 1, Hp, Wp, ws, H) >= size
    for bad in ((1, 15, 14, 7, 3), (1, 14, 13, 7, 3), (1, 18, 18, 9, 3), (0, 14, 14, 7, 3), (1, 14, 14, 0, 3), (1, 14, 14, 7, 0)):
        assert lib.mmskin_swin_attention_workspace_bytes(*bad) == -1, bad
