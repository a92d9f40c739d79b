"""CoaT-Lite encoders through the reference's generic timm branch (loadImageModelClassifier.py:117-152): module tree, state_dict with the
shared cpe / crpe alias keys, parameter counts and the freezing modes, against the CPU restatement in tests/coat_oracle.py.  No GPU
needed."""
import pytest

from coat_oracle import OracleCoaT

COUNTS = {"coat_lite_tiny": 5_400_960, "coat_lite_mini": 10_498_560, "coat_lite_small": 19_325_504, "coat_lite_medium": 44_058_048}


def _encoder(name, mode):
    from models.loadImageModelClassifier import loadModels
    return loadModels.loadModelImageEncoder(name, 512, mode)


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_coat_lite_matches_timm_layout(name):
    model, dim = _encoder(name, "unfrozen_weights")
    ref = OracleCoaT(name)
    assert dim == ref.num_features == model.num_features
    sd = model.state_dict()
    got = {k: tuple(v.shape) for k, v in sd.items()}
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    assert "serial_blocks1.0.factoratt_crpe.crpe.conv_list.2.bias" in got and "crpe1.conv_list.2.bias" in got
    assert sd["serial_blocks1.0.cpe.proj.weight"].data_ptr() == sd["cpe1.proj.weight"].data_ptr()
    assert sd["serial_blocks4.1.factoratt_crpe.crpe.conv_list.0.weight"].data_ptr() == sd["crpe4.conv_list.0.weight"].data_ptr()
    assert sum(p.numel() for p in model.parameters()) == COUNTS[name]
    assert sum(p.numel() for p in ref.parameters()) == COUNTS[name]
    assert [k for k, _ in model.named_parameters()] == [k for k, _ in ref.named_parameters()]
    assert [k for k, _ in model.named_children()] == [k for k, _ in ref.named_children()]
    assert [k for k, _ in model.named_children()][-2:] == ["head_drop", "head"]
    model.load_state_dict(ref.state_dict(), strict=True)


def test_coat_lite_small_freezing_modes():
    for mode in ("partial", "frozen_weights"):      # reference :135-140: the last child is the Identity head -> nothing to unfreeze
        model, dim = _encoder("coat_lite_small.in1k", mode)
        assert dim == 512
        assert not any(p.requires_grad for p in model.parameters()), mode
    model, dim = _encoder("coat_lite_small.in1k", "unfrozen_weights")
    assert dim == 512 and all(p.requires_grad for p in model.parameters())
    model, dim = _encoder("coat_lite_small.in1k", "last_layer_unfrozen_weights")
    assert dim == 512
    assert {k for k, p in model.named_parameters() if p.requires_grad} == {"norm4.weight", "norm4.bias"}


def test_coat_init_follows_timm():
    model, _ = _encoder("coat_lite_tiny", "unfrozen_weights")
    sd = model.state_dict()
    assert float(sd["serial_blocks2.0.factoratt_crpe.qkv.bias"].abs().max()) == 0.0
    assert float(sd["serial_blocks2.0.mlp.fc2.bias"].abs().max()) == 0.0
    assert 0.015 < float(sd["serial_blocks3.1.mlp.fc1.weight"].std()) < 0.025
    assert float(sd["serial_blocks3.1.mlp.fc1.weight"].abs().max()) <= 2.0
    assert 0.0 < float(sd["cls_token1"].std()) < 0.04
    assert model.patch_embed1.norm.eps == 1e-5 and model.serial_blocks1[0].norm1.eps == 1e-6 and model.norm4.eps == 1e-6


@pytest.mark.parametrize("name", ["coat_lite_xl", "coat_tiny", "coat_small.in1k"])
def test_coat_without_plan_raises(name):
    with pytest.raises(NotImplementedError):
        _encoder(name, "frozen_weights")


def test_multimodal_model_with_coat_lite_small():
    from models import multimodalIntraInterModal as M
    model = M.MultimodalModel(num_classes=6, num_heads=8, device="cpu", cnn_model_name="coat_lite_small.in1k",
                              text_model_name="one-hot-encoder", vocab_size=20, unfreeze_weights="unfrozen_weights",
                              attention_mecanism="att-intramodal+residual+cross-attention-metadados")
    assert model.cnn_dim_output == 512
