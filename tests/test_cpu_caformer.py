"""CAFormer encoders through the reference's generic timm branch (loadImageModelClassifier.py:117-152): module tree, state_dict,
parameter counts and "partial" unfreezing, against the CPU restatement in tests/caformer_oracle.py.  No GPU needed."""
import pytest

from caformer_oracle import OracleCAFormer


def _encoder(name, mode):
    from models.loadImageModelClassifier import loadModels
    return loadModels.loadModelImageEncoder(name, 512, mode)


def test_caformer_b36_partial_encoder_matches_timm_layout():
    model, dim = _encoder("caformer_b36.sail_in22k_ft_in1k", "partial")
    assert dim == 768 and model.num_features == 768
    ref = OracleCAFormer("caformer_b36")
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert list(got) == list(want)
    assert got == want
    assert sum(p.numel() for p in model.parameters()) == 93_312_102
    trainable = {k for k, p in model.named_parameters() if p.requires_grad}
    assert trainable and all(k.startswith("stages.3.") for k in trainable)
    assert trainable == {k for k in got if k.startswith("stages.3.")}
    model.load_state_dict(ref.state_dict(), strict=True)


@pytest.mark.parametrize("name,count", [("caformer_s18", 23_237_936), ("caformer_s36", 36_193_382), ("caformer_m36", 52_565_862)])
def test_caformer_parameter_counts(name, count):
    model, dim = _encoder(name, "unfrozen_weights")
    assert sum(p.numel() for p in model.parameters()) == count
    assert dim == OracleCAFormer(name).num_features
    assert all(p.requires_grad for p in model.parameters())


def test_caformer_layernorms_have_no_bias_except_head():
    model, _ = _encoder("caformer_s18", "frozen_weights")
    keys = set(model.state_dict())
    assert "head.norm.bias" in keys
    assert not any(k.endswith("norm.bias") or k.endswith("norm1.bias") or k.endswith("norm2.bias") for k in keys - {"head.norm.bias"})
    assert not any(p.requires_grad for p in model.parameters())


def test_caformer_unknown_size_raises():
    with pytest.raises(NotImplementedError):
        _encoder("caformer_xl99", "frozen_weights")


def test_multimodal_model_with_caformer_b36():
    from models import multimodalIntraInterModal as M
    model = M.MultimodalModel(num_classes=6, num_heads=8, device="cpu", cnn_model_name="caformer_b36.sail_in22k_ft_in1k",
                              text_model_name="one-hot-encoder", vocab_size=20, unfreeze_weights="unfrozen_weights",
                              attention_mecanism="att-intramodal+residual+cross-attention-metadados")
    assert model.cnn_dim_output == 768
