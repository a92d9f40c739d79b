"""No GPU: the DynamicCNN drop-in (models/dynamicMultimodalmodel.py), its trunk module (mmskin.backbone.HipDynamicCNNFeatures) and the
plan's host side (csrc/dynamic_cnn.hip: arch-string parsing, parameter table, refusals) against tests/golden/dynamic_cnn.json, which was
recorded from the reference's own class, and against the restatement of tests/dynamic_cnn_oracle.py."""
import ctypes
import json
import os

import pytest
import torch

import dynamic_cnn_oracle as do
from mmskin import _lib
from mmskin.backbone import HipDynamicCNNFeatures, dynamic_cnn_arch

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dynamic_cnn.json")) as f:
    GOLDEN = json.load(f)
ERR_ARG, ERR_UNSUPPORTED = 1, 3


def _seeded(cls, kw):
    torch.manual_seed(do.GOLDEN_SEED)
    return cls(**kw)


def _check_init(model, rec):
    sd = model.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == rec["keys"]
    sums = do.tensor_sums(sd)
    for k, (s, a) in rec["sums"].items():
        assert sums[k][0] == pytest.approx(s, rel=1e-12, abs=1e-12) and sums[k][1] == pytest.approx(a, rel=1e-12, abs=1e-12), k


@pytest.mark.parametrize("name", list(do.GOLDEN_CONFIGS))
def test_restatement_reproduces_the_reference(name):
    kw, rec = do.GOLDEN_CONFIGS[name], GOLDEN["configs"][name]
    assert GOLDEN["seed"] == do.GOLDEN_SEED
    m = _seeded(do.OracleDynamicCNN, kw).eval()
    _check_init(m, rec)
    img, meta = do.golden_inputs(kw["vocab_size"])
    with torch.no_grad():
        logits = m(img, meta).double()
    assert torch.allclose(logits, torch.tensor(rec["logits"], dtype=torch.float64), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", list(do.GOLDEN_CONFIGS))
def test_drop_in_has_the_reference_keys_shapes_and_seeded_init(name):
    from models.dynamicMultimodalmodel import DynamicCNN
    kw, rec = do.GOLDEN_CONFIGS[name], GOLDEN["configs"][name]
    hip = _seeded(DynamicCNN, kw)
    _check_init(hip, rec)
    cpu = do.OracleDynamicCNN(**kw)
    cpu.load_state_dict(hip.state_dict(), strict=True)
    hip2 = DynamicCNN(**kw)
    hip2.load_state_dict(cpu.state_dict(), strict=True)
    for (ka, a), (kb, b) in zip(hip.state_dict().items(), hip2.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka
    # image_encoder.0 is conv_block: the two key families alias one storage, as in the reference
    assert hip2.image_encoder[0] is hip2.conv_block
    assert hip2.state_dict()["image_encoder.0.0.weight"].data_ptr() == hip2.state_dict()["conv_block.0.weight"].data_ptr()


def test_drop_in_signature_and_unknown_branch():
    import inspect

    from models.dynamicMultimodalmodel import DynamicCNN
    sig = inspect.signature(DynamicCNN.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("config", inspect.Parameter.empty), ("in_channels", 3), ("num_classes", 10), ("attention_mecanism", "concatenation"),
        ("text_model_name", "one-hot-encoder"), ("n", 2), ("device", "cpu"), ("num_heads", 8), ("common_dim", 512), ("vocab_size", 85),
        ("text_encoder_dim_output", 512)]
    m = DynamicCNN(config={})
    assert m.conv_block.arch == "dynamic-cnn/64-128-256/l2/p1/k3" and m.cnn_dim_output == 256
    with pytest.raises(_lib.MMSkinError, match="in_channels"):
        DynamicCNN(config={}, in_channels=1)


@pytest.mark.parametrize("case", do.TRUNK_CASES, ids=do.trunk_id)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_plan_tensor_table_equals_named_parameters(case, dtype):
    filters, layers, pool, (n, h, w) = case
    m = HipDynamicCNNFeatures(filters, layers, pool, compute_dtype=dtype)
    ref = do.make_trunk(filters, layers, pool)
    assert [(k, tuple(p.shape)) for k, p in m.named_parameters()] == [(k, tuple(p.shape)) for k, p in ref.named_parameters()]
    plan = m._plan_for(n, h, w, None)              # raises when the C table disagrees with named_parameters()
    table = plan.tensor_table(0)
    assert [(t[0], t[3]) for t in table] == [(k, tuple(p.shape)) for k, p in m.named_parameters()]
    assert [t[1] for t in table] == [off for off, _, _ in m._layout]
    assert plan.tensor_table(1) == [] and plan.feat_dim == filters[-1] and plan.out_hw == (1, 1)
    assert plan.param_numel == sum(p.numel() for p in m.parameters()) and plan.ws_bytes > 0
    assert plan.grad_segments() == []
    flags = ctypes.c_int()
    lib = _lib.load()
    assert lib.mmskin_backbone_unit_flags(plan.handle, 0, ctypes.byref(flags)) == ERR_UNSUPPORTED and lib.mmskin_last_error()


def test_fused_tail_needs_less_workspace_than_the_unfused_one():
    lib = _lib.load()
    sizes = {}
    for tail in ("", "/t1", "/t0"):
        h = ctypes.c_void_p()
        assert lib.mmskin_backbone_create(b"dynamic-cnn/64-128/l2/p1/k3" + tail.encode(), 2, 32, 32, _lib.BF16, ctypes.byref(h)) == 0
        sizes[tail] = lib.mmskin_backbone_workspace_bytes(h)
        lib.mmskin_backbone_destroy(h)
    assert sizes[""] == sizes["/t1"]
    # what the fused tail does not store: the pooled activation (bf16) and its argmax bytes, N x 8 x 8 x 128 each, 256-byte aligned
    assert sizes["/t0"] - sizes[""] == 2 * 8 * 8 * 128 * 2 + 2 * 8 * 8 * 128


REFUSALS = [
    # arch, H, W, code, word the message must carry
    ("dynamic-cnn/64-128/l2/p1/k5", 32, 32, ERR_UNSUPPORTED, "kernel_size"),
    ("dynamic-cnn/64-96/l2/p1/k3", 32, 32, ERR_UNSUPPORTED, "filters"),
    ("dynamic-cnn/64-2048/l2/p1/k3", 32, 32, ERR_UNSUPPORTED, "filters"),
    ("dynamic-cnn/16-32/l2/p1/k3", 32, 32, ERR_UNSUPPORTED, "filters"),
    ("dynamic-cnn/128-256/l2/p1/k3", 32, 32, ERR_UNSUPPORTED, "filters[0]"),
    ("dynamic-cnn/64-128/l2/p1/k3", 256, 64, ERR_ARG, "height"),
    ("dynamic-cnn/64-128/l2/p1/k3", 64, 241, ERR_ARG, "width"),
    ("dynamic-cnn/64-64-64-64-64-64/l1/p1/k3", 32, 32, ERR_ARG, "use_pooling"),     # 32 -> 16 -> 8 -> 4 -> 2 -> 1, then a sixth pool
    ("dynamic-cnn//l2/p1/k3", 32, 32, ERR_ARG, "filters"),
    ("dynamic-cnn/64-128/l0/p1/k3", 32, 32, ERR_ARG, "layers_per_block"),
    ("dynamic-cnn/64-128/l2/p2/k3", 32, 32, ERR_ARG, "cannot read"),
    ("dynamic-cnn/64-128/l2/k3/p1", 32, 32, ERR_ARG, "cannot read"),
    ("dynamic-cnn/64-128-/l2/p1/k3", 32, 32, ERR_ARG, "cannot read"),
    ("dynamic-cnn/64x128/l2/p1/k3", 32, 32, ERR_ARG, "cannot read"),
    ("dynamic-cnn/64-128/l2/p1/k3/", 32, 32, ERR_ARG, "cannot read"),
    ("dynamic-cnn/64-128/l2/p1", 32, 32, ERR_ARG, "cannot read"),
]


@pytest.mark.parametrize("arch,H,W,code,word", REFUSALS, ids=[r[0] + "@%dx%d" % (r[1], r[2]) for r in REFUSALS])
def test_plan_refusals(arch, H, W, code, word):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.mmskin_backbone_create(arch.encode(), 2, H, W, _lib.F32, ctypes.byref(h)) == code
    assert not h.value
    msg = lib.mmskin_last_error().decode()
    assert msg and word in msg, msg


def test_unsupported_configuration_raises_when_the_first_plan_is_made():
    m = HipDynamicCNNFeatures([16, 32], 2, True)           # the NAS script's initial_filters: constructible, refused by the plan
    assert m.arch == dynamic_cnn_arch([16, 32], 2, True) == "dynamic-cnn/16-32/l2/p1/k3"
    with pytest.raises(_lib.MMSkinError, match="error 3"):
        m._plan_for(2, 32, 32, None)
    with pytest.raises(_lib.MMSkinError, match="error 3"):
        HipDynamicCNNFeatures([64, 128], 2, True, kernel_size=5)._plan_for(2, 32, 32, None)


def test_gap_workspace_bytes_refuses_what_the_unfused_entry_point_refuses():
    lib = _lib.load()
    for N, C, H, W, groups, pool in ((1, 96, 4, 4, 8, 0), (1, 64, 4, 4, 4, 1), (1, 32, 4, 4, 8, 0), (1, 64, 1, 4, 8, 1), (1, 2048, 4, 4, 8, 0),
                                     (0, 64, 4, 4, 8, 0), (1, 64, 4, 4, 8, 0), (3, 256, 7, 9, 8, 1), (1, 64, 1, 4, 8, 0), (2, 1024, 2, 2, 8, 1)):
        a = lib.mmskin_groupnorm8_relu_workspace_bytes(N, C, H, W, groups, pool)
        b = lib.mmskin_groupnorm8_relu_gap_workspace_bytes(N, C, H, W, groups, pool)
        assert (a == -1) == (b == -1), (N, C, H, W, groups, pool)
        if a > 0:
            assert 0 < b <= a      # no activation, argmax or gradient tensor to carve
