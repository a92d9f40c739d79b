"""Swin Transformer on the HIP path: the fused shifted-window attention kernels (csrc/swin_attn.hip) against the fp64 formulation written
the timm way in tests/swin_oracle.py (roll, partition, index buffer, img_mask; pinned there against a formulation that never rolls), and
the whole encoder against the CPU restatement (timm itself is absent).  Kernel tolerances are the sibling kernels'
(tests/test_gpu_davit_ops.py::_chk): 1e-4 of max(1, max|want|) for outputs, 2e-4 for gradients; encoder bounds are those of
test_gpu_coat.py."""
import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV, linear_mode, rel_err
from helpers import disable_dropout
from oracle.detinit import det_init_, det_inputs, det_tensor
from swin_oracle import OracleSwin, shifted_window_attention_fp64

pytestmark = pytest.mark.gpu

TINY = "swin_tiny_patch4_window7_224"


def _chk(a, b, tol=1e-4, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape
    err, ref = (a - b).abs().max().item(), max(1.0, b.abs().max().item())
    print(f"{what}: max err {err:.3e} / {ref:.3e} = {err / ref:.3e} (bound {tol:.0e})")
    assert err <= tol * ref, (what, err, ref)


def _inputs(B, Hp, Wp, ws, H, Dh, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, Hp, Wp, 3, H, Dh, generator=g)
    table = torch.randn((2 * ws - 1) ** 2, H, generator=g)          # O(1) entries: the bias moves the softmax as much as q . k does
    dO = torch.randn(B, Hp, Wp, H, Dh, generator=g)
    return qkv, table, dO


# (B, Hp, Wp, ws, shift, H, Dh): all four region patterns; a wrap inside a single window row; swin_tiny stage 0; ws 4 with Dh 64; ws 3;
# no shift; one window on three waves of a four-wave workgroup; the stage-3 head count; and timm's per-axis shift of a 7 x 14 stage
CASES = [(2, 14, 14, 7, 3, 3, 32), (1, 7, 21, 7, 3, 2, 32), (2, 56, 56, 7, 3, 3, 32), (3, 8, 12, 4, 2, 1, 64), (1, 6, 9, 3, 1, 5, 32),
         (2, 14, 14, 7, 0, 6, 32), (1, 7, 7, 7, 0, 3, 32), (2, 7, 7, 7, 0, 24, 32), (1, 7, 14, 7, (0, 3), 24, 32)]


@pytest.mark.parametrize("B,Hp,Wp,ws,shift,H,Dh", CASES)
def test_swin_window_attention_matches_fp64(B, Hp, Wp, ws, shift, H, Dh):
    from mmskin import ops
    qkv, table, dO = _inputs(B, Hp, Wp, ws, H, Dh, 31 * Hp + Wp + H)
    q_ref, t_ref = qkv.double().requires_grad_(True), table.double().requires_grad_(True)
    o_ref = shifted_window_attention_fp64(q_ref, t_ref, ws, shift)
    o_ref.backward(dO.double().reshape(o_ref.shape))
    q_dev, t_dev = qkv.to(DEV).requires_grad_(True), table.to(DEV).requires_grad_(True)
    assert ops.swin_window_attention_ok(q_dev, t_dev, ws, shift)
    o = ops.swin_window_attention(q_dev, t_dev, ws, shift)
    assert o.shape == (B, Hp, Wp, H, Dh) and o.is_contiguous()
    o.backward(dO.to(DEV))
    _chk(o.reshape(o_ref.shape), o_ref, 1e-4, "o")
    _chk(q_dev.grad, q_ref.grad, 2e-4, "dqkv")
    _chk(t_dev.grad, t_ref.grad, 2e-4, "dtable")


def test_swin_window_attention_without_shift_and_bias_is_window_attention():
    from mmskin import ops
    qkv, _, _ = _inputs(2, 14, 21, 7, 3, 32, 5)
    dev = qkv.to(DEV)
    want = ops.window_attention(dev, 7)
    got = ops.swin_window_attention(dev, torch.zeros(169, 3, device=DEV), 7, 0)
    err = float((got - want).abs().max())
    print(f"shift 0, zero table vs window_attention: max err {err:.3e} of {float(want.abs().max()):.3e}")
    assert err <= 1e-5 * float(want.abs().max())


def test_swin_window_attention_large_logits_stay_finite():
    """k scaled by 20: logits reach about +-60 before the -100 mask; the row maximum is subtracted before the exponential"""
    from mmskin import ops
    qkv, table, _ = _inputs(2, 14, 14, 7, 3, 32, 9)
    qkv[:, :, :, 1] *= 20.0
    logits = (qkv[:, :, :, 0].flatten(0, 2) * qkv[:, :, :, 1].flatten(0, 2)).sum(-1) * 32 ** -0.5
    assert float(logits.abs().max()) > 40.0
    o_ref = shifted_window_attention_fp64(qkv.double(), table.double(), 7, 3)
    o = ops.swin_window_attention(qkv.to(DEV), table.to(DEV), 7, 3)
    assert torch.isfinite(o).all()
    _chk(o.reshape(o_ref.shape), o_ref, 1e-4, "o (large logits)")


def test_swin_window_attention_backward_is_bitwise_repeatable():
    from mmskin import ops
    qkv, table, dO = _inputs(2, 28, 28, 7, 6, 32, 3)
    outs = []
    for _ in range(2):
        q, t = qkv.to(DEV).requires_grad_(True), table.to(DEV).requires_grad_(True)
        o = ops.swin_window_attention(q, t, 7, 3)
        o.backward(dO.to(DEV))
        outs.append((o.detach().clone(), q.grad.clone(), t.grad.clone()))
    for a, c in zip(*outs):
        assert torch.equal(a, c)


def test_swin_window_attention_dropout_mask_is_regenerated_in_backward():
    """The construction of test_window_attention_dropout_mask_is_regenerated_in_backward: o is linear in v, so with the forward's mask
    regenerated from (seed, offset) the gradient of sum(o * c) w.r.t. v is P'^T c and <dv, v> == sum(o * c)."""
    from mmskin import ops
    g = torch.Generator().manual_seed(11)
    qkv = torch.randn(2, 14, 7, 3, 2, 32, generator=g).to(DEV).requires_grad_(True)
    table = torch.randn(169, 2, generator=g).to(DEV).requires_grad_(True)
    c = torch.randn(2, 14, 7, 2, 32, generator=g).to(DEV)
    o = ops.swin_window_attention(qkv, table, 7, (3, 0), dropout_p=0.3, training=True)
    (o * c).sum().backward()
    lhs = (qkv.grad[:, :, :, 2] * qkv.detach()[:, :, :, 2]).sum().item()
    rhs = (o.detach() * c).sum().item()
    assert abs(lhs - rhs) <= 1e-3 * max(1.0, abs(rhs)), (lhs, rhs)
    o_eval = ops.swin_window_attention(qkv.detach(), table.detach(), 7, (3, 0), dropout_p=0.3, training=False)
    assert float((o_eval - o.detach()).abs().max()) > 1e-3          # the mask was applied


SENTINEL = -7.25


def _c_abi_forward(qkv, table, o, lse, Hp, Wp, ws, shift, H, Dh):
    from mmskin import _lib
    from mmskin._lib import call, ptr, stream
    from mmskin.attention import _qkv_ptrs
    call("mmskin_swin_attention_forward", *_qkv_ptrs(qkv), ptr(table), ptr(o), ptr(lse), qkv.shape[0], Hp, Wp, ws, shift, shift, H, Dh,
         3 * H * Dh, Dh, H * Dh, Dh, Dh ** -0.5, 0.0, 0, 0, stream())


@pytest.mark.parametrize("what,Hp,Wp,ws,shift,Dh", [("Hp % ws", 15, 14, 7, 3, 32), ("Wp % ws", 14, 13, 7, 3, 32), ("shift == ws", 14, 14, 7, 7, 32),
                                                    ("negative shift", 14, 14, 7, -1, 32), ("ws = 9", 18, 18, 9, 4, 32), ("Dh = 24", 14, 14, 7, 3, 24)])
def test_swin_window_attention_refuses_and_writes_nothing(what, Hp, Wp, ws, shift, Dh):
    """invalid ARGUMENTS only (every pointer is a live tensor of the size the arguments describe): an error, and no launch"""
    from mmskin import _lib, ops
    B, H = 1, 2
    qkv = torch.randn(B, Hp, Wp, 3, H, Dh, device=DEV)
    table = torch.zeros((2 * ws - 1) ** 2, H, device=DEV)
    o = torch.full((B, Hp, Wp, H, Dh), SENTINEL, device=DEV)
    lse = torch.full((B * (Hp // ws + 1) * (Wp // ws + 1), H, ws * ws), SENTINEL, device=DEV)
    with pytest.raises(_lib.MMSkinError):
        _c_abi_forward(qkv, table, o, lse, Hp, Wp, ws, shift, H, Dh)
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all()) and bool((lse == SENTINEL).all())
    assert not ops.swin_window_attention_ok(qkv, table, ws, shift)
    with pytest.raises(_lib.MMSkinError):
        ops.swin_window_attention(qkv, table, ws, shift)
    dq = torch.full_like(qkv, SENTINEL)
    dt = torch.full_like(table, SENTINEL)
    from mmskin._lib import call, ptr, stream
    from mmskin.attention import _qkv_ptrs
    wsp = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.MMSkinError):
        call("mmskin_swin_attention_backward", ptr(o), *_qkv_ptrs(qkv), ptr(table), ptr(o), ptr(lse), *_qkv_ptrs(dq), ptr(dt), ptr(wsp),
             B, Hp, Wp, ws, shift, shift, H, Dh, 3 * H * Dh, Dh, H * Dh, Dh, Dh ** -0.5, 0.0, 0, 0, stream())
    torch.cuda.synchronize()
    assert bool((dq == SENTINEL).all()) and bool((dt == SENTINEL).all())
    size = _lib.load().mmskin_swin_attention_workspace_bytes(B, Hp, Wp, ws, H)         # depends on the geometry alone
    assert size == -1 if what in ("Hp % ws", "Wp % ws", "ws = 9") else size > 0


def test_swin_window_attention_refuses_a_table_of_the_wrong_shape_and_bad_dropout():
    from mmskin import _lib, ops
    qkv = torch.randn(1, 14, 14, 3, 2, 32, device=DEV)
    for shape in ((169, 3), (168, 2), (2, 169), (49, 2)):
        table = torch.zeros(shape, device=DEV)
        assert not ops.swin_window_attention_ok(qkv, table, 7, 3)
        with pytest.raises(_lib.MMSkinError):
            ops.swin_window_attention(qkv, table, 7, 3)
    with pytest.raises(_lib.MMSkinError):
        ops.swin_window_attention(qkv, torch.zeros(169, 2, device=DEV), 7, 3, dropout_p=1.0, training=True)
    assert _lib.load().mmskin_swin_attention_workspace_bytes(2, 56, 56, 7, 3) >= 4 * 2 * 64 * 169 * 3


# ---- the encoder
def _pair(name=TINY, **kw):
    from models.hip_swin import HipSwinTransformer
    cpu = det_init_(OracleSwin(name, **kw))
    hip = HipSwinTransformer(name, drop_path_rate=0.0, **kw)
    hip.load_state_dict(cpu.state_dict(), strict=True)
    return cpu, hip.to(DEV)


def _run(m, x, w, dev, train=True):
    m.train(train)
    for p in m.parameters():
        p.grad = None
    f = m(x.to(dev))
    (f * w.to(dev)).sum().backward()
    return f.detach().cpu(), {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}


def _assert_grads_close(g_hip, g_cpu, tol=5e-3):
    assert set(g_hip) == set(g_cpu)
    scale = max(float(v.abs().max()) for v in g_cpu.values())
    bad = {}
    for k, g in g_cpu.items():
        err = float((g_hip[k] - g).abs().max())
        if err > tol * max(float(g.abs().max()), 1e-3 * scale):
            bad[k] = (err, float(g.abs().max()))
    assert not bad, dict(list(bad.items())[:8])


@pytest.mark.parametrize("B,kw", [(2, {}), (1, {"img_size": (224, 448)}), (2, {"img_size": 128, "window_size": 4})],
                         ids=["224", "224x448", "128-window4"])
def test_swin_tiny_matches_oracle(B, kw):
    cpu, hip = _pair(**kw)
    hw = kw.get("img_size", 224)
    hw = (hw, hw) if isinstance(hw, int) else hw
    x, w = det_tensor(f"swin.x.{hw}", (B, 3) + hw), det_tensor("swin.w", (B, cpu.num_features))
    f_cpu, g_cpu = _run(cpu, x, w, "cpu")
    f_hip, g_hip = _run(hip, x, w, DEV)
    print(f"swin_tiny {hw}: rel_err(features) = {rel_err(f_hip, f_cpu):.3e}")
    assert f_hip.shape == (B, 768)
    assert rel_err(f_hip, f_cpu) < 5e-4, rel_err(f_hip, f_cpu)
    tables = [k for k in g_cpu if k.endswith("relative_position_bias_table")]
    assert len(tables) == 12 and all(float(g_cpu[k].abs().max()) > 0 for k in tables)
    _assert_grads_close(g_hip, g_cpu)


def test_swin_tiny_bf16_operand_mode_vs_emulation():
    from bf16_emulation import assert_grads_not_worse_than_emulation, bf16_operand_emulation, grad_distance_report
    cpu, hip = _pair()
    x, w = det_tensor("swin.xb", (2, 3, 224, 224)), det_tensor("swin.wb", (2, 768))
    f_ref, g_ref = _run(cpu, x, w, "cpu")
    emu = det_init_(OracleSwin(TINY))
    with bf16_operand_emulation():
        f_emu, g_emu = _run(emu, x, w, "cpu")
    with linear_mode("bf16"):
        f_hip, g_hip = _run(hip, x, w, DEV)
    print(f"bf16: rel_err hip {rel_err(f_hip, f_ref):.3e}, emulation {rel_err(f_emu, f_ref):.3e}")
    assert rel_err(f_emu, f_ref) > 1e-4
    assert rel_err(f_hip, f_ref) <= 1.5 * rel_err(f_emu, f_ref) + 1e-3, (rel_err(f_hip, f_ref), rel_err(f_emu, f_ref))
    assert set(g_hip) == set(g_ref)
    rows = grad_distance_report(g_ref, g_hip, g_emu)
    worst = max(rows.items(), key=lambda kv: kv[1][0] / (kv[1][2] + 2e-3))
    print("bf16: worst gradient row (l2_hip, cos_hip, l2_emu, cos_emu):", worst)
    assert_grads_not_worse_than_emulation(rows)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_swin_small_frozen_no_grad(mode):
    from bf16_emulation import bf16_operand_emulation
    from models.loadImageModelClassifier import loadModels
    name = "swin_small_patch4_window7_224"
    cpu = det_init_(OracleSwin(name)).eval()
    hip, dim = loadModels.loadModelImageEncoder(name + ".ms_in1k", 512, "frozen_weights")
    hip.load_state_dict(cpu.state_dict(), strict=True)
    hip = hip.to(DEV).eval()
    x = det_tensor("swin.x3", (2, 3, 224, 224))
    with torch.no_grad():
        f_ref = cpu(x)
        if mode == "bf16":
            with bf16_operand_emulation():
                f_emu = cpu(x)
        with linear_mode(mode):
            f_hip = hip(x.to(DEV)).cpu()
    assert f_hip.shape == (2, 768) and dim == 768
    if mode == "fp32":
        assert rel_err(f_hip, f_ref) < 5e-4, rel_err(f_hip, f_ref)
    else:
        assert rel_err(f_hip, f_ref) <= 1.5 * rel_err(f_emu, f_ref) + 1e-3, (rel_err(f_hip, f_ref), rel_err(f_emu, f_ref))


def test_multimodal_swin_tiny_train_step():
    from models import multimodalIntraInterModal as M
    model = M.MultimodalModel(num_classes=6, num_heads=8, device=DEV, cnn_model_name=TINY, text_model_name="one-hot-encoder", vocab_size=20,
                              unfreeze_weights="unfrozen_weights",
                              attention_mecanism="att-intramodal+residual+cross-attention-metadados").to(DEV).train()
    disable_dropout(model)
    img, meta, lab = det_inputs(2, 224, 20, 6)
    out = model(img.to(DEV), meta.to(DEV))
    F.cross_entropy(out, lab.to(DEV)).backward()
    assert out.shape == (2, 6) and model.cnn_dim_output == 768
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.image_encoder.parameters())


def test_swin_tiny_drop_path_runs_and_changes_the_output():
    from models.hip_swin import HipSwinTransformer
    cpu = det_init_(OracleSwin(TINY))
    x = det_tensor("swin.xd", (8, 3, 224, 224)).to(DEV)
    outs = {}
    for rate in (0.0, 0.1):
        hip = HipSwinTransformer(TINY, drop_path_rate=rate)
        hip.load_state_dict(cpu.state_dict(), strict=True)
        hip = hip.to(DEV).train()
        torch.manual_seed(1)
        f = hip(x)
        f.sum().backward()
        assert torch.isfinite(f).all() and all(torch.isfinite(p.grad).all() for p in hip.parameters())
        outs[rate] = f.detach()
        if rate:        # eval mode: stochastic depth is off, the two encoders agree
            with torch.no_grad():
                assert float((hip.eval()(x) - outs[0.0]).abs().max()) <= 1e-4 * float(outs[0.0].abs().max())
    assert float((outs[0.1] - outs[0.0]).abs().max()) > 1e-3 * float(outs[0.0].abs().max())
