"""CoaT-Lite on the HIP path: the fused factorized-attention kernels (csrc/factor_attn.hip), the class-token-aware position encoding,
and the whole encoder against the CPU restatement in tests/coat_oracle.py (timm's formulation; timm itself is absent).
Kernel tolerances are the sibling kernels' (tests/test_gpu_davit_ops.py::_chk): 1e-4 of max(1, max|want|) for outputs, 2e-4 for
gradients; encoder bounds are those of test_gpu_caformer.py / test_gpu_davit.py."""
import pytest
import torch
import torch.nn.functional as F

from coat_oracle import OracleCoaT
from gpu_util import DEV, linear_mode, rel_err
from helpers import disable_dropout
from oracle.detinit import det_init_, det_inputs, det_tensor

pytestmark = pytest.mark.gpu

WINDOWS = ((3, 2), (5, 3), (7, 3))      # (window, heads)


def _chk(a, b, tol=1e-4, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape
    err, ref = (a - b).abs().max().item(), max(1.0, b.abs().max().item())
    print(f"{what}: max err {err:.3e} / {ref:.3e} = {err / ref:.3e} (bound {tol:.0e})")
    assert err <= tol * ref, (what, err, ref)


def _factor_attention_fp64(qkv, H, W, ws, bs):
    """timm FactorAttnConvRelPosEnc.forward (without qkv / proj) with explicit permutes and F.conv2d; qkv [B, N, 3, 8, Ch] -> [B, N, 8 * Ch]"""
    B, N, _, heads, Ch = qkv.shape
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)                       # [B, 8, N, Ch]
    fac = q @ (k.softmax(dim=2).transpose(-1, -2) @ v)
    v_img = v[:, :, 1:].transpose(-1, -2).reshape(B, heads * Ch, H, W)
    parts = torch.split(v_img, [n * Ch for _, n in WINDOWS], dim=1)
    conv = torch.cat([F.conv2d(p, w, b, padding=kk // 2, groups=p.shape[1]) for p, w, b, (kk, _) in zip(parts, ws, bs, WINDOWS)], dim=1)
    conv = conv.reshape(B, heads, Ch, H * W).transpose(-1, -2)
    crpe = F.pad(q[:, :, 1:] * conv, (0, 0, 1, 0, 0, 0))
    return (Ch ** -0.5 * fac + crpe).transpose(1, 2).reshape(B, N, heads * Ch)


def _fa_inputs(B, H, W, Ch, seed):
    g = torch.Generator().manual_seed(seed)
    N = 1 + H * W
    qkv = torch.randn(B, N, 3, 8, Ch, generator=g)
    ws = [torch.randn(n * Ch, 1, k, k, generator=g) / k for k, n in WINDOWS]
    bs = [torch.randn(n * Ch, generator=g) * 0.3 for _, n in WINDOWS]
    dO = torch.randn(B, N, 8 * Ch, generator=g)
    return qkv, ws, bs, dO


# the four stage shapes of coat_lite_small at 224 (H = 56 / 28 / 14 / 7, Ch = 8 / 16 / 40 / 64), Ch = 32, odd and non-square grids, a single
# pixel, and token counts that cross the 128-token chunk boundary by one (1 + 8 * 16 = 129, 1 + 16 * 16 = 257)
@pytest.mark.parametrize("B,H,W,Ch", [(2, 56, 56, 8), (2, 28, 28, 16), (2, 14, 14, 40), (2, 7, 7, 64), (2, 14, 14, 32), (2, 5, 9, 8),
                                      (3, 1, 1, 16), (1, 13, 17, 40), (2, 8, 16, 64), (1, 16, 16, 32), (1, 127, 1, 8), (2, 3, 43, 16)])
def test_factor_attention_matches_fp64(B, H, W, Ch):
    from mmskin import ops
    qkv, ws, bs, dO = _fa_inputs(B, H, W, Ch, 17 * H + W + Ch)
    ref_in = qkv.double().requires_grad_(True)
    ws_r = [t.double().requires_grad_(True) for t in ws]
    bs_r = [t.double().requires_grad_(True) for t in bs]
    y_ref = _factor_attention_fp64(ref_in, H, W, ws_r, bs_r)
    y_ref.backward(dO.double())
    dev = qkv.to(DEV).requires_grad_(True)
    ws_d = [t.to(DEV).requires_grad_(True) for t in ws]
    bs_d = [t.to(DEV).requires_grad_(True) for t in bs]
    y = ops.factor_attention(dev, H, W, ws_d, bs_d)
    assert y.shape == (B, 1 + H * W, 8 * Ch) and y.is_contiguous()
    y.backward(dO.to(DEV))
    _chk(y, y_ref, 1e-4, "att")
    _chk(dev.grad, ref_in.grad, 2e-4, "dqkv")
    for (k, _), wd, wr, bd, br in zip(WINDOWS, ws_d, ws_r, bs_d, bs_r):
        _chk(wd.grad, wr.grad, 2e-4, f"dw{k}")
        _chk(bd.grad, br.grad, 2e-4, f"db{k}")


def test_factor_attention_large_logits_stay_finite():
    """the column softmax subtracts the column maximum across chunks: k up to +-60 over 785 tokens"""
    from mmskin import ops
    qkv, ws, bs, _ = _fa_inputs(1, 28, 28, 16, 5)
    qkv[:, :, 1] *= 20.0
    y_ref = _factor_attention_fp64(qkv.double(), 28, 28, [t.double() for t in ws], [t.double() for t in bs])
    y = ops.factor_attention(qkv.to(DEV), 28, 28, [t.to(DEV) for t in ws], [t.to(DEV) for t in bs])
    assert torch.isfinite(y).all()
    _chk(y, y_ref, 1e-4, "att (large logits)")


def test_factor_attention_backward_is_bitwise_repeatable():
    from mmskin import ops
    qkv, ws, bs, dO = _fa_inputs(2, 28, 28, 16, 3)
    outs = []
    for _ in range(2):
        leaves = [t.to(DEV).requires_grad_(True) for t in [qkv] + ws + bs]
        y = ops.factor_attention(leaves[0], 28, 28, leaves[1:4], leaves[4:7])
        y.backward(dO.to(DEV))
        outs.append([y.detach().clone()] + [t.grad.clone() for t in leaves])
    for a, c in zip(*outs):
        assert torch.equal(a, c)


def test_factor_attention_rejects_other_shapes():
    from mmskin import _lib, ops
    qkv, ws, bs, _ = _fa_inputs(1, 4, 4, 8, 1)
    with pytest.raises(_lib.MMSkinError):
        ops.factor_attention(qkv.to(DEV), 4, 5, [t.to(DEV) for t in ws], [t.to(DEV) for t in bs])
    bad = torch.randn(1, 17, 3, 8, 24)
    with pytest.raises(_lib.MMSkinError):
        ops.factor_attention(bad.to(DEV), 4, 4, [t.to(DEV) for t in ws], [t.to(DEV) for t in bs])


@pytest.mark.parametrize("B,H,W,C", [(2, 14, 14, 320), (1, 56, 56, 64), (3, 7, 5, 128), (2, 2, 3, 512), (2, 1, 1, 64), (2, 9, 4, 100)])
def test_conv_pos_enc_tokens(B, H, W, C):
    """timm coat.py ConvPosEnc on [B, 1 + H * W, C]: output, dx, dw, db vs fp64 (the bounds of test_conv_pos_enc_fused); the class row
    passes through exactly, forward and backward."""
    from mmskin import ops
    g = torch.Generator().manual_seed(B + H * 3 + C)
    N = 1 + H * W
    x = torch.randn(B, N, C, generator=g); w = torch.randn(C, 1, 3, 3, generator=g) * 0.3; b = torch.randn(C, generator=g)
    dy = torch.randn(B, N, C, generator=g)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    feat = xr[:, 1:].transpose(1, 2).reshape(B, C, H, W)
    y_ref = torch.cat((xr[:, :1], (F.conv2d(feat, wr, br, padding=1, groups=C) + feat).flatten(2).transpose(1, 2)), dim=1)
    y_ref.backward(dy.double())
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    y = ops.conv_pos_enc_tokens(xd, H, W, wd, bd)
    y.backward(dy.to(DEV))
    _chk(y, y_ref, 1e-4, "y"); _chk(xd.grad, xr.grad, 1e-4, "dx"); _chk(wd.grad, wr.grad, 2e-4, "dw"); _chk(bd.grad, br.grad, 2e-4, "db")
    assert torch.equal(y[:, 0].detach().cpu(), x[:, 0])
    assert torch.equal(xd.grad[:, 0].cpu(), dy[:, 0])
    xd2, wd2, bd2 = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    ops.conv_pos_enc_tokens(xd2, H, W, wd2, bd2).backward(dy.to(DEV))
    assert torch.equal(xd2.grad, xd.grad) and torch.equal(wd2.grad, wd.grad) and torch.equal(bd2.grad, bd.grad)


def _pair(name):
    from models.hip_coat import HipCoaT
    cpu = det_init_(OracleCoaT(name))
    hip = HipCoaT(name)
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


@pytest.mark.parametrize("name,B,hw", [("coat_lite_tiny", 2, (224, 224)), ("coat_lite_small", 1, (224, 224)), ("coat_lite_tiny", 2, (96, 128))])
def test_coat_lite_matches_oracle(name, B, hw):
    cpu, hip = _pair(name)
    x, w = det_tensor(f"coat.x.{name}.{hw}", (B, 3) + hw), det_tensor(f"coat.w.{name}", (B, cpu.num_features))
    f_cpu, g_cpu = _run(cpu, x, w, "cpu")
    f_hip, g_hip = _run(hip, x, w, DEV)
    print(f"{name} {hw}: rel_err(features) = {rel_err(f_hip, f_cpu):.3e}")
    assert rel_err(f_hip, f_cpu) < 5e-4, rel_err(f_hip, f_cpu)
    assert "cpe1.proj.weight" in g_cpu and "crpe1.conv_list.2.bias" in g_cpu and not any(k.startswith("serial_blocks1.0.cpe") for k in g_cpu)
    _assert_grads_close(g_hip, g_cpu)


def test_coat_lite_tiny_bf16_operand_mode_vs_emulation():
    from bf16_emulation import assert_grads_not_worse_than_emulation, bf16_operand_emulation, grad_distance_report
    cpu, hip = _pair("coat_lite_tiny")
    x, w = det_tensor("coat.xb", (2, 3, 224, 224)), det_tensor("coat.wb", (2, 320))
    f_ref, g_ref = _run(cpu, x, w, "cpu")
    emu = det_init_(OracleCoaT("coat_lite_tiny"))
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
def test_coat_lite_small_frozen_no_grad(mode):
    from bf16_emulation import bf16_operand_emulation
    from models.loadImageModelClassifier import loadModels
    cpu = det_init_(OracleCoaT("coat_lite_small")).eval()
    hip, dim = loadModels.loadModelImageEncoder("coat_lite_small.in1k", 512, "frozen_weights")
    hip.load_state_dict(cpu.state_dict(), strict=True)
    hip = hip.to(DEV).eval()
    x = det_tensor("coat.x3", (2, 3, 224, 224))
    with torch.no_grad():
        f_ref = cpu(x)
        if mode == "bf16":
            with bf16_operand_emulation():
                f_emu = cpu(x)
        with linear_mode(mode):
            f_hip = hip(x.to(DEV)).cpu()
    assert f_hip.shape == (2, 512) and dim == 512
    if mode == "fp32":
        assert rel_err(f_hip, f_ref) < 5e-4, rel_err(f_hip, f_ref)
    else:
        assert rel_err(f_hip, f_ref) <= 1.5 * rel_err(f_emu, f_ref) + 1e-3, (rel_err(f_hip, f_ref), rel_err(f_emu, f_ref))


def test_multimodal_coat_lite_small_train_step():
    from models import multimodalIntraInterModal as M
    model = M.MultimodalModel(num_classes=6, num_heads=8, device=DEV, cnn_model_name="coat_lite_small.in1k",
                              text_model_name="one-hot-encoder", vocab_size=20, unfreeze_weights="unfrozen_weights",
                              attention_mecanism="att-intramodal+residual+cross-attention-metadados").to(DEV).train()
    disable_dropout(model)
    img, meta, lab = det_inputs(2, 224, 20, 6)
    out = model(img.to(DEV), meta.to(DEV))
    F.cross_entropy(out, lab.to(DEV)).backward()
    assert out.shape == (2, 6) and model.cnn_dim_output == 512
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.image_encoder.parameters())
