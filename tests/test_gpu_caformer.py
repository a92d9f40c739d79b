"""CAFormer on the HIP path: the fused StarReLU + depthwise 7x7 kernels, the StarReLU MLP, LayerNorm without bias, and the whole
encoder against the CPU restatement in tests/caformer_oracle.py (timm's NCHW formulation; timm itself is absent)."""
import pytest
import torch
import torch.nn.functional as F

from caformer_oracle import OracleCAFormer, bf16_attention
from gpu_util import DEV, linear_mode, rel_err
from helpers import disable_dropout
from oracle.detinit import det_init_, det_inputs, det_tensor

pytestmark = pytest.mark.gpu


def _max_rel(got, want):
    got, want = got.detach().double(), want.detach().double()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def _dw7_reference(z, w, s, b, dy):
    """fp64 CPU: y = conv2d(s relu(z)^2 + b, w, pad 3, groups C) on NHWC tensors, and the gradients of z, w, s, b."""
    z64 = z.double().permute(0, 3, 1, 2).requires_grad_()
    w64 = w.double().requires_grad_()
    s64, b64 = s.double().requires_grad_(), b.double().requires_grad_()
    y = F.conv2d(s64 * F.relu(z64) ** 2 + b64, w64, padding=3, groups=z.shape[-1])
    y.backward(dy.double().permute(0, 3, 1, 2))
    return y.permute(0, 2, 3, 1).detach(), z64.grad.permute(0, 2, 3, 1), w64.grad, s64.grad, b64.grad


@pytest.mark.parametrize("shape", [(2, 56, 56, 256), (2, 28, 28, 512), (1, 5, 6, 128), (3, 13, 17, 132)])
@pytest.mark.parametrize("sb", [(1.0, 0.0), (-0.15, 0.1)])
def test_dw7_star_matches_fp64(shape, sb):
    from mmskin import ops
    N, H, W, C = shape
    z = det_tensor(f"dw7.z.{shape}", shape)
    w = det_tensor(f"dw7.w.{C}", (C, 1, 7, 7), scale=1 / 7)
    dy = det_tensor(f"dw7.dy.{shape}", shape)
    s, b = torch.tensor([sb[0]]), torch.tensor([sb[1]])
    y_ref, dz_ref, dw_ref, ds_ref, db_ref = _dw7_reference(z, w, s, b, dy)
    zd, wd, sd, bd = (t.to(DEV).requires_grad_() for t in (z, w, s, b))
    y = ops.dw7_star(zd, wd, sd, bd)
    y.backward(dy.to(DEV))
    assert _max_rel(y.detach().cpu(), y_ref) < 1e-5
    assert _max_rel(zd.grad.cpu(), dz_ref) < 1e-5
    assert _max_rel(wd.grad.cpu(), dw_ref) < 1e-5
    assert abs(float(sd.grad) - float(ds_ref)) < 1e-5 * float(dy.abs().sum() * z.abs().max() ** 2)
    assert abs(float(bd.grad) - float(db_ref)) < 1e-5 * float(dy.abs().sum() * w.abs().sum(dim=(1, 2, 3)).max())


def test_dw7_star_backward_is_bitwise_repeatable():
    from mmskin import ops
    shape = (2, 28, 28, 256)
    z, dy = det_tensor("dw7r.z", shape).to(DEV), det_tensor("dw7r.dy", shape).to(DEV)
    w = det_tensor("dw7r.w", (256, 1, 7, 7), scale=1 / 7).to(DEV)
    s, b = torch.tensor([0.7], device=DEV), torch.tensor([-0.3], device=DEV)
    outs = []
    for _ in range(2):
        leaves = [t.clone().requires_grad_() for t in (z, w, s, b)]
        ops.dw7_star(*leaves).backward(dy)
        outs.append([t.grad.clone() for t in leaves])
    for a, c in zip(*outs):
        assert torch.equal(a, c)


def _star_mlp_reference(x, w1, w2, s, b, res):
    x64, w164, w264, s64, b64 = (t.double().requires_grad_() for t in (x, w1, w2, s, b))
    y = res.double() + F.linear(s64 * F.relu(F.linear(x64, w164)) ** 2 + b64, w264)
    return y, (x64, w164, w264, s64, b64)


@pytest.mark.parametrize("mode,rows,tol", [("bf16", 4096, 5e-2), ("fp32", 4096, 1e-4), ("bf16", 200, 1e-4)])
@pytest.mark.parametrize("sb", [(1.0, 0.0), (-0.15, 0.1)])
def test_star_relu_mlp(mode, rows, tol, sb):
    """bf16 mode at 4096 rows takes the kept-operand path (MlpFn with StarReLU); fp32 mode and 200 rows the elementwise StarReLU fallback."""
    from mmskin import ops
    D = 128
    x = det_tensor(f"smlp.x.{rows}", (rows, D))
    w1 = det_tensor("smlp.w1", (4 * D, D), scale=D ** -0.5)
    w2 = det_tensor("smlp.w2", (D, 4 * D), scale=(4 * D) ** -0.5)
    res = det_tensor(f"smlp.r.{rows}", (rows, D))
    dy = det_tensor(f"smlp.dy.{rows}", (rows, D))
    s, b = torch.tensor([sb[0]]), torch.tensor([sb[1]])
    y_ref, leaves_ref = _star_mlp_reference(x, w1, w2, s, b, res)
    y_ref.backward(dy.double())
    with linear_mode(mode):
        leaves = [t.to(DEV).requires_grad_() for t in (x, w1, w2, s, b)]
        y = ops.mlp(leaves[0], leaves[1], None, leaves[2], None, residual=res.to(DEV), star_relu=(leaves[3], leaves[4]))
        y.backward(dy.to(DEV))
        torch.cuda.synchronize()
    assert _max_rel(y.detach().cpu(), y_ref) < tol
    for got, want in zip(leaves, leaves_ref):
        assert rel_err(got.grad.cpu().double(), want.grad) < tol, (got.shape, rel_err(got.grad.cpu().double(), want.grad))


def test_star_relu_elementwise_and_repeatable():
    from mmskin import ops
    z, dy = det_tensor("sr.z", (3000, 37)), det_tensor("sr.dy", (3000, 37))
    s, b = torch.tensor([-0.15]), torch.tensor([0.1])
    z64, s64, b64 = (t.double().requires_grad_() for t in (z, s, b))
    y_ref = s64 * F.relu(z64) ** 2 + b64
    y_ref.backward(dy.double())
    grads = []
    for _ in range(2):
        leaves = [t.to(DEV).requires_grad_() for t in (z, s, b)]
        y = ops.star_relu(*leaves)
        y.backward(dy.to(DEV))
        grads.append([t.grad.clone() for t in leaves])
    assert _max_rel(y.detach().cpu(), y_ref) < 1e-6
    for got, want in zip(grads[0], (z64, s64, b64)):
        assert rel_err(got.cpu().double(), want.grad) < 1e-5
    for a, c in zip(*grads):
        assert torch.equal(a, c)


@pytest.mark.parametrize("M,N", [(300, 256), (4099, 320), (77, 3000)])
def test_layernorm_without_bias(M, N):
    from mmskin import ops
    from mmskin.nn import HipLayerNormNoBias
    x, dy = det_tensor(f"lnnb.x.{N}", (M, N)), det_tensor(f"lnnb.dy.{N}", (M, N))
    g = 1.0 + 0.2 * det_tensor(f"lnnb.g.{N}", (N,))
    x64, g64 = x.double().requires_grad_(), g.double().requires_grad_()
    y_ref = F.layer_norm(x64, (N,), g64, None, 1e-6)
    y_ref.backward(dy.double())
    mod = HipLayerNormNoBias(N, eps=1e-6).to(DEV)
    assert set(mod.state_dict()) == {"weight"}
    with torch.no_grad():
        mod.weight.copy_(g.to(DEV))
    xd = x.to(DEV).requires_grad_()
    y = mod(xd)
    y.backward(dy.to(DEV))
    assert _max_rel(y.detach().cpu(), y_ref) < 1e-5
    assert _max_rel(xd.grad.cpu(), x64.grad) < 1e-4
    assert _max_rel(mod.weight.grad.cpu(), g64.grad) < 1e-4
    if N % 4 == 0 and N <= 2048:      # the mixed-output inference path too
        with torch.no_grad():
            y16 = ops.layernorm(x.to(DEV), mod.weight, None, 1e-6, out_dtype=torch.bfloat16)
        assert _max_rel(y16.float().cpu(), y_ref.detach()) < 1e-2


def _pair(name):
    from models.hip_caformer import HipCAFormer
    cpu = det_init_(OracleCAFormer(name))
    hip = HipCAFormer(name)
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


def test_caformer_s18_matches_oracle():
    cpu, hip = _pair("caformer_s18")
    x, w = det_tensor("caf.x", (2, 3, 224, 224)), det_tensor("caf.w", (2, 512))
    f_cpu, g_cpu = _run(cpu, x, w, "cpu")
    f_hip, g_hip = _run(hip, x, w, DEV)
    assert rel_err(f_hip, f_cpu) < 5e-4, rel_err(f_hip, f_cpu)
    _assert_grads_close(g_hip, g_cpu)


def test_caformer_b36_forward_backward():
    cpu, hip = _pair("caformer_b36.sail_in22k_ft_in1k")
    x, w = det_tensor("cafb.x", (1, 3, 224, 224)), det_tensor("cafb.w", (1, 768))
    f_cpu, g_cpu = _run(cpu, x, w, "cpu")
    f_hip, g_hip = _run(hip, x, w, DEV)
    assert rel_err(f_hip, f_cpu) < 5e-4, rel_err(f_hip, f_cpu)
    assert set(g_hip) == set(g_cpu) and all(torch.isfinite(g).all() for g in g_hip.values())


def test_caformer_s18_bf16_operand_mode_vs_emulation():
    from bf16_emulation import assert_grads_not_worse_than_emulation, bf16_operand_emulation, grad_distance_report
    cpu, hip = _pair("caformer_s18")
    x, w = det_tensor("caf.xb", (4, 3, 224, 224)), det_tensor("caf.wb", (4, 512))
    f_ref, g_ref = _run(cpu, x, w, "cpu")
    emu = det_init_(OracleCAFormer("caformer_s18"))
    with bf16_operand_emulation(), bf16_attention():
        f_emu, g_emu = _run(emu, x, w, "cpu")
    with linear_mode("bf16"):
        f_hip, g_hip = _run(hip, x, w, DEV)
    assert rel_err(f_emu, f_ref) > 1e-4
    assert rel_err(f_hip, f_ref) <= 1.5 * rel_err(f_emu, f_ref) + 1e-3, (rel_err(f_hip, f_ref), rel_err(f_emu, f_ref))
    # The StarReLU scalars' gradients are sums over 10^5 - 10^6 terms that largely cancel: the bf16 roundings of the gradient flowing
    # in (through the fused attention backward, which the emulation models only in part) move them 2 - 20x further from the fp32
    # oracle than the emulation's.  They are held to 25 % of the oracle's value instead; every tensor parameter to 2x the emulation.
    scalars = {k for k in g_ref if k.endswith(("act.scale", "act.bias", "act1.scale", "act1.bias"))}
    for k in scalars:
        assert abs(float(g_hip[k] - g_ref[k])) <= 0.25 * abs(float(g_ref[k])) + 1e-6 * max(float(g.abs().max()) for g in g_ref.values()), k
    rows = grad_distance_report({k: v for k, v in g_ref.items() if k not in scalars}, g_hip, g_emu)
    assert_grads_not_worse_than_emulation(rows, slack=2.0)


def test_caformer_s18_input_160x192():
    cpu, hip = _pair("caformer_s18")
    x, w = det_tensor("caf.x2", (1, 3, 160, 192)), det_tensor("caf.w2", (1, 512))
    f_cpu, g_cpu = _run(cpu, x, w, "cpu")
    f_hip, g_hip = _run(hip, x, w, DEV)
    assert rel_err(f_hip, f_cpu) < 5e-4, rel_err(f_hip, f_cpu)
    _assert_grads_close(g_hip, g_cpu)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_caformer_s18_frozen_no_grad(mode):
    from bf16_emulation import bf16_operand_emulation
    from models.loadImageModelClassifier import loadModels
    cpu = det_init_(OracleCAFormer("caformer_s18")).eval()
    hip, _ = loadModels.loadModelImageEncoder("caformer_s18", 512, "frozen_weights")
    hip.load_state_dict(cpu.state_dict(), strict=True)
    hip = hip.to(DEV).eval()
    x = det_tensor("caf.x3", (2, 3, 224, 224))
    with torch.no_grad():
        f_ref = cpu(x)
        if mode == "bf16":
            with bf16_operand_emulation(), bf16_attention():
                f_emu = cpu(x)
        with linear_mode(mode):
            f_hip = hip(x.to(DEV)).cpu()
    if mode == "fp32":
        assert rel_err(f_hip, f_ref) < 5e-4, rel_err(f_hip, f_ref)
    else:   # the no-gradient fused bf16 attention rounds more than the emulation models (3.4x its distance measured): bound 4x
        assert rel_err(f_hip, f_ref) <= 4.0 * rel_err(f_emu, f_ref) + 1e-3, (rel_err(f_hip, f_ref), rel_err(f_emu, f_ref))


def test_multimodal_caformer_b36_train_step():
    """The reference's current configuration (train_pad_20.py:510-516) end to end, one step at batch 2."""
    from models import multimodalIntraInterModal as M
    model = M.MultimodalModel(num_classes=6, num_heads=8, device=DEV, cnn_model_name="caformer_b36.sail_in22k_ft_in1k",
                              text_model_name="one-hot-encoder", vocab_size=20, unfreeze_weights="unfrozen_weights",
                              attention_mecanism="att-intramodal+residual+cross-attention-metadados").to(DEV).train()
    disable_dropout(model)
    img, meta, lab = det_inputs(2, 224, 20, 6)
    out = model(img.to(DEV), meta.to(DEV))
    F.cross_entropy(out, lab.to(DEV)).backward()
    assert out.shape == (2, 6) and model.cnn_dim_output == 768
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.image_encoder.parameters())
