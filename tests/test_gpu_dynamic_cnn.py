"""-m gpu: the DynamicCNN trunk plan (csrc/dynamic_cnn.hip through mmskin.backbone.HipDynamicCNNFeatures) and the drop-in model
(models/dynamicMultimodalmodel.py) against the plain-torch restatement of tests/dynamic_cnn_oracle.py.

Trunk: one train step (forward, backward of (f * w).sum()) in fp32 and bf16 against the restatement in fp64, at the cases of
dynamic_cnn_oracle.TRUNK_CASES.  Acceptance as tests/test_gpu_vgg.py::test_vgg_train_step_vs_oracle, with its constants: fp32 features
within 1e-4 and every gradient at most 3x torch CPU fp32's own distance from fp64 plus 2e-4; bf16 features within 3e-2 and every gradient,
layer by layer, at most 1.5x the distance of a CPU emulation plus 0.02.  The emulation keeps fp32 arithmetic and rounds to bf16 what the
plan stores in bf16: the image, the conv weights, every conv output y, and each stored activation (z, or the pooled tensor where a pool
follows; the last layer stores neither).  Measured on the CPU for these cases (relative L2 against fp64): CPU fp32 features 1.3e-7 and
gradients at most 7.6e-7; the emulation's features 9e-4 to 2.3e-3, its best gradient 1.3e-3 to 2.9e-3 and its worst (always the first
conv's weight, a sum with heavy cancellation as in VGG) 1.7e-2, 1.1e-1 and 2.1e-1 -- GroupNorm's conditioning leaves VGG's constants
neither vacuous nor too tight, so they stay.

Model: forward + backward of every branch in fp32 mode against the restatement loaded with the same state_dict, with the bounds of
test_gpu_vgg.py's model test (logits 1e-3 absolute, gradients 5e-3 relative L2): fp32 arithmetic on both sides, different summation order.
"""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dynamic_cnn_oracle as do
from gpu_util import DEV
from helpers import disable_dropout
from mmskin import _lib
from mmskin._lib import call, ptr, stream

pytestmark = pytest.mark.gpu


def _l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _rb(t):
    return t.bfloat16().float()


def trunk_pair(case):
    """the restatement with seeded default weights and non-trivial GroupNorm affine parameters, and the inputs of one step"""
    filters, layers, pool, (n, h, w) = case
    torch.manual_seed(4321)
    cpu = do.OracleTrunk(filters, layers, pool)
    g = torch.Generator().manual_seed(99)
    with torch.no_grad():
        for m in cpu.modules():
            if isinstance(m, nn.GroupNorm):
                m.weight.copy_(1 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
    x = torch.randn(n, 3, h, w, generator=g)
    wgt = torch.randn(n, filters[-1], generator=g)
    return cpu, x, wgt


def clone_trunk(cpu, case):
    filters, layers, pool, _ = case
    m = do.OracleTrunk(filters, layers, pool)
    m.load_state_dict(cpu.state_dict())
    return m


def bf16_storage_emulation(model):
    """fp32 arithmetic with bf16 STORAGE of what the plan stores in bf16: conv weights, every conv output, the stored activations"""
    seq = list(model.conv_block)
    for i, m in enumerate(seq):
        last = not any(isinstance(t, nn.Conv2d) for t in seq[i + 1:])     # behind the last conv nothing is stored: the fused tail
        if isinstance(m, nn.Conv2d):
            m.weight.data = _rb(m.weight.data)
            m.register_forward_hook(lambda mod, i, o: _rb(o))
        elif isinstance(m, nn.ReLU) and not last and not (i + 1 < len(seq) and isinstance(seq[i + 1], nn.MaxPool2d)):
            m.register_forward_hook(lambda mod, i, o: _rb(o))
        elif isinstance(m, nn.MaxPool2d) and not last:
            m.register_forward_hook(lambda mod, i, o: _rb(o))
    return model


def cpu_step(model, x, w):
    model.train()
    f = model(x)
    (f * w).sum().backward()
    return f.detach().double(), {k[len("conv_block."):]: p.grad.detach().double() for k, p in model.named_parameters()}


def cpu_runs(case, with_emulation):
    cpu, x, w = trunk_pair(case)
    runs = {"cpu": cpu_step(clone_trunk(cpu, case), x, w), "truth": cpu_step(clone_trunk(cpu, case).double(), x.double(), w.double())}
    if with_emulation:
        runs["emu"] = cpu_step(bf16_storage_emulation(clone_trunk(cpu, case)), _rb(x), w)
    return cpu, x, w, runs


# The first conv alone (one layer, no pool: dynamic-cnn/64/l1/p0/k3) on an image of odd height and width, so the rounding of the packed
# image's width to an even number (FirstGeom) shows in every row the conv reads.  33 x 35: mmskin_backbone_create takes no side under 32.
FIRST_CONV_ODD = ((64,), 1, False, (2, 33, 35))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", do.TRUNK_CASES + (FIRST_CONV_ODD,), ids=do.trunk_id)
def test_trunk_train_step_vs_oracle(case, dtype):
    from mmskin.backbone import HipDynamicCNNFeatures
    filters, layers, pool, _ = case
    cpu, x, w, runs = cpu_runs(case, dtype == "bf16")
    hip = HipDynamicCNNFeatures(filters, layers, pool, compute_dtype=dtype)
    hip.load_state_dict(cpu.conv_block.state_dict(), strict=True)
    hip = hip.to(DEV).train()
    f = hip(x.to(DEV))
    (f * w.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    f_h, g_h = f.detach().cpu().double(), {k: p.grad.detach().cpu().double() for k, p in hip.named_parameters()}
    (f_t, g_t), (f_c, g_c) = runs["truth"], runs["cpu"]
    assert f_h.shape == f_t.shape and set(g_h) == set(g_t)
    keys = list(g_t)
    f_hip, f_cpu = _l2(f_h, f_t), _l2(f_c, f_t)
    hip_l2 = {k: _l2(g_h[k], g_t[k]) for k in keys}
    cpu_l2 = {k: _l2(g_c[k], g_t[k]) for k in keys}
    worst = max(keys, key=lambda k: hip_l2[k])
    print(do.trunk_id(case), dtype, "feat", f_hip, f_cpu, "grad worst", worst, hip_l2[worst], cpu_l2[worst])
    assert all(torch.isfinite(g).all() for g in g_h.values())
    if dtype == "fp32":
        assert f_hip < 1e-4
        assert all(hip_l2[k] <= 3 * cpu_l2[k] + 2e-4 for k in keys), [(k, hip_l2[k], cpu_l2[k]) for k in keys if hip_l2[k] > 3 * cpu_l2[k] + 2e-4]
    else:
        emu_l2 = {k: _l2(runs["emu"][1][k], g_t[k]) for k in keys}
        print("emulation worst", max(emu_l2.values()), "feat", _l2(runs["emu"][0], f_t))
        assert f_hip < 3e-2
        assert all(hip_l2[k] <= 1.5 * emu_l2[k] + 0.02 for k in keys), [(k, hip_l2[k], emu_l2[k]) for k in keys if hip_l2[k] > 1.5 * emu_l2[k] + 0.02]


def test_trunk_eval_forward_and_second_step_reuse_the_plan():
    """train and eval run the same kernels (GroupNorm keeps no running statistics); a second step on the cached plan gives the same bits"""
    from mmskin.backbone import HipDynamicCNNFeatures
    case = do.TRUNK_CASES[0]
    cpu, x, w = trunk_pair(case)
    hip = HipDynamicCNNFeatures(*case[:3], compute_dtype="fp32")
    hip.load_state_dict(cpu.conv_block.state_dict(), strict=True)
    hip = hip.to(DEV).train()
    outs, grads = [], []
    for _ in range(2):
        hip.zero_grad(set_to_none=True)
        f = hip(x.to(DEV))
        (f * w.to(DEV)).sum().backward()
        outs.append(f.detach().clone())
        grads.append(hip.last_flat_grad.clone())
    with torch.no_grad():
        e = hip.eval()(x.to(DEV))
    assert len(hip._plans) == 1
    assert torch.equal(outs[0], outs[1]) and torch.equal(grads[0], grads[1]) and torch.equal(outs[0], e)


@pytest.mark.parametrize("branch", do.BRANCHES)
def test_dynamic_cnn_model_vs_oracle(branch, monkeypatch):
    from models.dynamicMultimodalmodel import DynamicCNN
    monkeypatch.setenv("MMSKIN_BACKBONE_DTYPE", "fp32")
    kw = dict(do.MODEL_KW, attention_mecanism=branch)
    torch.manual_seed(7)
    cpu = do.OracleDynamicCNN(**kw)
    hip = DynamicCNN(**dict(kw, device=DEV))
    hip.load_state_dict(cpu.state_dict(), strict=True)
    hip = hip.to(DEV)
    g = torch.Generator().manual_seed(8)
    img, meta = torch.randn(4, 3, 32, 32, generator=g), torch.randn(4, 20, generator=g)
    lab = torch.tensor([0, 3, 5, 1])
    res = {}
    for name, m, dev in (("cpu", cpu, "cpu"), ("hip", hip, DEV)):
        m.train(); disable_dropout(m)
        out = m(img.to(dev), meta.to(dev))
        F.cross_entropy(out, lab.to(dev)).backward()
        res[name] = (out.detach().cpu(), {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in m.named_parameters()})
    assert (res["cpu"][0] - res["hip"][0]).abs().max() < 1e-3
    assert list(res["cpu"][1]) == list(res["hip"][1])
    none_cpu, none_hip = ({k for k, v in res[n][1].items() if v is None} for n in ("cpu", "hip"))
    assert none_cpu == none_hip, none_cpu ^ none_hip
    with_grad = [k for k, v in res["cpu"][1].items() if v is not None]
    assert with_grad and all(torch.isfinite(res["hip"][1][k]).all() for k in with_grad)
    # a gradient that is exactly zero on the CPU (the q / k rows of a length-1 attention) must be exactly zero here too
    worst = max(with_grad, key=lambda k: _l2(res["hip"][1][k], res["cpu"][1][k]))
    assert _l2(res["hip"][1][worst], res["cpu"][1][worst]) < 5e-3, (worst, _l2(res["hip"][1][worst], res["cpu"][1][worst]))


def test_default_config_trains_a_step():
    """`DynamicCNN(config={})`, the reference's calling code with only the import path changed: bf16 trunk, one optimizer step"""
    from models.dynamicMultimodalmodel import DynamicCNN
    torch.manual_seed(11)
    model = DynamicCNN(config={}, device=DEV).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(12)
    img, meta, lab = torch.randn(2, 3, 64, 64, generator=g).to(DEV), torch.randn(2, 85, generator=g).to(DEV), torch.tensor([1, 7], device=DEV)
    before = model.conv_block.state_dict()["0.weight"].clone()
    model.train()
    out = model(img, meta)
    assert out.shape == (2, 10)
    loss = F.cross_entropy(out, lab)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and not torch.equal(before, model.conv_block.state_dict()["0.weight"])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.conv_block.parameters())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("arch", ["dynamic-cnn/64-128/l2/p1/k3", "dynamic-cnn/64-128/l1/p0/k3", "dynamic-cnn/64-128/l2/p1/k3/t0"])
def test_plan_stays_inside_its_workspace(arch, dtype):
    """forward + backward on a buffer of ws_bytes + 64 KiB whose tail holds a canary; every gradient element is written"""
    GUARD = 65536
    lib = _lib.load()
    N, H, W = 2, 36, 44
    h = ctypes.c_void_p()
    call("mmskin_backbone_create", arch.encode(), N, H, W, {"fp32": _lib.F32, "bf16": _lib.BF16}[dtype], ctypes.byref(h))
    try:
        size, numel, C = lib.mmskin_backbone_workspace_bytes(h), lib.mmskin_backbone_param_numel(h), lib.mmskin_backbone_feature_dim(h)
        g = torch.Generator().manual_seed(3)
        params = (0.05 * torch.randn(numel, generator=g)).to(DEV)
        x, dfeat = torch.randn(N, 3, H, W, generator=g).to(DEV), torch.randn(N, C, generator=g).to(DEV)
        wsp = torch.zeros(size + GUARD, dtype=torch.uint8, device=DEV)
        wsp[size:] = 0xA5
        feat, grads = torch.full((N, C), float("nan"), device=DEV), torch.full((numel,), float("nan"), device=DEV)
        call("mmskin_backbone_forward", h, ptr(x), ptr(params), None, ptr(wsp), ptr(feat), 1, stream())
        call("mmskin_backbone_backward", h, ptr(dfeat), ptr(params), ptr(wsp), ptr(grads), stream())
        torch.cuda.synchronize()
        assert bool((wsp[size:] == 0xA5).all()), "the plan wrote behind the workspace it reports"
        assert bool(torch.isfinite(feat).all()) and bool(torch.isfinite(grads).all()), "an output element was not written"
    finally:
        lib.mmskin_backbone_destroy(h)
