"""-m gpu: the criterion kernels (csrc/criterion.hip) through mmskin.criterion against the float64 restatement
tests/criterion_oracle.py, which tests/test_cpu_criterion.py pins to values recorded from torch and from the reference's classes.

The bound, the same for every comparison here: the kernel's largest error against float64 may be at most twice the error that
the SAME formula has when torch evaluates it in fp32 on the CPU (the factor 2: another summation order over B and C), with a
floor of 1e-6 max(1, max |want|) for the cases where the fp32 evaluation happens to be exact.  dlogits in bf16 is the fp32
result rounded once to 8 significant bits, so there half a bf16 ulp of the element, 2^(floor(log2 |want|) - 8) -- the precision
of the output format -- is added; the loss is fp32 for either dtype.  Every case prints both errors."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import criterion_oracle as co
from gpu_util import DEV
from helpers import CLASS_WEIGHTS, SMALL, disable_dropout
from mmskin import criterion as mc
from models import multimodalIntraInterModal as M
from oracle.detinit import det_init_, det_inputs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (3, 2), (7, 6), (64, 6), (65, 9), (257, 8),      # the 64-row workgroup edge and one past it
          (5, 64), (5, 65),                                         # the last one-class-per-lane width and the first 16-per-lane one
          (5, 1000), (3, 1024),                                     # the 16-per-lane register limit and its boundary
          (4099, 7)]                                                # more than one partial block; prime
CONFIGS = co.golden_cases()                                         # kind x reduction x {weights, none}; focal gamma 0, 1.5, 2


def inputs(B, C, seed=0, scale=3.0):
    rng = np.random.default_rng(seed + 1000 * B + C)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)          # fp32-representable: every party reads the same numbers
    return {"logits": f32(rng.normal(0.0, scale, (B, C))), "labels": rng.integers(0, C, B), "weight": f32(rng.uniform(0.3, 3.0, C)),
            "soft": f32(rng.dirichlet(np.ones(C), B)), "upstream": f32(rng.normal(0.0, 1.0, B))}


def rounded(inp, dtype):
    """the logits as the dtype holds them (float64 values), so that the oracle, the fp32 formula and the kernel read the same numbers"""
    out = dict(inp)
    out["logits"] = torch.from_numpy(inp["logits"]).to(dtype).double().numpy()
    return out


def module_for(kind, reduction, w, gamma):
    if kind == "ce":
        return mc.CrossEntropyLoss(weight=w, reduction=reduction)
    if kind == "focal":
        return mc.FocalLoss(alpha=w, gamma=gamma, reduction=reduction)
    return mc.SoftTargetCrossEntropy(weight=w)


def formula_fp32(kind, reduction, z, target, w, gamma):
    """the criterion as torch evaluates the reference's formula in fp32 (1 - exp(-ce), not expm1): the yardstick of the bound"""
    if kind == "ce":
        return F.cross_entropy(z, target, weight=w, reduction=reduction)
    if kind == "soft":
        lsm = F.log_softmax(z, dim=-1)
        return -((target * lsm * w.unsqueeze(0)) if w is not None else target * lsm).sum(dim=-1).mean()
    ce = F.cross_entropy(z, target, reduction="none")
    rows = (1 - torch.exp(-ce)) ** gamma * (ce if w is None else w.gather(0, target) * ce)
    return rows.mean() if reduction == "mean" else rows.sum() if reduction == "sum" else rows


def run(fn, z, target, upstream, reduction):
    """(loss, dlogits) of fn on leaf logits z; `none` is contracted with the upstream vector"""
    z = z.detach().clone().requires_grad_(True)
    loss = fn(z, target)
    ((loss * upstream).sum() if reduction == "none" else loss).backward()
    return loss.detach(), z.grad.detach()


def evaluate(inp, kind, reduction, weighted, gamma, dtype):
    """-> dict of (got, want float64, fp32-formula) for loss and dlogits, all numpy float64"""
    inp = rounded(inp, dtype)
    w64 = inp["weight"] if weighted else None
    if kind == "soft":
        want = co.soft(inp["logits"], inp["soft"], w64)
    else:
        want = co.hard(inp["logits"], inp["labels"], w64, kind, reduction, gamma, upstream=inp["upstream"] if reduction == "none" else None)
    t = lambda a, d=torch.float32: None if a is None else torch.from_numpy(np.asarray(a)).to(d)
    target = t(inp["soft"]) if kind == "soft" else t(inp["labels"], torch.int64)
    ref = run(lambda z, y: formula_fp32(kind, reduction, z, y, t(w64), gamma), t(inp["logits"]), target, t(inp["upstream"]), reduction)
    crit = module_for(kind, reduction, None if w64 is None else t(w64).to(DEV), gamma)
    got = run(crit, t(inp["logits"]).to(DEV, dtype), target.to(DEV), t(inp["upstream"]).to(DEV), reduction)
    assert got[0].dtype == torch.float32 and got[1].dtype == dtype
    f64 = lambda x: x.double().cpu().numpy()
    return {"loss": (f64(got[0]), np.asarray(want[0]), f64(ref[0])), "dlogits": (f64(got[1]), np.asarray(want[1]), f64(ref[1]))}


def half_bf16_ulp(x):
    """bf16 keeps 8 significant bits: values in [2^e, 2^(e+1)) are 2^(e-7) apart"""
    a = np.abs(x)
    return np.where(a > 0, np.exp2(np.floor(np.log2(np.where(a > 0, a, 1.0))) - 8), 0.0)


def check(res, dtype, what, ratios=None):
    for name, (got, want, ref) in res.items():
        assert np.isfinite(got).all(), (what, name)
        floor = 1e-6 * max(1.0, float(np.abs(want).max()))
        ref_err = float(np.abs(ref - want).max())
        allowed = max(2.0 * ref_err, floor) + (half_bf16_ulp(want) if name == "dlogits" and dtype == torch.bfloat16 else 0.0)
        err = np.abs(got - want)
        worst = float((err / allowed).max())
        print(f"{what} {name}: kernel err {float(err.max()):.3e}  fp32 formula err {ref_err:.3e}  floor {floor:.1e}  err/allowed {worst:.3f}")
        if ratios is not None:
            ratios.append(worst)
        assert worst <= 1.0, (what, name, float(err.max()), ref_err, floor)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,C", SHAPES)
def test_forward_and_dlogits_match_float64_within_twice_the_fp32_formula(B, C, dtype):
    inp = inputs(B, C)
    ratios = []
    for kind, reduction, weighted, gamma in CONFIGS:
        check(evaluate(inp, kind, reduction, weighted, gamma, dtype), dtype, f"({B},{C}) {co.case_key(kind, reduction, weighted, gamma)}", ratios)
    print(f"({B},{C}) {dtype}: worst err/allowed over {len(CONFIGS)} configurations = {max(ratios):.3f}")


@pytest.mark.parametrize("gamma", [1.0, 1.5, 2.0, 5.0])
def test_focal_on_confident_rows(gamma):
    """rows whose true class leads by 6 .. 18: 1 - pt is 2e-3 .. 1e-8, where 1 - exp(-ce) cancels in fp32 and -expm1(-ce) does not"""
    B, C = 65, 6
    inp = inputs(B, C, seed=7, scale=1.0)
    inp["logits"][np.arange(B), inp["labels"]] += np.linspace(6.0, 18.0, B)
    for reduction in ("none", "sum", "mean"):
        res = evaluate(inp, "focal", reduction, True, gamma, torch.float32)
        check(res, torch.float32, f"confident gamma={gamma:g} {reduction}")
        if reduction == "none":
            got, want, ref = res["loss"]
            rel = lambda x: float((np.abs(x - want) / np.abs(want)).max())
            print(f"confident gamma={gamma:g}: worst RELATIVE row error  kernel {rel(got):.3e}  fp32 formula {rel(ref):.3e}")


def test_large_logits_and_constant_rows_stay_finite():
    B, C = 9, 6
    inp = inputs(B, C, seed=3)
    inp["logits"] = np.where(np.random.default_rng(4).random((B, C)) < 0.5, 80.0, -80.0)
    inp["logits"][2] = 80.0                                         # identical logits: p = 1 / C
    inp["logits"][3] = -80.0
    inp["logits"][4] = 0.0
    inp["logits"][5] = [80.0, 78.0, -80.0, 79.5, 0.0, 80.0]
    for dtype in (torch.float32, torch.bfloat16):
        for kind, reduction, weighted, gamma in CONFIGS:
            check(evaluate(inp, kind, reduction, weighted, gamma, dtype), dtype, f"large {dtype} {co.case_key(kind, reduction, weighted, gamma)}")


IGNORED = ([1, 5, 30, 64, 66], [0, 7, 65])                            # rows labelled -100, rows labelled C + 3


def with_ignored(inp, C):
    y = inp["labels"].copy()
    y[IGNORED[0]] = -100
    y[IGNORED[1]] = C + 3
    return dict(inp, labels=y)


@pytest.mark.parametrize("kind,reduction,gamma", [("ce", "mean", 0.0), ("ce", "sum", 0.0), ("ce", "none", 0.0), ("focal", "mean", 2.0),
                                                  ("focal", "none", 1.5)])
def test_ignored_labels_give_no_loss_and_no_gradient(kind, reduction, gamma):
    B, C = 67, 6
    inp = with_ignored(inputs(B, C, seed=11), C)
    res = evaluate_ignored(inp, kind, reduction, gamma)
    got_loss, got_grad = res
    rows = sorted(IGNORED[0] + IGNORED[1])
    assert not got_grad[rows].any(), "an ignored row received a gradient"
    others = np.setdiff1d(np.arange(B), rows)
    assert (np.abs(got_grad[others]).sum(axis=1) > 0).all(), "a valid row received none"
    if reduction == "none":
        assert not got_loss[rows].any()


def evaluate_ignored(inp, kind, reduction, gamma):
    """kernel against the oracle (which test_cpu_criterion holds to torch's ignore_index) under the bound of this file; the fp32
    yardstick is the oracle's own formula evaluated in fp32 by torch on the valid rows, which for CE is torch's ignore_index"""
    C = inp["logits"].shape[1]
    w = torch.tensor(inp["weight"], dtype=torch.float32)
    z = torch.from_numpy(inp["logits"]).float()
    y = torch.from_numpy(inp["labels"])
    up = torch.from_numpy(inp["upstream"]).float()
    want = co.hard(z.double().numpy(), inp["labels"], w.double().numpy(), kind, reduction, gamma, upstream=up.double().numpy() if reduction == "none" else None)
    crit = module_for(kind, reduction, w.to(DEV), gamma)
    got = run(crit, z.to(DEV), y.to(DEV), up.to(DEV), reduction)
    got = (got[0].double().cpu().numpy(), got[1].double().cpu().numpy())
    if kind == "ce":
        y_torch = torch.where((y < 0) | (y >= C), torch.full_like(y, -100), y)      # torch knows one ignore_index: map C + 3 onto it
        ref = run(lambda a, b: F.cross_entropy(a, b, weight=w, reduction=reduction), z, y_torch, up, reduction)
        res = {"loss": (got[0], np.asarray(want[0]), ref[0].double().numpy()), "dlogits": (got[1], want[1], ref[1].double().numpy())}
    else:                                                             # the reference's focal loss cannot gather alpha at -100: floor only
        res = {"loss": (got[0], np.asarray(want[0]), np.asarray(want[0])), "dlogits": (got[1], want[1], want[1])}
    check(res, torch.float32, f"ignored {kind} {reduction}")
    return got


def test_ce_mean_divides_by_the_valid_weights_as_torch_ignore_index():
    B, C = 67, 6
    inp = inputs(B, C, seed=12)
    y = torch.from_numpy(inp["labels"])
    y[IGNORED[0]] = -100
    w = torch.tensor(inp["weight"], dtype=torch.float32)
    z = torch.from_numpy(inp["logits"]).float()
    want, want_grad = run(lambda a, b: F.cross_entropy(a.double(), b, weight=w.double()), z, y, None, "mean")
    ref, ref_grad = run(lambda a, b: F.cross_entropy(a, b, weight=w), z, y, None, "mean")
    got, got_grad = run(mc.CrossEntropyLoss(weight=w.to(DEV)), z.to(DEV), y.to(DEV), None, "mean")
    f64 = lambda x: x.double().cpu().numpy()
    check({"loss": (f64(got), f64(want), f64(ref)), "dlogits": (f64(got_grad), f64(want_grad), f64(ref_grad))}, torch.float32, "ignore_index")


def test_all_rows_ignored_mean_is_nan_as_torch_and_the_gradient_is_zero():
    z = torch.randn(5, 6)
    y = torch.full((5,), -100)
    assert torch.isnan(F.cross_entropy(z, y))
    got, grad = run(mc.CrossEntropyLoss(), z.to(DEV), y.to(DEV), None, "mean")
    assert torch.isnan(got) and not grad.any()
    got, grad = run(mc.CrossEntropyLoss(reduction="sum"), z.to(DEV), y.to(DEV), None, "sum")
    assert float(got) == 0.0 and not grad.any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,C", [(7, 6), (257, 8), (5, 1000)])
def test_focal_with_gamma_zero_is_cross_entropy_bit_for_bit(B, C, dtype):
    inp = inputs(B, C, seed=5)
    z = torch.from_numpy(inp["logits"]).to(DEV, dtype)
    y = torch.from_numpy(inp["labels"]).to(DEV)
    up = torch.from_numpy(inp["upstream"]).float().to(DEV)
    for w in (None, torch.from_numpy(inp["weight"]).float().to(DEV)):
        for reduction in ("sum", "none"):
            ce = run(mc.CrossEntropyLoss(weight=w, reduction=reduction), z, y, up, reduction)
            focal = run(mc.FocalLoss(alpha=w, gamma=0, reduction=reduction), z, y, up, reduction)
            assert torch.equal(ce[0], focal[0]) and torch.equal(ce[1], focal[1]), (reduction, w is not None)


def test_upstream_gradient_scales_dlogits():
    inp = inputs(65, 9, seed=6)
    z = torch.from_numpy(inp["logits"]).float().to(DEV)
    y = torch.from_numpy(inp["labels"]).to(DEV)
    w = torch.from_numpy(inp["weight"]).float().to(DEV)
    for crit in (mc.CrossEntropyLoss(weight=w), mc.FocalLoss(alpha=w, gamma=2), mc.FocalLoss(alpha=w, gamma=1.5, reduction="sum")):
        _, once = run(crit, z, y, None, "mean")
        _, thrice = run(lambda a, b: 3.0 * crit(a, b), z, y, None, "mean")
        # g / denominator, times w[y], times the focal slope, times (p - 1[j = y]): four roundings in either run, 8 x 2^-24
        assert torch.allclose(thrice, 3.0 * once, rtol=5e-7, atol=0)
    soft_t = torch.from_numpy(inp["soft"]).float().to(DEV)
    _, once = run(mc.SoftTargetCrossEntropy(weight=w), z, soft_t, None, "mean")
    _, thrice = run(lambda a, b: 3.0 * mc.SoftTargetCrossEntropy(weight=w)(a, b), z, soft_t, None, "mean")
    assert torch.allclose(thrice, 3.0 * once, rtol=5e-7, atol=1e-9)
    # `none` under a random upstream vector against the oracle: part of CONFIGS in the parity test above, at every shape


def test_forward_backward_and_meter_are_bitwise_repeatable():
    B, C = 4099, 7
    inp = inputs(B, C, seed=8)
    z = torch.from_numpy(inp["logits"]).float().to(DEV)
    y = torch.from_numpy(inp["labels"]).to(DEV)
    w = torch.from_numpy(inp["weight"]).float().to(DEV)
    for make in (lambda: mc.CrossEntropyLoss(weight=w), lambda: mc.FocalLoss(alpha=w, gamma=2), lambda: mc.FocalLoss(alpha=w, gamma=1.5, reduction="sum")):
        outs = []
        for _ in range(2):
            crit = make()
            crit.meter = mc.EpochMeter(C, DEV)
            loss, grad = run(crit, z, y, None, "mean")
            crit(z, y)                                                # a second batch into the same accumulators
            outs.append((loss.cpu(), grad.cpu(), crit.meter.block.cpu()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert torch.equal(outs[0][2], outs[1][2]), "the meter's double / counters differ between two runs"
    t = torch.from_numpy(inp["soft"]).float().to(DEV)
    a, b = run(mc.SoftTargetCrossEntropy(weight=w), z, t, None, "mean"), run(mc.SoftTargetCrossEntropy(weight=w), z, t, None, "mean")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_meter_confusion_probs_loss_and_reset():
    from sklearn.metrics import confusion_matrix
    C = 6
    rng = np.random.default_rng(9)
    m = mc.EpochMeter(C, DEV)
    probs = m.probs(64 + 64 + 17)
    zs, ys, losses = [], [], []
    for n in (64, 64, 17):
        z = torch.from_numpy(rng.normal(0, 2, (n, C))).float()
        z[::5, 4] = z[::5].max(dim=1).values                          # known ties: class 4 equals the row maximum
        z[3] = 1.25                                                   # a constant row: class 0
        y = torch.from_numpy(rng.integers(0, C, n))
        losses.append(m.update(z.to(DEV), y.to(DEV)))
        zs.append(z)
        ys.append(y)
    z, y = torch.cat(zs), torch.cat(ys)
    got = m.compute()
    assert np.array_equal(got["confusion"], confusion_matrix(y.numpy(), z.argmax(dim=1).numpy(), labels=np.arange(C)))
    assert got["rows"] == 145
    per_batch = [float(v) for v in losses]
    want_loss = (per_batch[0] * 64 + per_batch[1] * 64 + per_batch[2] * 17) / 145
    assert got["loss"] == pytest.approx(want_loss, rel=1e-6)          # fp32 batch means times n against the double of the sums
    want_p = co.softmax(z.double().numpy())
    ref_p = torch.softmax(z, dim=1).double().numpy()
    check({"probs": (probs.double().cpu().numpy(), want_p, ref_p)}, torch.float32, "meter probs")
    from sklearn.metrics import accuracy_score
    assert got["accuracy"] == pytest.approx(accuracy_score(y.numpy(), z.argmax(dim=1).numpy()))
    m.reset()
    assert not m.block.any() and m.compute()["rows"] == 0


def test_meter_attached_to_a_weighted_criterion_keeps_the_batch_means():
    C = 9
    inp = inputs(65, C, seed=10)
    z = torch.from_numpy(inp["logits"]).float().to(DEV)
    y = torch.from_numpy(inp["labels"]).to(DEV)
    w = torch.from_numpy(inp["weight"]).float().to(DEV)
    for crit in (mc.CrossEntropyLoss(weight=w), mc.CrossEntropyLoss(weight=w, reduction="sum"), mc.FocalLoss(alpha=w, gamma=2)):
        crit.meter = m = mc.EpochMeter(C, DEV)
        crit(z, y)
        crit(z[:17], y[:17])
        kind = type(crit)(w) if isinstance(crit, mc.CrossEntropyLoss) else mc.FocalLoss(alpha=w, gamma=2)
        want = (float(kind(z, y)) * 65 + float(kind(z[:17], y[:17])) * 17) / 82
        assert m.compute()["loss"] == pytest.approx(want, rel=1e-6)


def test_one_training_step_with_the_fused_criterion():
    kw = dict(SMALL, attention_mecanism="crossattention", device=DEV)
    model = det_init_(M.MultimodalModel(**kw)).to(DEV)
    model.train()
    disable_dropout(model)
    img, meta, lab = det_inputs(4, 32, 20, 6)
    w = torch.tensor(CLASS_WEIGHTS, device=DEV)
    steps = {}
    for name, crit in (("torch", nn.CrossEntropyLoss(weight=w)), ("fused", mc.CrossEntropyLoss(weight=w))):
        model.zero_grad(set_to_none=True)
        out = model(img.to(DEV), meta.to(DEV))
        loss = crit(out, lab.to(DEV))
        loss.backward()
        steps[name] = (out.detach().double().cpu(), float(loss.detach()), {k: p.grad.double().cpu() for k, p in model.named_parameters() if p.grad is not None})
    w64 = np.asarray(CLASS_WEIGHTS, dtype=np.float32).astype(np.float64)
    want = {k: co.hard(v[0].numpy(), lab.numpy(), w64, "ce", "mean")[0] for k, v in steps.items()}     # each on its own run's logits
    err, ref_err = abs(steps["fused"][1] - want["fused"]), abs(steps["torch"][1] - want["torch"])
    print(f"one step: loss fused {steps['fused'][1]:.8f} (err {err:.3e})  torch {steps['torch'][1]:.8f} (err {ref_err:.3e})")
    assert err <= max(2 * ref_err, 1e-6 * max(1.0, abs(want["fused"])))
    assert sorted(steps["torch"][2]) == sorted(steps["fused"][2]) and len(steps["fused"][2]) > 0
    worst = 0.0
    for k, g in steps["fused"][2].items():
        assert torch.isfinite(g).all(), k
        ref = steps["torch"][2][k]
        worst = max(worst, float((g - ref).abs().max() / (ref.abs().max() + 1e-30)))
    print(f"one step: worst relative parameter-gradient difference fused vs torch criterion = {worst:.3e}")


def test_second_order_raises_and_shapes_are_checked():
    from mmskin._lib import MMSkinError
    z = torch.randn(4, 6, device=DEV, requires_grad=True)
    y = torch.tensor([0, 1, 2, 3], device=DEV)
    loss = mc.CrossEntropyLoss()(z, y)
    (g,) = torch.autograd.grad(loss, z, create_graph=True)
    with pytest.raises(MMSkinError, match="second-order"):
        g.sum().backward()
    with pytest.raises(ValueError, match=r"\[B, C\]"):
        mc.CrossEntropyLoss()(torch.randn(4, 6, 2, device=DEV), y)
    with pytest.raises(MMSkinError, match="1 classes"):
        mc.CrossEntropyLoss()(torch.randn(4, 1, device=DEV), y)
