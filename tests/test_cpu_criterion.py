"""The criterion without a GPU: tests/criterion_oracle.py (the float64 restatement that tests/test_gpu_criterion.py holds the
kernels to) against tests/golden/criterion.json, recorded from torch's CrossEntropyLoss and the reference's own FocalLoss and
SoftTargetCrossEntropy in float64; the CPU path of the three modules against the same records; EpochMeter's metric formulas
against sklearn; and the argument checks of the C ABI, which fire before any launch."""
import json
import os

import numpy as np
import pytest
import torch

import criterion_oracle as co
from mmskin import _lib
from mmskin import criterion as mc
from mmskin._lib import MMSkinError

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criterion.json")) as f:
    GOLDEN = json.load(f)["shapes"]

CASES = [(B, C) + case for B, C in co.GOLDEN_SHAPES for case in co.golden_cases()]


def recorded(B, C, kind, reduction, weighted, gamma):
    shape = GOLDEN[f"{B}x{C}"]
    rec = shape["cases"][co.case_key(kind, reduction, weighted, gamma)]
    return {k: np.asarray(v) for k, v in shape["inputs"].items()}, np.asarray(rec["loss"]), np.asarray(rec["dlogits"])


def test_fixture_holds_every_case_and_the_seeded_inputs():
    assert sorted(GOLDEN) == sorted(f"{B}x{C}" for B, C in co.GOLDEN_SHAPES)
    for B, C in co.GOLDEN_SHAPES:
        assert sorted(GOLDEN[f"{B}x{C}"]["cases"]) == sorted(co.case_key(*c) for c in co.golden_cases())
        for k, v in co.golden_inputs(B, C).items():
            assert np.array_equal(np.asarray(GOLDEN[f"{B}x{C}"]["inputs"][k]), v), k


@pytest.mark.parametrize("B,C,kind,reduction,weighted,gamma", CASES)
def test_oracle_equals_the_recorded_reference(B, C, kind, reduction, weighted, gamma):
    inp, want_loss, want_grad = recorded(B, C, kind, reduction, weighted, gamma)
    loss, grad = co.run_case(inp, kind, reduction, weighted, gamma)
    np.testing.assert_allclose(loss, want_loss, rtol=1e-12, atol=0)
    np.testing.assert_allclose(grad, want_grad, rtol=1e-12, atol=1e-12 * np.abs(want_grad).max())
    if kind == "focal":                                        # the milk10K ordering of alpha: the same number to the last bits
        loss2, grad2 = co.run_case(inp, kind, reduction, weighted, gamma, alpha_last=True)
        np.testing.assert_allclose(loss2, want_loss, rtol=1e-12, atol=0)
        np.testing.assert_allclose(grad2, grad, rtol=1e-14, atol=0)


def module_for(kind, reduction, w, gamma):
    if kind == "ce":
        return mc.CrossEntropyLoss(weight=w, reduction=reduction)
    if kind == "focal":
        return mc.FocalLoss(alpha=w, gamma=gamma, reduction=reduction)
    return mc.SoftTargetCrossEntropy(weight=w)


@pytest.mark.parametrize("B,C,kind,reduction,weighted,gamma", CASES)
def test_cpu_path_of_the_modules_equals_the_records_to_fp32_rounding(B, C, kind, reduction, weighted, gamma):
    inp, want_loss, want_grad = recorded(B, C, kind, reduction, weighted, gamma)
    z = torch.from_numpy(inp["logits"]).float().requires_grad_(True)
    w = torch.from_numpy(inp["weight"]).float() if weighted else None
    target = torch.from_numpy(inp["soft"]).float() if kind == "soft" else torch.from_numpy(inp["labels"])
    loss = module_for(kind, reduction, w, gamma)(z, target)
    ((loss * torch.from_numpy(inp["upstream"]).float()).sum() if reduction == "none" else loss).backward()
    # fp32 inputs (2^-24 relative each) through a log-sum-exp of |logits| <= ~12 and a sum over B <= 7 rows: 1e-5 is ~100 ulp
    np.testing.assert_allclose(loss.detach().numpy(), want_loss, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(z.grad.numpy(), want_grad, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(want_grad).max()))


def test_oracle_ignores_labels_outside_the_classes_as_torch_ignores_minus_100():
    inp = co.golden_inputs(7, 6)
    y = inp["labels"].copy()
    y[[1, 4]] = -100
    z = torch.from_numpy(inp["logits"]).requires_grad_(True)
    want = torch.nn.functional.cross_entropy(z, torch.from_numpy(y), weight=torch.from_numpy(inp["weight"]))
    want.backward()
    loss, grad = co.hard(inp["logits"], y, inp["weight"], "ce", "mean")
    np.testing.assert_allclose(loss, want.item(), rtol=1e-13)
    np.testing.assert_allclose(grad, z.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert not grad[[1, 4]].any()
    y2 = y.copy()
    y2[[1, 4]] = 9                                             # C + 3: the same rows, the same answer
    assert np.array_equal(co.hard(inp["logits"], y2, inp["weight"], "ce", "mean")[1], grad)
    assert np.isnan(co.hard(inp["logits"], np.full(7, -100), None, "ce", "mean")[0])


# ------------------------------------------------------------------------------------------------ the meter's formulas
def expand(cm):
    t, p = np.nonzero(cm)
    n = cm[t, p]
    return np.repeat(t, n), np.repeat(p, n)


def confusion_cases():
    rng = np.random.default_rng(5)
    out = [(f"random C={C}", rng.integers(0, 9, (C, C))) for C in (2, 6, 9)]
    absent = rng.integers(1, 9, (6, 6))
    absent[3, :] = 0                                           # class 3 never present
    unpredicted = rng.integers(1, 9, (6, 6))
    unpredicted[:, 2] = 0                                      # class 2 never predicted
    both = rng.integers(1, 9, (9, 9))
    both[4, :] = 0
    both[:, 4] = 0                                             # class 4 neither present nor predicted
    binary = np.array([[5, 0], [3, 0]])                        # the positive class never predicted: precision by zero_division
    return out + [("never present", absent), ("never predicted", unpredicted), ("absent altogether", both), ("binary", binary)]


@pytest.mark.parametrize("name,cm", confusion_cases(), ids=[n for n, _ in confusion_cases()])
def test_meter_metrics_equal_sklearn(name, cm):
    import warnings
    from sklearn.metrics import accuracy_score, balanced_accuracy_score, f1_score, precision_score, recall_score
    C = cm.shape[0]
    m = mc.EpochMeter(C, "cpu")
    m.block.numpy()[m.HEADER:].view(np.int32)[:] = cm.reshape(-1)
    m.block.numpy()[:8].view(np.float64)[0] = 12.5
    m.block.numpy()[8:16].view(np.int64)[0] = cm.sum()
    got = m.compute()
    y, p = expand(cm)
    kw = dict(zero_division=0) if C == 2 else dict(average="weighted", zero_division=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                        # balanced_accuracy_score warns about the absent class it skips
        want = {"accuracy": accuracy_score(y, p), "balanced_accuracy": balanced_accuracy_score(y, p),
                "precision": precision_score(y, p, **kw), "recall": recall_score(y, p, **kw), "f1_score": f1_score(y, p, **kw)}
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=1e-12, abs=1e-15), k
    assert np.array_equal(got["confusion"], cm) and got["rows"] == cm.sum() and got["loss"] == pytest.approx(12.5 / cm.sum())


def test_meter_on_cpu_tensors_counts_as_the_device_path_is_specified():
    from sklearn.metrics import confusion_matrix
    rng = np.random.default_rng(2)
    crit = mc.CrossEntropyLoss()
    crit.meter = m = mc.EpochMeter(6, "cpu")
    probs = m.probs(64 + 17)
    zs, ys, losses = [], [], []
    for n in (64, 17):
        z = torch.from_numpy(rng.normal(0, 2, (n, 6))).float()
        z[::5, 3] = z[::5].max(dim=1).values                   # ties: the first maximum counts
        y = torch.from_numpy(rng.integers(0, 6, n))
        losses.append(float(crit(z, y)) * n)
        zs.append(z)
        ys.append(y)
    z, y = torch.cat(zs), torch.cat(ys)
    got = m.compute()
    assert np.array_equal(got["confusion"], confusion_matrix(y.numpy(), z.argmax(dim=1).numpy(), labels=np.arange(6)))
    assert got["rows"] == 81 and got["loss"] == pytest.approx(sum(losses) / 81, rel=1e-12)
    assert torch.allclose(probs, torch.softmax(z, dim=1))
    m.reset()
    assert not m.block.any() and np.isnan(m.compute()["loss"])
    with pytest.raises(ValueError, match="is full"):
        m.probs(3)
        m.update(z[:4], y[:4])


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def forward_status(dtype=_lib.F32, kind=mc.CE, reduction=2, gamma=0.0, B=4, C=6, entry="mmskin_criterion_forward"):
    tail = (None,) * 6 if entry.endswith("forward") else (None,) * 4
    _lib.call(entry, None, dtype, None, None, kind, reduction, gamma, B, C, *tail)


@pytest.mark.parametrize("entry", ["mmskin_criterion_forward", "mmskin_criterion_backward"])
@pytest.mark.parametrize("kw,word", [(dict(C=1), "1 classes"), (dict(C=1025), "1025 classes"), (dict(B=0), "batch 0"),
                                     (dict(B=(1 << 20) + 1), "batch 1048577"), (dict(kind=mc.FOCAL, gamma=0.5), "gamma 0.5"),
                                     (dict(kind=mc.FOCAL, gamma=-1.0), "gamma -1"), (dict(kind=mc.SOFT, reduction=1), "`mean` only"),
                                     (dict(dtype=7), "dtype 7"), (dict(kind=3), "unknown kind"), (dict(reduction=5), "unknown reduction"),
                                     (dict(), "null argument")])
def test_abi_rejects_bad_arguments_before_any_launch(entry, kw, word):
    with pytest.raises(MMSkinError, match=word):
        forward_status(entry=entry, **kw)


def test_scratch_size_is_monotone_in_the_batch_and_covers_the_side_buffer():
    lib = _lib.load()
    for kind in (mc.CE, mc.FOCAL, mc.SOFT):
        sizes = [lib.mmskin_criterion_scratch_floats(B, 6, kind) for B in (1, 2, 63, 64, 65, 256, 4099, 1 << 20)]
        assert sizes == sorted(sizes) and sizes[0] >= 2 + 3 + 1
        assert all(s >= 2 * B + 3 * -(-B // 64) + 1 for s, B in zip(sizes, (1, 2, 63, 64, 65, 256, 4099, 1 << 20)))
    assert lib.mmskin_criterion_scratch_floats(0, 6, 0) == -1 and lib.mmskin_criterion_scratch_floats(4, 1025, 0) == -1


def test_module_arguments_are_checked_where_they_are_given():
    with pytest.raises(ValueError, match="gamma"):
        mc.FocalLoss(gamma=0.5)
    with pytest.raises(ValueError, match="reduction"):
        mc.CrossEntropyLoss(reduction="avg")
    with pytest.raises(ValueError, match="num_classes"):
        mc.EpochMeter(1, "cpu")


def test_drop_in_module_names_import_and_construct_with_the_reference_arguments():
    import mmskin
    import models.focalLoss as focalLoss
    import models.softtargetsCrossEntropy as softtargetsCrossEntropy
    alpha = torch.tensor([0.5, 1.0, 2.0])
    f = focalLoss.FocalLoss(alpha=alpha, gamma=2, reduction='mean')
    s = softtargetsCrossEntropy.SoftTargetCrossEntropy(weight=alpha)
    assert isinstance(f, mc.FocalLoss) and isinstance(s, mc.SoftTargetCrossEntropy)
    assert f.alpha is alpha and f.gamma == 2 and f.reduction == 'mean' and s.weight is alpha
    assert mmskin.FocalLoss is mc.FocalLoss and mmskin.CrossEntropyLoss is mc.CrossEntropyLoss and mmskin.EpochMeter is mc.EpochMeter
    assert focalLoss.FocalLoss().alpha is None and softtargetsCrossEntropy.SoftTargetCrossEntropy().weight is None
    z = torch.randn(4, 3, requires_grad=True)
    f(z, torch.tensor([0, 1, 2, 1])).backward()
    assert z.grad is not None and torch.isfinite(z.grad).all()
