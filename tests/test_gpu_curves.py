"""mmskin.curves.FoldCurves on device tensors against its own host path and against scikit-learn, from a fold directory, and
through evaluate_model(..., curves=True) on the device.  The integers, thresholds, indices and the AUC are compared exactly; the
remaining fp64 summaries within 1e-12 (another order of a sum of at most N non-negative terms in [0, 1])."""
import os

import numpy as np
import pytest
import torch

import curves_oracle as co
from gpu_util import DEV
from helpers import SMALL
from mmskin import FoldCurves, evaluate as ev
from models import multimodalIntraInterModal as M
from oracle.detinit import det_init_, det_inputs
from oracle.model import OracleMultimodalModel

pytestmark = pytest.mark.gpu
SPEC, SENS = (0.8, 0.9, 0.95), (0.8, 0.9)


def assert_same_curves(a, b):
    for k in ("thr", "tp", "fp", "n_points", "pos", "neg"):
        assert getattr(a, k).dtype == getattr(b, k).dtype and np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(a.auc, b.auc, equal_nan=True)
    assert np.allclose(a.average_precision, b.average_precision, rtol=0, atol=1e-12, equal_nan=True)
    for name in ("youden", "sens_at_spec", "spec_at_sens"):
        ga, gb = getattr(a, name), getattr(b, name)
        assert np.array_equal(ga["index"], gb["index"]) and np.array_equal(ga["threshold"], gb["threshold"], equal_nan=True), name
        assert np.allclose(ga["value"], gb["value"], rtol=0, atol=1e-12, equal_nan=True), name


@pytest.mark.parametrize("kind", ["continuous", "eighths"])
def test_device_path_equals_the_host_path_and_scikit_learn(kind):
    metrics = pytest.importorskip("sklearn.metrics")
    probs, labels = co.fold(1000, 6, kind)
    labels[::13] = -1
    on_device = FoldCurves.from_probs(torch.from_numpy(probs).to(DEV), torch.from_numpy(labels).to(DEV), SPEC, SENS)
    assert_same_curves(on_device, FoldCurves.from_probs(probs, labels, SPEC, SENS))
    keep = labels >= 0
    for c in range(6):
        y, score = labels[keep] == c, probs[keep, c]
        for got, want in zip(on_device.roc(c), metrics.roc_curve(y, score, drop_intermediate=False)):
            assert np.array_equal(got, want), c
        for got, want in zip(on_device.precision_recall(c), metrics.precision_recall_curve(y, score)):
            assert np.array_equal(got, want), c
        assert abs(on_device.average_precision[c] - metrics.average_precision_score(y, score)) <= 1e-12
        assert abs(on_device.auc[c] - metrics.roc_auc_score(y, score)) <= 1e-12
    bad = torch.from_numpy(probs).to(DEV)
    bad[1, 2] = float("nan")                                          # row 1 counts (row 0 is dropped)
    with pytest.raises(ValueError, match="NaN"):
        FoldCurves.from_probs(bad, torch.from_numpy(labels).to(DEV))


def test_evaluate_model_with_curves_and_from_fold_dir(tmp_path):
    kw = dict(SMALL, attention_mecanism="crossattention")
    cpu = det_init_(OracleMultimodalModel(**dict(kw, device="cpu")))
    hip = M.MultimodalModel(**dict(kw, device=DEV))
    hip.load_state_dict(cpu.state_dict(), strict=True)
    hip = hip.to(DEV)
    img, meta, lab = det_inputs(13, 32, 20, 6)
    names = [f"lesion_{i}.png" for i in range(13)]
    loader = [(names[a:b], img[a:b], meta[a:b], lab[a:b]) for a, b in ((0, 5), (5, 10), (10, 13))]
    metrics, labels, preds, probs = ev.evaluate_model(hip, loader, None, DEV, 2, str(tmp_path), "custom-cnn", extras=True, curves=True)
    fc = metrics["curves"]
    assert isinstance(fc, FoldCurves)
    assert_same_curves(fc, FoldCurves.from_probs(probs, labels))
    assert np.array_equal(fc.auc, metrics["per_class_auc"], equal_nan=True)
    folder = os.path.join(str(tmp_path), "custom-cnn_fold_2")
    assert os.path.exists(os.path.join(folder, "curves.npz"))
    assert np.array_equal(np.load(os.path.join(folder, "curves.npz"))["tp"], fc.tp)
    assert_same_curves(fc, FoldCurves.from_fold_dir(folder))
    plain = ev.evaluate_model(hip, loader, None, DEV, 3, str(tmp_path), "custom-cnn", extras=True)[0]
    assert "curves" not in plain and "curves.npz" not in os.listdir(os.path.join(str(tmp_path), "custom-cnn_fold_3"))
    for k in plain:
        if k != "fold":
            assert np.array_equal(np.asarray(plain[k]), np.asarray(metrics[k]), equal_nan=True), k
