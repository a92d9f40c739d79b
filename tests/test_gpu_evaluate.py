"""-m gpu: the one-vs-rest AUC kernel (csrc/auc.hip) through mmskin.evaluate.ovr_auc_counts against the integer counts of the numpy
restatement tests/evaluate_oracle.py (which tests/test_cpu_evaluate.py pins to values recorded from the reference's own
evaluate_model), and evaluate_model end to end on the device.

The counts are integers: every comparison of them is exact.  The AUC is a float64 sum of at most C ratios of those integers on
either side: 1e-12 absolute, rounding only.  The end-to-end probabilities are held to the bound tests/test_gpu_model.py uses for
the fp32 logits of the custom-cnn encoder (rtol 1e-3, atol 1e-5)."""
import numpy as np
import pytest
import torch

import evaluate_oracle as eo
from gpu_util import DEV
from helpers import SMALL
from mmskin import evaluate as ev
from mmskin._lib import MMSkinError
from models import multimodalIntraInterModal as M
from oracle.detinit import det_init_, det_inputs
from oracle.model import OracleMultimodalModel

pytestmark = pytest.mark.gpu
DISCRETE, same = eo.DISCRETE, eo.same

# N: one row, one wave and its neighbours, one workgroup of 256 rows and its neighbours, several workgroups, a prime.
# C: tile heights 256 (C <= 32) and 204 (C = 40); C = 1024: 8-row tiles; N = 20011: 79 row blocks x 26 chunks of the j range.
SHAPES = [(N, C) for C in (2, 3, 7, 40) for N in (1, 2, 63, 64, 65, 255, 256, 257, 513, 1031)] + [(70, 1024), (20011, 6)]


def scores(N, C, seed=0, levels=None):
    """fp32 scores in [0, 1); with `levels` only that many distinct values (ties)"""
    rng = np.random.default_rng(seed + 1000 * N + C)
    p = rng.random((N, C)).astype(np.float32)
    if levels:
        p = (np.floor(p * levels) / levels).astype(np.float32)
    return p, rng.integers(0, C, N).astype(np.int64)


def device_counts(probs, labels):
    return ev.ovr_auc_counts(torch.from_numpy(probs).to(DEV), torch.from_numpy(labels).to(DEV))


def assert_counts_equal(got, want, what):
    for k in ("pos", "neg", "wins2"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (what, k, got[k][:8], want[k][:8])
    assert got["nan"] == want["nan"], (what, got["nan"], want["nan"])


@pytest.mark.parametrize("N,C", SHAPES)
def test_counts_equal_the_oracle_exactly(N, C):
    probs, labels = scores(N, C, levels=64 if N % 2 else None)        # odd N: quantised scores, so ties occur
    got, want = device_counts(probs, labels), eo.counts(probs, labels)
    assert_counts_equal(got, want, (N, C))
    assert int(want["pos"].sum()) == N and np.array_equal(want["pos"] + want["neg"], np.full(C, N))
    assert same(ev.auc_from_counts(got, C), eo.auc(want), 1e-12)


def test_constant_column_and_perfect_separation():
    N, C = 513, 7
    probs, labels = scores(N, C, seed=1)
    probs[:, 3] = 0.25                                                # every pair of class 3 ties
    probs[:, 5] = np.where(labels == 5, 0.75, 0.5) + 0.125 * probs[:, 5]      # every positive of class 5 above every negative
    got = device_counts(probs, labels)
    assert_counts_equal(got, eo.counts(probs, labels), "constant / separated")
    assert got["pos"][3] > 0 and got["wins2"][3] == got["pos"][3] * got["neg"][3]
    assert got["pos"][5] > 0 and got["wins2"][5] == 2 * got["pos"][5] * got["neg"][5]
    auc = ev.per_class_auc(got)
    assert auc[3] == 0.5 and auc[5] == 1.0


def test_heavy_ties():
    N, C = 1031, 3
    probs, labels = scores(N, C, seed=2, levels=4)
    assert len(np.unique(probs)) == 4
    assert_counts_equal(device_counts(probs, labels), eo.counts(probs, labels), "four values")


def test_labels_outside_the_range_are_ignored():
    N, C = 257, 7
    probs, labels = scores(N, C, seed=3, levels=32)
    labels[::5] = -1
    labels[3::7] = C
    labels[256] = -100
    got, want = device_counts(probs, labels), eo.counts(probs, labels)
    assert_counts_equal(got, want, "ignored")
    keep = (labels >= 0) & (labels < C)
    assert 0 < keep.sum() < N
    assert_counts_equal(got, eo.counts(probs[keep], labels[keep]), "ignored rows removed")


def test_nan_entries_are_counted_and_make_the_auc_none():
    N, C = 65, 3
    probs, labels = scores(N, C, seed=4)
    probs[5, 0] = probs[5, 2] = probs[64, 1] = np.nan
    probs[9, 1] = np.nan
    labels[9] = -1                                                    # the NaN of an ignored row does not count
    got, want = device_counts(probs, labels), eo.counts(probs, labels)
    assert want["nan"] == 3
    assert_counts_equal(got, want, "nan")
    assert ev.auc_from_counts(got, C) is None


def test_two_runs_are_bitwise_equal():
    N, C = 1031, 40
    probs, labels = scores(N, C, seed=5, levels=16)
    p, y = torch.from_numpy(probs).to(DEV), torch.from_numpy(labels).to(DEV)
    a, b = ev.ovr_auc_counts(p, y), ev.ovr_auc_counts(p, y)
    assert_counts_equal(a, b, "repeat")


def test_empty_and_non_contiguous_inputs_raise():
    with pytest.raises(MMSkinError, match="rows"):
        ev.ovr_auc_counts(torch.zeros(0, 6, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV))
    with pytest.raises(MMSkinError, match="contiguous"):
        ev.ovr_auc_counts(torch.rand(6, 64, device=DEV).t(), torch.zeros(64, dtype=torch.int64, device=DEV))
    with pytest.raises(MMSkinError, match="classes"):
        ev.ovr_auc_counts(torch.rand(8, 1, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV))


def test_evaluate_model_end_to_end(tmp_path):
    kw = dict(SMALL, attention_mecanism="crossattention")
    cpu = det_init_(OracleMultimodalModel(**dict(kw, device="cpu")))
    hip = M.MultimodalModel(**dict(kw, device=DEV))
    hip.load_state_dict(cpu.state_dict(), strict=True)
    hip = hip.to(DEV)
    img, meta, lab = det_inputs(13, 32, 20, 6)
    names = [f"lesion_{i}.png" for i in range(13)]
    loader = [(names[a:b], img[a:b], meta[a:b], lab[a:b]) for a, b in ((0, 5), (5, 10), (10, 13))]      # a plain list of batches

    metrics, labels, preds, probs, got_names = ev.evaluate_model(hip, loader, None, DEV, 2, str(tmp_path), "custom-cnn", extras=True,
                                                                 image_names=True)
    assert not hip.training and got_names == names
    assert np.array_equal(labels, lab.numpy()) and probs.shape == (13, 6) and probs.dtype == np.float32
    confusion = np.zeros((6, 6), dtype=np.int64)
    np.add.at(confusion, (labels, preds), 1)
    assert np.array_equal(metrics["confusion"], confusion), "the returned predictions do not reproduce the meter's confusion matrix"
    want = eo.metrics(labels, preds, probs)
    for k in DISCRETE + ("auc",):
        print(f"end to end {k}: got {metrics[k]!r} oracle {want[k]!r}")
        assert same(metrics[k], want[k], 1e-12), (k, metrics[k], want[k])
    assert np.allclose(metrics["per_class_auc"], eo.per_class_auc(eo.counts(probs, labels)), rtol=0, atol=1e-15, equal_nan=True)
    for file, arr in (("labels", labels), ("predictions", preds), ("probabilities", probs), ("targets", np.arange(6))):
        assert np.array_equal(np.load(tmp_path / "custom-cnn_fold_2" / (file + ".npy")), arr), file

    # the same loader through a CPU copy of the model: the host paths throughout
    cpu_metrics, cpu_labels, cpu_preds, cpu_probs = ev.evaluate_model(cpu, loader, None, "cpu", 2, str(tmp_path), "cpu-copy", extras=True)
    err = np.abs(probs.astype(np.float64) - cpu_probs)
    print(f"end to end: max |prob diff| device vs CPU copy = {err.max():.3e}; loss {metrics['loss']:.7f} vs {cpu_metrics['loss']:.7f}")
    assert np.array_equal(cpu_labels, labels)
    assert np.allclose(probs, cpu_probs, rtol=1e-3, atol=1e-5), err.max()
