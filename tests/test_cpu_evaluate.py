"""CPU: mmskin.evaluate on its host paths against tests/golden/evaluate.json (recorded from the reference's own evaluate_model
with scikit-learn) and against the independent restatement tests/evaluate_oracle.py.

Bounds.  The discrete metrics are ratios of small integers, formed once in float64 on either side: 1e-12 absolute.  The AUC is,
on either side, a float64 sum of at most N C terms in [0, 1] divided by an exactly known integer: rounding only, 1e-12
absolute.  The integer counts are compared exactly; NaN equals NaN."""
import math
import os

import numpy as np
import pytest
import torch

import evaluate_oracle as eo
from mmskin import evaluate as ev
from mmskin._lib import MMSkinError

DISCRETE, same = eo.DISCRETE, eo.same
KEYS = ("fold",) + DISCRETE + ("auc",)


class SizedLoader(list):
    """a list of batches that, like a DataLoader, knows its dataset's length"""

    def __init__(self, batches, rows):
        super().__init__(batches)
        self.dataset = range(rows)


def run_case(case, tmp_path, sized, **kw):
    logits = torch.tensor(case["logits"], dtype=torch.float64).float()
    labels = np.asarray(case["labels"], dtype=np.int64)
    loader = eo.loader_for(labels, case["batches"])
    if sized:
        loader = SizedLoader(loader, len(labels))
    return ev.evaluate_model(eo.StoredLogits(logits), loader, None, "cpu", 3, str(tmp_path), "stub", **kw)


def test_oracle_reproduces_the_reference_metrics_on_its_own_outputs():
    """the yardstick itself: the numpy restatement on the reference's labels / predictions / probabilities gives the reference's
    metrics, so a GPU test that holds the kernel to the oracle holds it to the reference"""
    gold = eo.golden()
    assert sorted(gold["cases"]) == sorted(eo.GOLDEN_CASES)
    for name, case in gold["cases"].items():
        probs = np.asarray(case["probabilities"]).astype(np.float32)
        got = eo.metrics(case["labels"], case["predictions"], probs)
        for k in DISCRETE + ("auc",):
            print(f"{name} {k}: oracle {got[k]!r} reference {case['metrics'][k]!r}")
            assert same(got[k], case["metrics"][k]), (name, k, got[k], case["metrics"][k])
        small = eo.counts(probs, case["labels"])
        brute = eo.counts_brute(probs, case["labels"])
        assert all(np.array_equal(small[k], brute[k]) for k in ("pos", "neg", "wins2")) and small["nan"] == brute["nan"] == 0
    assert math.isnan(gold["cases"]["c3_single_class"]["metrics"]["auc"])


@pytest.mark.parametrize("sized", [False, True], ids=["concatenated", "preallocated"])
@pytest.mark.parametrize("name", eo.GOLDEN_CASES)
def test_host_path_reproduces_every_golden_metric_and_writes_the_arrays(name, sized, tmp_path):
    case = eo.golden()["cases"][name]
    metrics, labels, preds, probs = run_case(case, tmp_path, sized)
    assert tuple(metrics) == KEYS and metrics["fold"] == 3
    for k in DISCRETE + ("auc",):
        print(f"{name} {k}: got {metrics[k]!r} reference {case['metrics'][k]!r}")
        assert same(metrics[k], case["metrics"][k]), (name, k, metrics[k], case["metrics"][k])
    assert labels.dtype == np.int64 and preds.dtype == np.int64 and probs.dtype == np.float32
    assert np.array_equal(labels, case["labels"]) and np.array_equal(preds, case["predictions"])
    # the soft-max rows: the reference's are torch.softmax in fp32 as well, another order of the C-term sum; C + 2 roundings of 2^-24
    C = probs.shape[1]
    assert np.abs(probs.astype(np.float64) - np.asarray(case["probabilities"])).max() <= (C + 2) * 2.0 ** -24
    folder = os.path.join(str(tmp_path), "stub_fold_3")
    assert sorted(os.listdir(folder)) == ["labels.npy", "predictions.npy", "probabilities.npy", "targets.npy"]
    for file, want in (("labels", labels), ("predictions", preds), ("probabilities", probs), ("targets", np.arange(C))):
        got = np.load(os.path.join(folder, file + ".npy"))
        assert got.dtype == want.dtype and np.array_equal(got, want), file


def test_extras_image_names_and_targets(tmp_path):
    case = eo.golden()["cases"]["c6_n97"]
    targets = ["ACK", "BCC", "MEL", "NEV", "SCC", "SEK", "one too many"]
    logits = torch.tensor(case["logits"], dtype=torch.float64).float()
    labels = np.asarray(case["labels"], dtype=np.int64)
    out = ev.evaluate_model(eo.StoredLogits(logits), eo.loader_for(labels, case["batches"]), targets, "cpu", 1, str(tmp_path), extras=True,
                            image_names=True)
    metrics, got_labels, preds, probs, names = out
    assert names == [f"img_{i:04d}.png" for i in range(97)]
    assert tuple(metrics) == KEYS + ("loss", "confusion", "per_class_auc")
    want_cm = np.zeros((6, 6), dtype=np.int64)
    np.add.at(want_cm, (got_labels, preds), 1)
    assert np.array_equal(metrics["confusion"], want_cm)
    want_loss = float(torch.nn.functional.cross_entropy(logits.double(), torch.from_numpy(labels)))
    assert abs(metrics["loss"] - want_loss) <= 1e-6 * max(1.0, want_loss)             # three fp32 batch means against one float64 mean
    oracle_auc = eo.per_class_auc(eo.counts(probs, got_labels))
    assert np.allclose(metrics["per_class_auc"], oracle_auc, rtol=0, atol=1e-15)
    assert np.array_equal(np.load(os.path.join(str(tmp_path), "None_fold_1", "targets.npy")), np.array(targets)[:6])


def random_case(rng, N, C, levels=None, absent=()):
    probs = rng.random((N, C)).astype(np.float32)
    if levels:
        probs = (np.floor(probs * levels) / levels).astype(np.float32)
    labels = rng.integers(0, C, N)
    for c in absent:
        labels[labels == c] = (c + 1) % C
    return probs, labels.astype(np.int64)


CASES = [(1, 2, None, ()), (2, 2, None, ()), (97, 6, None, ()), (97, 6, 4, ()), (300, 7, 16, (3,)), (64, 2, 3, ()), (513, 40, 8, (0, 39)),
         (70, 1024, 5, ()), (2000, 3, None, (1, 2))]


@pytest.mark.parametrize("N,C,levels,absent", CASES)
def test_host_counts_equal_the_oracle_exactly(N, C, levels, absent):
    probs, labels = random_case(np.random.default_rng(N + C), N, C, levels, absent)
    labels[::11] = -1                                                 # ignored rows
    labels[5::13] = C
    got = ev.ovr_auc_counts(torch.from_numpy(probs), torch.from_numpy(labels))
    want = eo.counts(probs, labels)
    for k in ("pos", "neg", "wins2"):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), k
    assert got["nan"] == want["nan"] == 0
    if N <= 600 and C <= 40:
        assert np.array_equal(want["wins2"], eo.counts_brute(probs, labels)["wins2"])
    assert same(ev.auc_from_counts(got, C), eo.auc(want), 1e-15)


@pytest.mark.parametrize("N,C,levels,absent", [c for c in CASES if c[0] >= 64 and c[1] <= 40])
def test_auc_from_counts_matches_roc_auc_score(N, C, levels, absent):
    metrics = pytest.importorskip("sklearn.metrics")
    from sklearn.preprocessing import label_binarize
    import warnings
    probs, labels = random_case(np.random.default_rng(7 * N + C), N, C, levels, absent)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if C == 2:
            want = metrics.roc_auc_score(labels, probs[:, 1])
        else:
            want = metrics.roc_auc_score(label_binarize(labels, classes=np.arange(C)), probs, average="weighted", multi_class="ovr")
    got = ev.auc_from_counts(ev.ovr_auc_counts(torch.from_numpy(probs), torch.from_numpy(labels)), C)
    print(f"N={N} C={C} levels={levels}: auc {got!r} sklearn {want!r}")
    assert same(got, float(want))


def test_a_nan_probability_gives_none_and_is_counted():
    probs, labels = random_case(np.random.default_rng(5), 50, 6)
    probs[7, 2] = np.nan
    probs[9, 0] = np.nan
    labels[9] = -1                                                    # an ignored row's NaN does not count
    counts = ev.ovr_auc_counts(torch.from_numpy(probs), torch.from_numpy(labels))
    want = eo.counts(probs, labels)
    assert counts["nan"] == want["nan"] == 1 and ev.auc_from_counts(counts, 6) is None and eo.auc(want) is None
    assert np.array_equal(counts["wins2"], want["wins2"]) and np.array_equal(want["wins2"], eo.counts_brute(probs, labels)["wins2"])


def test_nan_logits_make_the_metric_none_as_the_reference(tmp_path, capsys):
    logits, labels = eo.golden_inputs("c6_n97")
    logits[3, 1] = np.nan
    metrics = ev.evaluate_model(eo.StoredLogits(torch.from_numpy(logits)), eo.loader_for(labels, (97,)), None, "cpu", 0, str(tmp_path))[0]
    assert metrics["auc"] is None and "[WARN] AUC computation failed" in capsys.readouterr().out


def test_bad_shapes_raise(tmp_path):
    p, y = torch.rand(8, 3), torch.randint(0, 3, (8,))
    with pytest.raises(ValueError, match=r"fp32 \[N, C\]"):
        ev.ovr_auc_counts(p.double(), y)
    with pytest.raises(ValueError, match=r"fp32 \[N, C\]"):
        ev.ovr_auc_counts(p[:, 0], y)
    with pytest.raises(ValueError, match="integer"):
        ev.ovr_auc_counts(p, y[:7])
    with pytest.raises(ValueError, match="integer"):
        ev.ovr_auc_counts(p, y.float())
    with pytest.raises(MMSkinError, match="contiguous"):
        ev.ovr_auc_counts(torch.rand(3, 8).t(), y)
    with pytest.raises(MMSkinError, match="outside"):
        ev.ovr_auc_counts(torch.rand(0, 3), torch.zeros(0, dtype=torch.int64))
    with pytest.raises(MMSkinError, match="outside"):
        ev.ovr_auc_counts(torch.rand(8, 1), y)
    with pytest.raises(MMSkinError, match="outside"):
        ev.ovr_auc_counts(torch.rand(2, 1025), y[:2])
    with pytest.raises(ValueError, match="num_classes"):
        ev.auc_from_counts(ev.ovr_auc_counts(p, y), 4)
    with pytest.raises(ValueError, match="no batch"):
        ev.evaluate_model(eo.StoredLogits(p), [], None, "cpu", 0, str(tmp_path))
    short = SizedLoader(eo.loader_for(y.numpy(), (8,)), 5)
    with pytest.raises(ValueError, match="more than"):
        ev.evaluate_model(eo.StoredLogits(p), short, None, "cpu", 0, str(tmp_path))


def test_the_c_entry_checks_its_range_without_a_gpu():
    from mmskin import _lib
    lib = _lib.load()
    dummy = torch.zeros(8, dtype=torch.int64)
    for N, C, word in ((0, 6, "rows"), (2 ** 31, 6, "rows"), (8, 1, "classes"), (8, 1025, "classes")):
        assert lib.mmskin_ovr_auc_counts(_lib.ptr(dummy), _lib.ptr(dummy), N, C, _lib.ptr(dummy), None) == 1      # MMSKIN_ERR_ARG
        assert word in lib.mmskin_last_error().decode()
    assert lib.mmskin_ovr_auc_counts(None, _lib.ptr(dummy), 8, 6, _lib.ptr(dummy), None) == 1


def test_drop_in_module_name():
    from utils import model_metrics
    assert model_metrics.evaluate_model is ev.evaluate_model
