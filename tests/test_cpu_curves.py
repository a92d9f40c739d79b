"""CPU: tests/curves_oracle.py and the host path of mmskin.curves.FoldCurves against scikit-learn and against each other.

Bounds.  The integer arrays, the thresholds and the indices of the operating points are compared exactly.  The curve arrays
(fpr, tpr, precision, recall) are one float64 division of the same two integers on either side: exact.  The AUC against
roc_auc_score and the average precision against average_precision_score are float64 sums of at most N non-negative terms in
another order: 1e-12 absolute on values in [0, 1].  The AUC against evaluate.per_class_auc: bit for bit."""
import os
import re
import warnings

import numpy as np
import pytest
import torch

import curves_oracle as co
import evaluate_oracle as eo
from mmskin import FoldCurves, _lib, curves as cv_mod, evaluate as ev, ops
from mmskin._lib import MMSkinError

SPEC, SENS = (0.8, 0.9, 0.95), (0.8, 0.9, 0.95)
CASES = [(1, 2, "continuous"), (2, 2, "eighths"), (65, 3, "continuous"), (257, 6, "eighths"), (257, 3, "constant"), (130, 4, "separable"),
         (300, 11, "continuous"), (300, 11, "eighths")]


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def check_against_oracle(fc, probs, labels, spec=SPEC, sens=SENS):
    want = co.curves(probs, labels)
    for k in ("thr", "tp", "fp", "n_points", "pos", "neg"):
        got = getattr(fc, k)
        assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), k
    s = co.summary(want, spec, sens)
    assert same(fc.auc, s["auc"])
    both = ~np.isnan(s["average_precision"])
    assert np.array_equal(np.isnan(fc.average_precision), ~both)
    assert np.abs(fc.average_precision[both] - s["average_precision"][both]).max(initial=0.0) <= 1e-12
    for name, group in (("youden", fc.youden), ("sens_at_spec", fc.sens_at_spec), ("spec_at_sens", fc.spec_at_sens)):
        assert group["index"].dtype == np.int64 and np.array_equal(group["index"], s[name + "_index"]), name
        assert same(group["threshold"], s[name + "_threshold"]), name
        ok = ~np.isnan(s[name + "_value"])
        assert np.array_equal(np.isnan(group["value"]), ~ok), name
        assert np.abs(group["value"][ok] - s[name + "_value"][ok]).max(initial=0.0) <= 1e-12, name
    return want, s


@pytest.mark.parametrize("N,C,kind", CASES)
def test_host_path_equals_the_oracle(N, C, kind):
    probs, labels = co.fold(N, C, kind)
    fc = FoldCurves.from_probs(probs, labels, SPEC, SENS)
    want, s = check_against_oracle(fc, probs, labels)
    if kind == "constant":
        assert (fc.n_points == 1).all()
    # the trapezoid area is the integer behind the existing AUC, and the AUC is that of evaluate bit for bit
    counts = ev.ovr_auc_counts(torch.from_numpy(probs), torch.from_numpy(labels))
    assert np.array_equal(s["wins2"], counts["wins2"])
    assert same(fc.auc, ev.per_class_auc(counts))


@pytest.mark.parametrize("N,C,kind", [c for c in CASES if c[0] >= 65])
def test_oracle_and_host_path_equal_scikit_learn(N, C, kind):
    metrics = pytest.importorskip("sklearn.metrics")
    probs, labels = co.fold(N, C, kind)
    fc = FoldCurves.from_probs(torch.from_numpy(probs), torch.from_numpy(labels))
    s = co.summary(co.curves(probs, labels))
    for c in range(C):
        y, score = labels == c, probs[:, c]
        fpr, tpr, thr = metrics.roc_curve(y, score, drop_intermediate=False)
        got = fc.roc(c)
        assert np.array_equal(got[0], fpr) and np.array_equal(got[1], tpr) and np.array_equal(got[2], thr), c
        precision, recall, thr = metrics.precision_recall_curve(y, score)
        got = fc.precision_recall(c)
        assert np.array_equal(got[0], precision) and np.array_equal(got[1], recall) and np.array_equal(got[2], thr), c
        for mine in (fc.average_precision[c], s["average_precision"][c]):
            assert abs(mine - metrics.average_precision_score(y, score)) <= 1e-12, c
        for mine in (fc.auc[c], s["auc"][c]):
            assert abs(mine - metrics.roc_auc_score(y, score)) <= 1e-12, c


def test_youden_and_operating_points_against_the_sklearn_curve():
    metrics = pytest.importorskip("sklearn.metrics")
    probs, labels = co.fold(257, 6, "eighths")
    fc = FoldCurves.from_probs(probs, labels, SPEC, SENS)
    for c in range(6):
        fpr, tpr, thr = metrics.roc_curve(labels == c, probs[:, c], drop_intermediate=False)
        k = fc.youden["index"][c]
        assert abs(fc.youden["value"][c] - (tpr[1:] - fpr[1:]).max()) <= 1e-12 and fc.youden["threshold"][c] == thr[1 + k]
        for a, q in enumerate(SPEC):
            ok = 1.0 - fpr >= q - 1e-12
            assert abs(fc.sens_at_spec["value"][c, a] - tpr[ok].max()) <= 1e-12
        for b, t in enumerate(SENS):
            ok = tpr >= t - 1e-12
            assert abs(fc.spec_at_sens["value"][c, b] - (1.0 - fpr[ok]).max()) <= 1e-12


def test_a_class_without_positives_or_without_negatives_is_nan():
    probs, labels = co.fold(120, 4, "continuous")
    labels[labels == 2] = 1                                           # class 2 has no positive row
    fc = FoldCurves.from_probs(probs, labels, SPEC, SENS)
    only = np.zeros(40, dtype=np.int64)                               # two classes, every row of class 0: no negative for 0, no positive for 1
    fc2 = FoldCurves.from_probs(co.fold(40, 2, "continuous")[0], only, SPEC, SENS)
    for f, classes in ((fc, [2]), (fc2, [0, 1])):
        for c in classes:
            assert np.isnan(f.auc[c]) and np.isnan(f.average_precision[c])
            for group in (f.youden, f.sens_at_spec, f.spec_at_sens):
                assert np.isnan(group["value"][c]).all() and np.isnan(group["threshold"][c]).all() and (group["index"][c] == -1).all()
            assert f.n_points[c] > 0 and f.tp[c, f.n_points[c] - 1] == f.pos[c] and f.fp[c, f.n_points[c] - 1] == f.neg[c]
    assert fc.pos[2] == 0 and fc2.neg[0] == 0 and fc2.pos[1] == 0
    assert not np.isnan(fc.auc[[0, 1, 3]]).any()
    check_against_oracle(fc, probs, labels)


def test_labels_outside_the_range_are_dropped():
    probs, labels = co.fold(200, 5, "eighths")
    dirty = labels.copy()
    dirty[::7], dirty[3::11] = -1, 5
    keep = (dirty >= 0) & (dirty < 5)
    a, b = FoldCurves.from_probs(probs, dirty), FoldCurves.from_probs(probs[keep], dirty[keep])
    assert (a.pos + a.neg == keep.sum()).all() and a.thr.shape == (5, 200) and b.thr.shape == (5, int(keep.sum()))
    n = b.thr.shape[1]
    for k in ("thr", "tp", "fp"):
        assert np.array_equal(getattr(a, k)[:, :n], getattr(b, k)) and not getattr(a, k)[:, n:].any(), k
    assert np.array_equal(a.n_points, b.n_points) and same(a.auc, b.auc) and same(a.average_precision, b.average_precision)
    check_against_oracle(a, probs, dirty)


def test_tie_rule_with_a_point_exactly_on_the_bound():
    """pos = 4, neg = 20.  The six points (scores 0.9, 0.8, 0.7, 0.6, 0.5, 0.1) have tp = 1, 1, 2, 3, 4, 4 and fp = 0, 1, 2, 2, 3, 20.
    q = 0.9: the bound 0.9 * 20 rounds to 18.0 in fp64, so the points with fp = 2 sit exactly on it and are admissible; the
    largest tp among the points 0 .. 3 is 3, at index 3.  q = 0.95: the bound is 19.0, the points 0 and 1 tie at tp = 1, the
    first wins.  Sensitivity 0.5: tp >= 2, first at index 2 (fp = 2); 1.0: tp >= 4, first at index 4; 0.0: index 0."""
    scores = np.asarray([0.9, 0.8, 0.7, 0.7, 0.6, 0.5, 0.5] + [0.1] * 17, dtype=np.float32)
    is_pos = np.asarray([1, 0, 1, 0, 1, 1, 0] + [0] * 17)
    probs = np.stack([scores, 1 - scores], axis=1)
    labels = np.where(is_pos == 1, 0, 1).astype(np.int64)
    spec, sens = (0.9, 0.95, 1.0), (0.5, 1.0, 0.0)
    fc = FoldCurves.from_probs(probs, labels, specificities=spec, sensitivities=sens)
    f32 = lambda v: float(np.float32(v))
    assert fc.pos[0] == 4 and fc.neg[0] == 20 and fc.n_points[0] == 6
    assert fc.tp[0, :6].tolist() == [1, 1, 2, 3, 4, 4] and fc.fp[0, :6].tolist() == [0, 1, 2, 2, 3, 20]
    assert fc.sens_at_spec["index"][0].tolist() == [3, 0, 0]
    assert fc.sens_at_spec["value"][0].tolist() == [0.75, 0.25, 0.25]
    assert fc.sens_at_spec["threshold"][0].tolist() == [f32(0.6), f32(0.9), f32(0.9)]
    assert fc.spec_at_sens["index"][0].tolist() == [2, 4, 0] and fc.spec_at_sens["value"][0].tolist() == [0.9, 0.85, 1.0]
    assert fc.spec_at_sens["threshold"][0].tolist() == [f32(0.7), f32(0.5), f32(0.9)]
    assert fc.youden["index"][0] == 4 and fc.youden["value"][0] == 68 / 80 and fc.youden["threshold"][0] == f32(0.5)
    check_against_oracle(fc, probs, labels, spec, sens)
    # no admissible point: the first point already has a false positive
    flipped = FoldCurves.from_probs(probs[:, ::-1].copy(), labels, specificities=(1.0,), sensitivities=())
    assert flipped.fp[0, 0] > 0 and flipped.sens_at_spec["index"][0, 0] == -1 and flipped.sens_at_spec["value"][0, 0] == 0.0
    assert flipped.sens_at_spec["threshold"][0, 0] == np.inf


def test_errors_are_the_same_on_either_kind_of_input():
    p, y = co.fold(8, 3, "continuous")
    for wrap in (lambda a: a, torch.from_numpy):
        with pytest.raises(ValueError, match=r"fp32 \[N, C\]"):
            FoldCurves.from_probs(wrap(p.astype(np.float64)), wrap(y))
        with pytest.raises(ValueError, match=r"fp32 \[N, C\]"):
            FoldCurves.from_probs(wrap(p[:, 0].copy()), wrap(y))
        with pytest.raises(ValueError, match="integer"):
            FoldCurves.from_probs(wrap(p), wrap(y[:7].copy()))
        with pytest.raises(ValueError, match="integer"):
            FoldCurves.from_probs(wrap(p), wrap(y.astype(np.float32)))
        with pytest.raises(ValueError, match="specificities"):
            FoldCurves.from_probs(wrap(p), wrap(y), specificities=(0.5, 1.5))
        with pytest.raises(ValueError, match="sensitivities"):
            FoldCurves.from_probs(wrap(p), wrap(y), sensitivities=(float("nan"),))
        with pytest.raises(MMSkinError, match="classes"):
            FoldCurves.from_probs(wrap(p[:, :1].copy()), wrap(y))
        with pytest.raises(MMSkinError, match="classes"):
            FoldCurves.from_probs(wrap(np.zeros((2, 1025), dtype=np.float32)), wrap(y[:2].copy()))
        with pytest.raises(MMSkinError, match="rows"):
            FoldCurves.from_probs(wrap(np.zeros((0, 3), dtype=np.float32)), wrap(np.zeros(0, dtype=np.int64)))
        with pytest.raises(MMSkinError, match="specificities"):
            FoldCurves.from_probs(wrap(p), wrap(y), specificities=[0.5] * (ops.CURVES_MAX_OPERATING_POINTS + 1))
    bad = p.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        FoldCurves.from_probs(bad, y)
    dropped = y.copy()
    dropped[2] = -1                                                   # the NaN of a dropped row does not count
    assert FoldCurves.from_probs(bad, dropped).pos.sum() == 7
    fc = FoldCurves.from_probs(p, y)
    with pytest.raises(ValueError, match="class"):
        fc.roc(3)
    with pytest.raises(MMSkinError, match="HIP device"):
        ops.ovr_curves(torch.from_numpy(p), torch.from_numpy(y))


def test_header_signatures_and_exports_agree_for_the_new_symbols():
    names = ("mmskin_ovr_curves", "mmskin_ovr_curves_summary", "mmskin_ovr_curves_scratch_ints", "mmskin_ovr_curves_summary_columns")
    lib = _lib.load()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name in names:
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols() and hasattr(lib, name), name
        decl = re.search(r"^(?:int|int64_t) " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert decl and len(decl.group(1).split(",")) == len(_lib._SIGNATURES[name][1]), name
    assert int(re.search(r"#define MMSKIN_CURVES_MAX_OPERATING_POINTS (\d+)", header).group(1)) == ops.CURVES_MAX_OPERATING_POINTS


def test_the_c_entries_check_their_range_without_a_gpu():
    lib = _lib.load()
    d = _lib.ptr(torch.zeros(64, dtype=torch.int64))
    for N, C, word in ((0, 6, "rows"), (2 ** 31, 6, "rows"), (8, 1, "classes"), (8, 1025, "classes")):
        assert lib.mmskin_ovr_curves(d, d, N, C, d, d, d, d, d, d, None) == 1                      # MMSKIN_ERR_ARG
        assert word in lib.mmskin_last_error().decode()
        assert lib.mmskin_ovr_curves_summary(d, d, d, d, d, N, C, d, 1, d, 1, d, None) == 1
        assert word in lib.mmskin_last_error().decode()
        assert lib.mmskin_ovr_curves_scratch_ints(N, C) == -1
    assert lib.mmskin_ovr_curves(None, d, 8, 6, d, d, d, d, d, d, None) == 1
    assert lib.mmskin_ovr_curves_summary(d, d, d, d, d, 8, 6, d, 9, d, 0, d, None) == 1
    assert "operating points" in lib.mmskin_last_error().decode()
    assert lib.mmskin_ovr_curves_summary_columns(3, 3) == 23 and lib.mmskin_ovr_curves_summary_columns(9, 0) == -1
    # the workspace: five [C][N] arrays and the block counts, each from a 256-byte boundary
    for N, C in ((1, 2), (1000, 6), (4097, 11)):
        cells, blocks = -(-N * C * 4 // 256) * 64, -(-(-(-N // 1024)) * C * 4 // 256) * 64
        assert lib.mmskin_ovr_curves_scratch_ints(N, C) == 5 * cells + blocks, (N, C)


def test_evaluate_model_writes_the_curves_and_changes_nothing_else(tmp_path):
    logits, labels = eo.golden_inputs("c6_n97")
    run = lambda sub, **kw: ev.evaluate_model(eo.StoredLogits(torch.from_numpy(logits)), eo.loader_for(labels, (40, 40, 17)), None, "cpu", 2,
                                              str(tmp_path / sub), "stub", **kw)
    plain, with_curves = run("a", extras=True), run("b", extras=True, curves=True)
    assert "curves" not in plain[0] and sorted(os.listdir(tmp_path / "a" / "stub_fold_2")) == ["labels.npy", "predictions.npy",
                                                                                              "probabilities.npy", "targets.npy"]
    fc = with_curves[0].pop("curves")
    assert isinstance(fc, FoldCurves) and tuple(plain[0]) == tuple(with_curves[0])
    for k, v in plain[0].items():
        assert np.array_equal(np.asarray(v), np.asarray(with_curves[0][k]), equal_nan=True), k
    for a, b in zip(plain[1:], with_curves[1:]):
        assert np.array_equal(a, b)
    folder = tmp_path / "b" / "stub_fold_2"
    assert sorted(os.listdir(folder)) == ["curves.npz", "labels.npy", "predictions.npy", "probabilities.npy", "targets.npy"]
    assert same(fc.auc, plain[0]["per_class_auc"])
    check_against_oracle(fc, with_curves[3], with_curves[1])
    saved = np.load(folder / cv_mod.FILE_NAME)
    for k in ("thr", "tp", "fp", "n_points", "pos", "neg", "auc", "average_precision", "specificities", "sensitivities"):
        assert np.array_equal(saved[k], getattr(fc, k), equal_nan=True), k
    for name, group in (("youden", fc.youden), ("sens_at_spec", fc.sens_at_spec), ("spec_at_sens", fc.spec_at_sens)):
        for k, v in group.items():
            assert np.array_equal(saved[f"{name}_{k}"], v, equal_nan=True), (name, k)
    again = FoldCurves.from_fold_dir(str(folder))
    assert np.array_equal(again.tp, fc.tp) and np.array_equal(again.thr, fc.thr) and same(again.auc, fc.auc)


def test_nan_probabilities_give_no_curves_in_evaluate_model(tmp_path):
    logits, labels = eo.golden_inputs("c6_n97")
    logits[3, 1] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        metrics = ev.evaluate_model(eo.StoredLogits(torch.from_numpy(logits)), eo.loader_for(labels, (97,)), None, "cpu", 0, str(tmp_path),
                                    curves=True)[0]
    assert metrics["auc"] is None and metrics["curves"] is None
    assert "curves.npz" not in os.listdir(tmp_path / "None_fold_0")
