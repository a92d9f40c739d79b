"""mmskin.bootstrap.BootstrapMetrics on the device against tests/bootstrap_oracle.py: a whole study, the rare-class NaN pattern,
cuts, the paired comparison, the limits, from_fold_dir and repeatability."""
import numpy as np
import pytest
import torch

import bootstrap_oracle as bo
from mmskin import ops
from mmskin._lib import MMSkinError
from mmskin.bootstrap import BootstrapMetrics

pytestmark = pytest.mark.gpu
TOL = 1e-12
NAMES = bo.METRICS + bo.CLASS_METRICS


def rare_fold(seed=0):
    """N = 60, K = 3, class 2 holds 2 rows; scores quantised to 1/8"""
    rng = np.random.default_rng(21 + seed)
    labels = np.array([0] * 30 + [1] * 28 + [2] * 2, dtype=np.int64)
    rng.shuffle(labels)
    raw = rng.random((60, 3)) + 0.6 * np.eye(3)[labels]
    return (np.round(raw / raw.sum(axis=1, keepdims=True) * 8) / 8).astype(np.float32), labels


def as_table(d, K):
    """a result's dict -> [7 + 2 K, ...] in the column order of the oracle"""
    return np.concatenate([np.stack([np.asarray(d[m]) for m in bo.METRICS])] + [np.moveaxis(np.asarray(d[m]), -1, 0) for m in bo.CLASS_METRICS])


def assert_same(a, b):
    for field in ("point", "mean", "std", "low", "high", "n_valid", "replicates"):
        for m in NAMES:
            assert np.array_equal(np.asarray(getattr(a, field)[m]), np.asarray(getattr(b, field)[m]), equal_nan=True), (field, m)


@pytest.fixture(scope="module")
def rare():
    scores, labels = rare_fold()
    B, seed = 64, 5
    point, table, confusion, counts, w = bo.study(scores, labels, None, seed, B)
    return scores, labels, B, seed, point, table, confusion, counts


def test_rare_class_nan_pattern_and_summary(rare):
    scores, labels, B, seed, point, table, confusion, counts = rare
    K = 3
    recall2 = table[7 + 2]
    assert np.isnan(recall2).any() and (~np.isnan(recall2)).any()           # the oracle: some replicates draw no row of class 2
    res = BootstrapMetrics(B, seed=seed, confidence=0.9).evaluate(scores, labels, return_counts=True)
    assert np.array_equal(res.confusion, confusion)
    assert np.array_equal(np.concatenate([res.counts[k] for k in ("pos", "neg", "wins2")], axis=1), counts)
    got = as_table(res.replicates, K)
    assert got.shape == table.shape
    assert np.array_equal(np.isnan(got), np.isnan(table))
    assert np.nanmax(np.abs(got - table)) <= TOL
    want = bo.summary(table, 0.9)
    assert np.array_equal(as_table(res.n_valid, K), want[0])
    assert res.n_valid["per_class_recall"][2] == int((~np.isnan(recall2)).sum()) < B
    for k, field in enumerate(("mean", "std", "low", "high"), start=1):
        have = as_table(getattr(res, field), K)
        assert np.array_equal(np.isnan(have), np.isnan(want[k])) and np.nanmax(np.abs(have - want[k])) <= TOL, field
    assert np.nanmax(np.abs(as_table(res.point, K) - point[:, 0])) <= TOL
    assert res.interval("auc") == (res.low["auc"], res.high["auc"])
    strat = BootstrapMetrics(B, seed=seed, stratified=True).evaluate(scores, labels)
    for m in NAMES:
        assert not np.isnan(strat.replicates[m]).any(), m
        assert (np.asarray(strat.n_valid[m]) == B).all(), m
    want_strat = bo.study(scores, labels, None, seed, B, stratified=True)[1]
    assert np.nanmax(np.abs(as_table(strat.replicates, K) - want_strat)) <= TOL


def test_cuts_and_repeatability(rare):
    scores, labels, B, seed = rare[:4]
    whole = BootstrapMetrics(B, seed=seed).evaluate(scores, labels)
    for step in (1, 7, B):
        assert_same(whole, BootstrapMetrics(B, seed=seed, replicates_per_call=step).evaluate(scores, labels))
    assert_same(whole, BootstrapMetrics(B, seed=seed).evaluate(torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()))
    other = BootstrapMetrics(B, seed=seed + 1).evaluate(scores, labels)
    assert not np.array_equal(whole.replicates["accuracy"], other.replicates["accuracy"])


def test_labels_out_of_range_are_dropped(rare):
    scores, labels, B, seed = rare[:4]
    more_scores = np.concatenate([scores[:3], scores])
    more_labels = np.concatenate([[-100, 3, 77], labels])
    assert_same(BootstrapMetrics(B, seed=seed).evaluate(scores, labels), BootstrapMetrics(B, seed=seed).evaluate(more_scores, more_labels))


def test_compare(rare):
    scores_a, labels, B, seed = rare[:4]
    scores_b = rare_fold(seed=1)[0]
    bs = BootstrapMetrics(B, seed=seed, confidence=0.9)
    cmp, a, b = bs.compare(scores_a, scores_b, labels), bs.evaluate(scores_a, labels), bs.evaluate(scores_b, labels)
    assert_same(cmp.a, a)
    assert_same(cmp.b, b)
    K = 3
    ta, tb = as_table(a.replicates, K), as_table(b.replicates, K)
    _, want_summary, want_p = bo.compare(ta, tb, 0.9)
    for m in NAMES:
        assert np.array_equal(cmp.replicates[m], a.replicates[m] - b.replicates[m], equal_nan=True), m
        assert np.array_equal(np.asarray(cmp.point[m]), np.asarray(a.point[m]) - np.asarray(b.point[m]), equal_nan=True), m
    assert np.array_equal(as_table(cmp.p_value, K), want_p)
    assert np.array_equal(as_table(cmp.n_valid, K), want_summary[0])
    for k, field in ((3, "low"), (4, "high")):
        have = as_table(getattr(cmp, field), K)
        assert np.array_equal(np.isnan(have), np.isnan(want_summary[k])) and np.nanmax(np.abs(have - want_summary[k])) <= TOL
    same = bs.compare(scores_a, scores_a, labels)
    for m in NAMES:
        d = same.replicates[m]
        assert (d[~np.isnan(d)] == 0).all() and (np.asarray(same.p_value[m]) == 1.0).all(), m


def test_limits_and_nan():
    bs = BootstrapMetrics(2, seed=1)
    N = ops.BOOTSTRAP_MAX_ROWS
    rng = np.random.default_rng(2)
    labels = rng.integers(0, 2, N).astype(np.int64)
    p1 = np.round(rng.random(N) * 64) / 64
    scores = np.stack([1 - p1, p1], axis=1).astype(np.float32)
    res = bs.evaluate(scores, labels, return_counts=True)
    _, table, confusion, counts, _ = bo.study(scores, labels, None, 1, 2)
    assert np.array_equal(res.confusion, confusion)
    assert np.array_equal(np.concatenate([res.counts[k] for k in ("pos", "neg", "wins2")], axis=1), counts)
    assert np.nanmax(np.abs(as_table(res.replicates, 2) - table)) <= TOL
    one_more = np.concatenate([scores, scores[:1]]), np.concatenate([labels, labels[:1]])
    with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_ROWS"):
        bs.evaluate(*one_more)
    for K in (65, 1):
        with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_CLASSES"):
            bs.evaluate(np.full((8, K), 1.0 / K, dtype=np.float32), np.zeros(8, dtype=np.int64))
    for B in (8193, 0):
        with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_RESAMPLES"):
            BootstrapMetrics(B)
        with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_RESAMPLES"):
            ops.bootstrap_accumulators(B, 2, "cuda:0")
    with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_ROWS"):
        ops.bootstrap_weights(0, N + 1, 2, "cuda:0")
    bad = scores[:100].copy()
    bad[17, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        bs.evaluate(bad, labels[:100])
    with pytest.raises(ValueError, match="NaN"):
        bs.evaluate(torch.from_numpy(bad).cuda(), torch.from_numpy(labels[:100]).cuda())


def test_from_fold_dir(tmp_path, rare):
    scores, labels, B, seed = rare[:4]
    preds = bo.first_argmax(scores)
    preds[:5] = (preds[:5] + 1) % 3                                          # the saved predictions are what is scored
    np.save(tmp_path / "probabilities.npy", scores)
    np.save(tmp_path / "labels.npy", labels)
    np.save(tmp_path / "predictions.npy", preds)
    bs = BootstrapMetrics(B, seed=seed)
    assert_same(bs.from_fold_dir(str(tmp_path)), bs.evaluate(scores, labels, preds))
    assert bs.evaluate(scores, labels, preds).point["accuracy"] != bs.evaluate(scores, labels).point["accuracy"]
