"""mmskin.subgroup.SubgroupAudit on the device against tests/subgroup_oracle.py: a whole audit on the balanced and the rare fold
(metrics, summaries, gaps, differences, p-values, the NaN pattern position by position), min_rows, cuts and repeatability, the paired
comparison of two models' gaps, from_fold_dir, by_name, and labels out of range dropped together with their group ids."""
import numpy as np
import pytest
import torch

import bootstrap_oracle as bo
import subgroup_oracle as so
from mmskin.subgroup import SubgroupAudit

pytestmark = pytest.mark.gpu
TOL = 1e-12
NAMES = so.METRICS + so.CLASS_METRICS
B, SEED, K, G = 32, 5, 3, 3
FIELDS = ("point", "mean", "std", "low", "high", "n_valid", "replicates")


def as_table(d, K=K):
    """a result's dict -> [7 + 4 K, ...] in the column order of the oracle"""
    return np.concatenate([np.stack([np.asarray(d[m]) for m in so.METRICS])] + [np.moveaxis(np.asarray(d[m]), -1, 0) for m in so.CLASS_METRICS])


def same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))             # position by position, nothing masked
    if (~np.isnan(want)).any():
        assert np.nanmax(np.abs(got - want)) <= TOL


def same_study(table, point, replicates, confidence):
    """a SubgroupTable against the oracle's point [M] and replicates [M, B]"""
    same(as_table(table.point), point)
    same(as_table(table.replicates), replicates)
    want = bo.summary(replicates, confidence)
    assert np.array_equal(as_table(table.n_valid), want[0])
    for k, field in enumerate(("mean", "std", "low", "high"), start=1):
        same(as_table(getattr(table, field)), want[k])


def assert_identical(a, b):
    tables = lambda r: [r.overall, *r.group, r.gap, r.lowest, r.highest]
    for ta, tb in zip(tables(a), tables(b)):
        for field in FIELDS:
            for m in NAMES:
                assert np.array_equal(np.asarray(getattr(ta, field)[m]), np.asarray(getattr(tb, field)[m]), equal_nan=True), (field, m)
    for m in NAMES:
        assert np.array_equal(a.lowest_share[m], b.lowest_share[m], equal_nan=True), m


@pytest.fixture(scope="module", params=[("balanced", True, 1), ("rare", False, 1), ("rare", False, 4)], ids=lambda p: f"{p[0]}-{p[1]}-{p[2]}")
def audited(request):
    kind, stratified, min_rows = request.param
    scores, labels, groups = so.balanced_fold() if kind == "balanced" else so.rare_fold()
    point, table, conf, counts, _ = so.study(scores, labels, None, groups, G, SEED, B, stratified, min_rows)
    fold = so.study(scores, labels, None, np.zeros(len(labels), dtype=np.int32), 1, SEED, B, stratified, min_rows)
    audit = SubgroupAudit(B, seed=SEED, confidence=0.9, stratified=stratified, min_rows=min_rows)
    res = audit.evaluate(scores, labels, groups, group_names=["II", "IV", "VI"], return_counts=True)
    return kind, stratified, min_rows, (scores, labels, groups), (point, table, conf, counts), fold, res


def test_groups_overall_and_gaps(audited):
    kind, stratified, min_rows, (scores, labels, groups), (point, table, conf, counts), fold, res = audited
    if kind == "balanced":
        assert not np.isnan(table).any()                              # the oracle: stratified, every group keeps every class
    else:
        assert np.isnan(table[1, 7 + 2]).all()                          # the oracle: group 1 holds no row of class 2
    assert res.num_groups == G and res.names == ["II", "IV", "VI"] and res.by_name("VI") is res.group[2]
    for g in range(G):
        t = res.group[g]
        same_study(t, point[g, :, 0], table[g], 0.9)
        assert np.array_equal(t.confusion, conf[:, g])
        assert np.array_equal(np.concatenate([t.counts[k] for k in ("pos", "neg", "wins2")], axis=1), counts[:, g])
        assert t.n_rows == int((groups == g).sum()) and np.array_equal(t.class_counts, np.bincount(labels[groups == g], minlength=K))
        if kind == "balanced":
            for m in NAMES:
                assert (np.asarray(t.n_valid[m]) == B).all(), m
    same_study(res.overall, fold[0][0, :, 0], fold[1][0], 0.9)
    assert res.overall.n_rows == len(labels)
    want_boot = bo.study(scores, labels, None, SEED, B, stratified)   # the fold's columns are BootstrapMetrics' own
    if min_rows == 1:
        same(as_table(res.overall.replicates)[:7 + 2 * K], want_boot[1])
    lowest, highest, gap, lowest_group = so.gaps(table)
    plow, phigh, pgap, _ = so.gaps(point)
    for t, p, r in ((res.lowest, plow, lowest), (res.highest, phigh, highest), (res.gap, pgap, gap)):
        same_study(t, p[:, 0], r, 0.9)
    total = lowest_group.sum(axis=1, keepdims=True).astype(np.float64)
    share = np.divide(lowest_group, total, out=np.full(lowest_group.shape, np.nan), where=total > 0)      # [M, G]
    for k, m in enumerate(so.METRICS):
        same(res.lowest_share[m], share[k])
    for j, m in enumerate(so.CLASS_METRICS):
        same(res.lowest_share[m], share[7 + j * K:7 + (j + 1) * K])
    if min_rows > 1:
        blank = np.isnan(res.group[2].replicates["accuracy"])
        assert blank.any() and not blank.all() and res.group[2].n_valid["accuracy"] == int((~blank).sum())


def test_paired_differences(audited):
    kind, stratified, min_rows, _, (point, table, _, _), fold, res = audited
    for a, b, ta, tb, pa, pb in ((0, 2, table[0], table[2], point[0], point[2]), ("IV", "II", table[1], table[0], point[1], point[0])):
        d = res.difference(a, b)
        want_delta, want_sum, want_p = bo.compare(ta, tb, 0.9)
        same(as_table(d.replicates), want_delta)
        same(as_table(d.point), (pa - pb)[:, 0])
        same(as_table(d.p_value), want_p)
        assert np.array_equal(as_table(d.n_valid), want_sum[0])
        for k, field in enumerate(("mean", "std", "low", "high"), start=1):
            same(as_table(getattr(d, field)), want_sum[k])
    v = res.versus_overall(2)
    want_delta, want_sum, want_p = bo.compare(table[2], fold[1][0], 0.9)
    same(as_table(v.replicates), want_delta)
    same(as_table(v.p_value), want_p)
    same(as_table(v.low), want_sum[3])
    same(as_table(v.point), (point[2] - fold[0][0])[:, 0])
    zero = res.difference(1, 1)
    for m in NAMES:
        r = zero.replicates[m]
        assert (r[~np.isnan(r)] == 0).all() and (np.asarray(zero.p_value[m]) == 1.0).all(), m
    with pytest.raises(KeyError):
        res.by_name("V")
    with pytest.raises(IndexError):
        res.difference(0, 3)


def test_cuts_and_repeatability():
    scores, labels, groups = so.rare_fold()
    whole = SubgroupAudit(B, seed=SEED).evaluate(scores, labels, groups)
    for step in (1, 7):
        assert_identical(whole, SubgroupAudit(B, seed=SEED, replicates_per_call=step).evaluate(scores, labels, groups))
    on_device = SubgroupAudit(B, seed=SEED).evaluate(*(torch.from_numpy(a).cuda() for a in (scores, labels, groups)))
    assert_identical(whole, on_device)
    other = SubgroupAudit(B, seed=SEED + 1).evaluate(scores, labels, groups)
    assert not np.array_equal(whole.group[0].replicates["accuracy"], other.group[0].replicates["accuracy"])
    assert whole.names == ["0", "1", "2"]


def test_labels_out_of_range_are_dropped_with_their_groups():
    scores, labels, groups = so.rare_fold()
    more = np.concatenate([scores[:3], scores]), np.concatenate([[-100, 3, 77], labels]), np.concatenate([[0, 1, 2], groups]).astype(np.int32)
    audit = SubgroupAudit(B, seed=SEED)
    assert_identical(audit.evaluate(scores, labels, groups), audit.evaluate(*more))


def test_compare_two_models_gaps():
    scores_a, labels, groups = so.balanced_fold()
    scores_b = np.roll(scores_a, 1, axis=0)                           # another model: the same rows' scores, shifted by one row
    audit = SubgroupAudit(B, seed=SEED, confidence=0.9)
    cmp = audit.compare(scores_a, scores_b, labels, groups)
    assert_identical(cmp.a, audit.evaluate(scores_a, labels, groups))
    assert_identical(cmp.b, audit.evaluate(scores_b, labels, groups))
    ta = so.study(scores_a, labels, None, groups, G, SEED, B)
    tb = so.study(scores_b, labels, None, groups, G, SEED, B)
    gap_a, gap_b = so.gaps(ta[1])[2], so.gaps(tb[1])[2]
    want_delta, want_sum, want_p = bo.compare(gap_a, gap_b, 0.9)
    same(as_table(cmp.replicates), want_delta)
    same(as_table(cmp.point), (so.gaps(ta[0])[2] - so.gaps(tb[0])[2])[:, 0])
    same(as_table(cmp.p_value), want_p)
    assert np.array_equal(as_table(cmp.n_valid), want_sum[0])
    same(as_table(cmp.low), want_sum[3])
    same(as_table(cmp.high), want_sum[4])
    itself = audit.compare(scores_a, scores_a, labels, groups)
    for m in NAMES:
        r = itself.replicates[m]
        assert (r[~np.isnan(r)] == 0).all() and (np.asarray(itself.p_value[m]) == 1.0).all(), m


def test_from_fold_dir(tmp_path):
    scores, labels, groups = so.rare_fold()
    preds = bo.first_argmax(scores)
    preds[:5] = (preds[:5] + 1) % K                                   # the saved predictions are what is scored
    np.save(tmp_path / "probabilities.npy", scores)
    np.save(tmp_path / "labels.npy", labels)
    np.save(tmp_path / "predictions.npy", preds)
    audit = SubgroupAudit(B, seed=SEED)
    got = audit.from_fold_dir(str(tmp_path), groups, group_names=["a", "b", "c"])
    assert_identical(got, audit.evaluate(scores, labels, groups, preds))
    assert got.names == ["a", "b", "c"]
    assert got.overall.point["accuracy"] != audit.evaluate(scores, labels, groups).overall.point["accuracy"]
