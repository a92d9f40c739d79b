"""The subgroup audit without a GPU: tests/subgroup_oracle.py (the numpy restatement the kernels are held to by
tests/test_gpu_subgroup_ops.py and tests/test_gpu_subgroup.py) against hand counts and against bootstrap_oracle.study, the two
folds of the GPU tests checked for what they are built to show, group_ids, and every limit and argument error of
mmskin.subgroup.SubgroupAudit and of the three C entry points (the refusals need no device)."""
import ctypes
import re

import numpy as np
import pytest

import bootstrap_oracle as bo
import subgroup_oracle as so
from mmskin import _lib, ops
from mmskin._lib import MMSkinError
from mmskin.subgroup import SubgroupAudit, group_ids

TOL = 1e-12


# ------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_on_a_six_row_fold_counted_by_hand():
    s1 = np.array([0.75, 0.25, 0.75, 0.5, 0.5, 0.25], dtype=np.float32)
    scores = np.stack([1 - s1, s1], axis=1)
    labels = np.array([1, 0, 0, 1, 0, 1])
    preds = np.array([1, 0, 1, 1, 0, 0])
    groups = np.array([0, 0, 0, 1, 1, -1])
    w = np.array([2, 1, 0, 1, 3, 1])
    conf, counts = so.integers(scores, labels, preds, groups, 2, w)
    # group 0 = rows 0, 1, 2 (w 2, 1, 0): the positive of class 1 (w 2, 0.75) beats the negative (w 1, 0.25): 2 * 2 * 1; the
    # weightless row 2 adds nothing.  group 1 = rows 3, 4 (w 1, 3): one tie in each class: 1 * 3.  row 5 is in no group.
    assert conf.tolist() == [[[1, 0], [0, 2]], [[3, 0], [0, 1]]]
    assert counts.tolist() == [[1, 2, 2, 1, 4, 4], [3, 1, 1, 3, 3, 3]]
    m = so.metrics(conf[0], counts[0])
    assert m[0] == 1.0 and m[5] == 1.0 and m[7 + 2 + 1] == 1.0                                 # accuracy, auc, auc of class 1
    assert m[7 + 4:].tolist() == [0.0, 0.0, 1 / 3, 2 / 3]                                      # fpr [2], predicted rate [2]
    assert so.metrics(conf[1], counts[1])[5] == 0.5
    assert np.isnan(so.metrics(conf[0], counts[0], min_rows=4)).all() and not np.isnan(so.metrics(conf[1], counts[1], min_rows=4)).any()
    conf3, counts3 = so.integers(scores, labels, preds, groups, 3, w)                          # an empty group: zeros, all NaN
    assert not conf3[2].any() and not counts3[2].any() and np.isnan(so.metrics(conf3[2], counts3[2])).all()
    one_class = so.metrics(np.array([[3, 1], [0, 0]], dtype=np.int32), np.array([4, 0, 0, 4, 0, 0]))
    assert np.isnan(one_class[5]) and np.isnan(one_class[7 + 4]) and one_class[7 + 5] == 0.25  # no negative of class 0: fpr undefined


@pytest.mark.parametrize("stratified", [False, True])
def test_one_group_is_the_bootstrap(stratified):
    scores, labels, _ = so.grouped_fold(65, 3, 1)
    point, table, conf, counts, w = so.study(scores, labels, None, np.zeros(65, dtype=np.int32), 1, 3, 6, stratified)
    want = bo.study(scores, labels, None, 3, 6, stratified)
    K = 3
    assert np.array_equal(point[0, :7 + 2 * K], want[0], equal_nan=True) and np.array_equal(table[0, :7 + 2 * K], want[1], equal_nan=True)
    assert np.array_equal(conf[:, 0], want[2]) and np.array_equal(counts[:, 0], want[3]) and np.array_equal(w, want[4])


def test_groups_partition_the_confusion_and_share_the_weights():
    scores, labels, groups = so.grouped_fold(130, 3, 5)
    preds = bo.first_argmax(scores)
    _, _, conf, counts, w = so.study(scores, labels, preds, groups, 5, 2, 3)
    assert np.array_equal(w, bo.weights(2, 130, 0, 3))                                          # drawn on the whole fold
    for b in range(3):
        inside = groups >= 0
        assert np.array_equal(conf[b].sum(axis=0), bo.integers(scores[inside], labels[inside], preds[inside], w[b][inside])[0])
    assert not conf[:, 1].any() and (counts[:, 4, 1:3] == 0).all()                              # group 1 is empty, group 4 holds class 0 only


def test_gaps_and_lowest_group():
    nan = np.nan
    table = np.array([[[0.5, 0.2, nan, nan]], [[0.5, 0.7, 0.1, nan]], [[0.9, nan, nan, nan]]])   # [G = 3, M = 1, B = 4]
    lowest, highest, gap, lowest_group = so.gaps(table)
    assert np.array_equal(lowest, [[0.5, 0.2, 0.1, nan]], equal_nan=True) and np.array_equal(highest, [[0.9, 0.7, 0.1, nan]], equal_nan=True)
    assert np.array_equal(gap, [[0.9 - 0.5, 0.7 - 0.2, nan, nan]], equal_nan=True)               # one group defined: no gap
    assert lowest_group.tolist() == [[2, 1, 0]]                                                 # the tie of replicate 0 goes to group 0
    assert so.gap_summary(table).shape == (3, 5, 1)


def test_the_folds_of_the_gpu_tests_show_what_they_are_built_for():
    scores, labels, groups = so.balanced_fold()
    for g in range(3):
        assert (np.bincount(labels[groups == g], minlength=3) >= 2).all()
    table = so.study(scores, labels, None, groups, 3, 5, 32, stratified=True)[1]
    assert not np.isnan(table).any()                                                            # n_valid == B in every column
    scores, labels, groups = so.rare_fold()
    assert np.bincount(labels[groups == 1], minlength=3)[2] == 0 and (groups == 2).sum() == 4
    table = so.study(scores, labels, None, groups, 3, 5, 32)[1]
    assert np.isnan(table[1, 7 + 2]).all() and not np.isnan(table[0, 0]).any()                  # group 1 never has a recall of class 2
    small = np.isnan(so.study(scores, labels, None, groups, 3, 5, 32, min_rows=4)[1][2, 0])
    assert small.any() and not small.all()                                                      # min_rows blanks group 2 in some replicates


# ------------------------------------------------------------------------------------------------------- group_ids
def test_group_ids():
    ids, names = group_ids(["FEMALE", "MALE", "", None, "FEMALE", float("nan"), "  "])
    assert ids.dtype == np.int32 and ids.tolist() == [0, 1, -1, -1, 0, -1, -1] and names == ["FEMALE", "MALE"]
    ids, names = group_ids(np.array([3.0, 1.0, np.nan, 6.0, 1.0]))
    assert ids.tolist() == [1, 0, -1, 2, 0] and names == ["1.0", "3.0", "6.0"]
    ids, names = group_ids(np.array([10, 40, 69.5, np.nan, 70, 93]), bins=[40, 70])
    assert ids.tolist() == [0, 1, 1, -1, 2, 2] and names == ["< 40", "[40, 70)", ">= 70"]
    assert group_ids([5, None, 7], bins=[6])[0].tolist() == [0, -1, 1]
    ids, names = group_ids([])
    assert ids.shape == (0,) and names == []
    for bad in ([], [3, 1], [1, 1], [[1, 2]]):
        with pytest.raises(ValueError, match="bins"):
            group_ids([1.0], bins=bad)


# ------------------------------------------------------------------------------------------------------- arguments (no device)
def test_constructor_errors():
    for bad in (0, ops.BOOTSTRAP_MAX_RESAMPLES + 1):
        with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_RESAMPLES"):
            SubgroupAudit(n_resamples=bad)
    for bad in (0.0, 1.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="confidence"):
            SubgroupAudit(confidence=bad)
    with pytest.raises(ValueError, match="replicates_per_call"):
        SubgroupAudit(replicates_per_call=0)
    with pytest.raises(ValueError, match="min_rows"):
        SubgroupAudit(min_rows=0)
    a = SubgroupAudit(n_resamples=17, seed=5, confidence=0.9, stratified=True, min_rows=3, replicates_per_call=4)
    assert (a.n_resamples, a.seed, a.confidence, a.stratified, a.min_rows, a.replicates_per_call) == (17, 5, 0.9, True, 3, 4)


def test_argument_errors_need_no_device():
    audit = SubgroupAudit(n_resamples=8)
    scores, labels, groups = so.grouped_fold(65, 3, 5)
    N = 65
    with pytest.raises(ValueError, match="fp32"):
        audit.evaluate(scores.astype(np.float64), labels, groups)
    with pytest.raises(ValueError, match="fp32"):
        audit.evaluate(scores[:, 0], labels, groups)
    with pytest.raises(ValueError, match="labels"):
        audit.evaluate(scores, labels[:-1], groups)
    with pytest.raises(ValueError, match="groups"):
        audit.evaluate(scores, labels, groups[:-1])
    with pytest.raises(ValueError, match="groups"):
        audit.evaluate(scores, labels, groups.astype(np.float32))
    with pytest.raises(ValueError, match="preds"):
        audit.evaluate(scores, labels, groups, preds=np.zeros(N - 1, dtype=np.int64))
    with pytest.raises(ValueError, match="prediction"):
        audit.evaluate(scores, labels, groups, preds=np.full(N, 3, dtype=np.int64))
    with pytest.raises(ValueError, match="group_names"):
        audit.evaluate(scores, labels, groups, group_names=["a", "b"])                          # ids reach 4
    with pytest.raises(ValueError, match="group_names"):
        audit.evaluate(scores, labels, groups, group_names=["a", "a", "b", "c", "d"])
    bad = scores.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        audit.evaluate(bad, labels, groups)
    with pytest.raises(ValueError, match="shape"):
        audit.compare(scores, np.ascontiguousarray(scores[:, :2]), labels, groups)
    for K in (1, 65):
        with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_CLASSES"):
            audit.evaluate(np.ones((5, K), dtype=np.float32), np.zeros(5, dtype=np.int64), np.zeros(5, dtype=np.int32))
    rows = ops.SUBGROUP_MAX_ROWS + 1
    with pytest.raises(MMSkinError, match="SUBGROUP_MAX_ROWS"):
        audit.evaluate(np.ones((rows, 2), dtype=np.float32), np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int32))
    with pytest.raises(MMSkinError, match="SUBGROUP_MAX_ROWS"):                                 # every row dropped: no row is left
        audit.evaluate(scores, np.full(N, -1, dtype=np.int64), groups)
    with pytest.raises(MMSkinError, match="SUBGROUP_MAX_GROUPS"):
        audit.evaluate(scores, labels, np.full(N, ops.SUBGROUP_MAX_GROUPS, dtype=np.int32))
    wide = np.full((8, 64), 1 / 64, dtype=np.float32)
    with pytest.raises(MMSkinError, match="SUBGROUP_MAX_CELLS"):
        audit.evaluate(wide, np.zeros(8, dtype=np.int64), np.array([0, 1, 2, 3, 4, 0, 1, 2], dtype=np.int32))    # 5 * 64 * 64 cells
    with pytest.raises(MMSkinError, match="SUBGROUP_MAX_CELLS"):
        ops.subgroup_check_limits("x", K=64, G=5)
    ops.subgroup_check_limits("x", N=8192, K=64, G=4, B=8192)
    ops.subgroup_check_limits("x", N=8192, K=8, G=16)
    ops.subgroup_check_limits("x", K=16, G=64)


def test_python_limits_are_the_header_macros():
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    for name in ("MAX_ROWS", "MAX_GROUPS", "MAX_CELLS"):
        assert int(re.search(rf"#define MMSKIN_SUBGROUP_{name} (\d+)", text).group(1)) == getattr(ops, f"SUBGROUP_{name}"), name


def test_c_entry_points_refuse_without_a_device():
    lib = _lib.load()
    one = ctypes.c_void_p(64)                                                         # never dereferenced: the checks come first
    for name in ("mmskin_subgroup_metric_columns", "mmskin_subgroup_replicates", "mmskin_subgroup_finalize", "mmskin_subgroup_gaps"):
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols() and hasattr(lib, name), name

    def refused(rc, word, code):
        assert rc == code, (rc, word)
        assert word in lib.mmskin_last_error().decode(), (word, lib.mmskin_last_error().decode())

    assert lib.mmskin_subgroup_metric_columns(6) == 31 and lib.mmskin_subgroup_metric_columns(65) == -1
    assert lib.mmskin_subgroup_metric_columns(1) == -1

    def replicates(N=10, K=2, G=2, B=4, mode=0, b0=0, b1=1, labels=one, members=None, group_start=one):
        return lib.mmskin_subgroup_replicates(0, mode, N, K, G, B, labels, one, one, members, members, one, one, one, group_start, b0, b1,
                                              one, one, None)

    for kw, word in ((dict(N=8193), "MMSKIN_SUBGROUP_MAX_ROWS"), (dict(N=0), "MMSKIN_SUBGROUP_MAX_ROWS"),
                     (dict(K=65), "MMSKIN_BOOTSTRAP_MAX_CLASSES"), (dict(K=1), "MMSKIN_BOOTSTRAP_MAX_CLASSES"),
                     (dict(G=65), "MMSKIN_SUBGROUP_MAX_GROUPS"), (dict(G=0), "MMSKIN_SUBGROUP_MAX_GROUPS"),
                     (dict(G=5, K=64), "MMSKIN_SUBGROUP_MAX_CELLS"), (dict(G=17, K=32), "MMSKIN_SUBGROUP_MAX_CELLS"),
                     (dict(B=8193), "MMSKIN_BOOTSTRAP_MAX_RESAMPLES"), (dict(B=0, b1=0), "MMSKIN_BOOTSTRAP_MAX_RESAMPLES")):
        rc = replicates(**kw)
        assert rc != 0 and rc == lib.mmskin_bootstrap_finalize(one, one, 8193, 3, 0.025, 0.975, one, one, None), kw   # UNSUPPORTED
        replicates(**kw)
        assert word in lib.mmskin_last_error().decode(), (kw, lib.mmskin_last_error().decode())
    unsupported = lib.mmskin_bootstrap_finalize(one, one, 8193, 3, 0.025, 0.975, one, one, None)
    arg = lib.mmskin_bootstrap_finalize(one, one, 8, 3, 0.9, 0.1, one, one, None)
    assert arg != 0 and arg != unsupported
    refused(replicates(mode=7), "mode", arg)
    refused(replicates(b0=2, b1=5), "range", arg)
    refused(replicates(b0=3, b1=2), "range", arg)
    refused(replicates(mode=1), "stratified", arg)
    refused(replicates(labels=None), "null", arg)
    refused(replicates(group_start=None), "null", arg)
    assert replicates(b0=2, b1=2, N=8192, K=64, G=4) == 0 and replicates(b0=1, b1=1, N=8192, K=8, G=16) == 0    # an empty range of a study at the corners

    def finalize(B=8, G=2, K=3, min_rows=1, q=(0.025, 0.975), metrics=one):
        return lib.mmskin_subgroup_finalize(one, one, B, G, K, min_rows, q[0], q[1], metrics, one, None)

    refused(finalize(B=8193), "MMSKIN_BOOTSTRAP_MAX_RESAMPLES", unsupported)
    refused(finalize(B=0), "MMSKIN_BOOTSTRAP_MAX_RESAMPLES", unsupported)
    refused(finalize(K=65), "MMSKIN_BOOTSTRAP_MAX_CLASSES", unsupported)
    refused(finalize(G=65), "MMSKIN_SUBGROUP_MAX_GROUPS", unsupported)
    refused(finalize(G=0), "MMSKIN_SUBGROUP_MAX_GROUPS", unsupported)
    refused(finalize(G=5, K=64), "MMSKIN_SUBGROUP_MAX_CELLS", unsupported)
    refused(finalize(q=(0.9, 0.1)), "quantiles", arg)
    refused(finalize(min_rows=0), "min_rows", arg)
    refused(finalize(metrics=None), "null", arg)

    def gaps(B=8, G=2, M=19, q=(0.025, 0.975), lowest=one):
        return lib.mmskin_subgroup_gaps(one, B, G, M, q[0], q[1], lowest, one, one, one, one, None)

    refused(gaps(B=8193), "MMSKIN_BOOTSTRAP_MAX_RESAMPLES", unsupported)
    refused(gaps(B=0), "MMSKIN_BOOTSTRAP_MAX_RESAMPLES", unsupported)
    refused(gaps(G=65), "MMSKIN_SUBGROUP_MAX_GROUPS", unsupported)
    refused(gaps(G=0), "MMSKIN_SUBGROUP_MAX_GROUPS", unsupported)
    refused(gaps(M=0), "columns", arg)
    refused(gaps(M=7 + 4 * 64 + 1), "columns", arg)
    refused(gaps(q=(0.5, 0.4)), "quantiles", arg)
    refused(gaps(lowest=None), "null", arg)
