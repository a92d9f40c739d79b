"""Bootstrap intervals without a GPU: tests/bootstrap_oracle.py (the numpy restatement the kernels are held to by
tests/test_gpu_bootstrap_ops.py and tests/test_gpu_bootstrap.py) against outside knowledge -- sklearn's accuracy_score,
balanced_accuracy_score and roc_auc_score with sample_weight = the resample weights, on every replicate --, the properties of the
weights, and the argument errors of mmskin.bootstrap.BootstrapMetrics and of the C entry points (the refusals need no device)."""
import ctypes

import numpy as np
import pytest
from sklearn.metrics import accuracy_score, balanced_accuracy_score, roc_auc_score

import bootstrap_oracle as bo
from mmskin import _lib, ops
from mmskin._lib import MMSkinError
from mmskin.bootstrap import BootstrapMetrics

N, B, SEED = 204, 32, 3
TOL = 1e-12                                                  # both sides are fp64 over exact integers


def fold(K, seed=0):
    """N rows, at least 20 per class, soft-max-like scores quantised to 1/16 so that ties are common"""
    rng = np.random.default_rng(100 + K + seed)
    labels = np.concatenate([np.repeat(np.arange(K), 20), rng.integers(0, K, N - 20 * K)]).astype(np.int64)
    rng.shuffle(labels)
    raw = rng.random((N, K)) + 0.8 * np.eye(K)[labels]
    scores = (np.round(raw / raw.sum(axis=1, keepdims=True) * 16) / 16).astype(np.float32)
    return scores, labels


@pytest.fixture(scope="module", params=[2, 3, 6])
def studied(request):
    K = request.param
    scores, labels = fold(K)
    out = {}
    for stratified in (False, True):
        out[stratified] = bo.study(scores, labels, None, SEED, B, stratified)
    return K, scores, labels, out


@pytest.mark.parametrize("stratified", [False, True])
def test_restatement_matches_sklearn_on_every_replicate(studied, stratified):
    K, scores, labels, out = studied
    _, table, _, _, w = out[stratified]
    preds = bo.first_argmax(scores)
    onehot = np.eye(K)[labels]
    # sklearn raises on a replicate without a positive and a negative row of every class: all must qualify
    for b in range(B):
        for c in range(K):
            assert w[b][labels == c].sum() > 0 and w[b][labels != c].sum() > 0, (b, c)
    for b in range(B):
        wb = w[b].astype(np.float64)
        got = dict(zip(bo.METRICS, table[:7, b]))
        assert abs(got["accuracy"] - accuracy_score(labels, preds, sample_weight=wb)) <= TOL
        assert abs(got["balanced_accuracy"] - balanced_accuracy_score(labels, preds, sample_weight=wb)) <= TOL
        s64 = scores.astype(np.float64)
        if K == 2:
            assert abs(got["auc"] - roc_auc_score(labels, s64[:, 1], sample_weight=wb)) <= TOL
            macro = 0.5 * (roc_auc_score(labels == 0, s64[:, 0], sample_weight=wb) + roc_auc_score(labels, s64[:, 1], sample_weight=wb))
            assert abs(got["macro_auc"] - macro) <= TOL
        else:
            assert abs(got["auc"] - roc_auc_score(onehot, s64, multi_class="ovr", average="weighted", sample_weight=wb)) <= TOL
            assert abs(got["macro_auc"] - roc_auc_score(onehot, s64, multi_class="ovr", average="macro", sample_weight=wb)) <= TOL
        for c in range(K):
            assert abs(table[7 + K + c, b] - roc_auc_score(labels == c, s64[:, c], sample_weight=wb)) <= TOL
            recall_c = wb[(labels == c) & (preds == c)].sum() / wb[labels == c].sum()
            assert abs(table[7 + c, b] - recall_c) <= TOL


def test_pair_loops_agree_with_the_sorted_restatement():
    scores, labels = fold(3)
    scores, labels = scores[:40], labels[:40]
    preds = bo.first_argmax(scores)
    for b, w in enumerate(bo.weights(SEED, 40, 0, 3)):
        assert np.array_equal(bo.integers(scores, labels, preds, w)[1]["wins2"], bo.integers_by_loops(scores, labels, preds, w)), b


def test_point_estimate_is_the_all_ones_replicate():
    from mmskin.evaluate import _host_counts
    scores, labels = fold(6)
    preds = bo.first_argmax(scores)
    confusion, counts = bo.integers(scores, labels, preds, np.ones(N, dtype=np.int32))
    host = _host_counts(scores, labels)
    for k in ("pos", "neg", "wins2"):
        assert np.array_equal(counts[k], host[k]), k
    plain = np.zeros_like(confusion)
    np.add.at(plain, (labels, preds), 1)
    assert np.array_equal(confusion, plain)


def test_weights_properties():
    scores, labels = fold(6)
    plain, strat = bo.weights(SEED, N, 0, 5), bo.weights(SEED, N, 0, 5, labels)
    assert (plain.sum(axis=1) == N).all() and (strat.sum(axis=1) == N).all()
    for c in range(6):
        assert (strat[:, labels == c].sum(axis=1) == (labels == c).sum()).all(), c
    # a function of (seed, b, N): not of the scores, of B, or of how the study is cut
    assert np.array_equal(bo.weights(SEED, N, 2, 5), plain[2:5])
    assert np.array_equal(bo.weights(SEED, N, 3, 4, labels), strat[3:4])
    other_scores = fold(6, seed=1)[0]
    a = bo.study(scores, labels, None, SEED, 4)[4]
    b = bo.study(other_scores, labels, None, SEED, 7)[4]
    assert np.array_equal(a, b[:4]) and np.array_equal(a, plain[:4])
    assert not np.array_equal(bo.weights(SEED + 1, N, 0, 1), plain[:1])
    assert not np.array_equal(plain[0], plain[1])


def test_draws_are_uniform_enough():
    # 64 replicates of 256 rows: each row expects 64 draws; a generator stuck on a few rows would miss this by far
    w = bo.weights(9, 256, 0, 64).sum(axis=0)
    assert w.sum() == 64 * 256 and w.min() >= 24 and w.max() <= 104   # 64 +- 5 sigma of a binomial(16384, 1/256): sigma = 7.98


def test_summary_and_p_value():
    table = np.array([[0.1, 0.4, np.nan, 0.3, 0.2], [np.nan] * 5, [0.5] * 5])
    s = bo.summary(table, 0.9)
    assert s[0].tolist() == [4.0, 0.0, 5.0]
    assert abs(s[1, 0] - 0.25) <= TOL and abs(s[2, 0] - np.std([0.1, 0.4, 0.3, 0.2], ddof=1)) <= TOL
    assert abs(s[3, 0] - np.percentile([0.1, 0.2, 0.3, 0.4], 5)) <= TOL and abs(s[4, 0] - np.percentile([0.1, 0.2, 0.3, 0.4], 95)) <= TOL
    assert np.isnan(s[1:, 1]).all() and s[2, 2] == 0.0
    delta, _, p = bo.compare(table, table)
    assert (delta[2] == 0).all() and p[2] == 1.0
    d, _, p = bo.compare(np.array([[1.0, 2.0, 3.0, np.nan]]), np.array([[0.0, 0.0, 4.0, 0.0]]))
    assert p[0] == min(1.0, 2 * min((1 + 1) / (3 + 1), (2 + 1) / (3 + 1)))


# ------------------------------------------------------------------------------------------------------- arguments (no device)
def test_constructor_errors():
    for bad in (0, ops.BOOTSTRAP_MAX_RESAMPLES + 1):
        with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_RESAMPLES"):
            BootstrapMetrics(n_resamples=bad)
    for bad in (0.0, 1.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="confidence"):
            BootstrapMetrics(confidence=bad)
    with pytest.raises(ValueError, match="replicates_per_call"):
        BootstrapMetrics(replicates_per_call=0)
    bs = BootstrapMetrics(n_resamples=17, seed=5, confidence=0.9, stratified=True, replicates_per_call=4)
    assert (bs.n_resamples, bs.seed, bs.confidence, bs.stratified, bs.replicates_per_call) == (17, 5, 0.9, True, 4)


def test_argument_errors_need_no_device():
    bs = BootstrapMetrics(n_resamples=8)
    scores, labels = fold(3)
    with pytest.raises(ValueError, match="fp32"):
        bs.evaluate(scores.astype(np.float64), labels)
    with pytest.raises(ValueError, match="fp32"):
        bs.evaluate(scores[:, 0], labels)
    with pytest.raises(ValueError, match="labels"):
        bs.evaluate(scores, labels[:-1])
    with pytest.raises(ValueError, match="labels"):
        bs.evaluate(scores, labels.astype(np.float32))
    with pytest.raises(ValueError, match="preds"):
        bs.evaluate(scores, labels, preds=np.zeros(N - 1, dtype=np.int64))
    with pytest.raises(ValueError, match="prediction"):
        bs.evaluate(scores, labels, preds=np.full(N, 3, dtype=np.int64))
    bad = scores.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        bs.evaluate(bad, labels)
    with pytest.raises(ValueError, match="shape"):
        bs.compare(scores, np.ascontiguousarray(scores[:, :2]), labels)
    with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_CLASSES"):
        bs.evaluate(np.ones((5, 1), dtype=np.float32), np.zeros(5, dtype=np.int64))
    with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_CLASSES"):
        bs.evaluate(np.ones((5, 65), dtype=np.float32), np.zeros(5, dtype=np.int64))
    with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_ROWS"):
        bs.evaluate(np.ones((16385, 2), dtype=np.float32), np.zeros(16385, dtype=np.int64))
    with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_ROWS"):                       # every row dropped: no row is left
        bs.evaluate(scores, np.full(N, -1, dtype=np.int64))


def test_c_entry_points_refuse_without_a_device():
    lib = _lib.load()
    one = ctypes.c_void_p(64)                                                         # never dereferenced: the checks come first

    def refused(rc, word):
        assert rc != 0
        assert word in lib.mmskin_last_error().decode()

    assert lib.mmskin_bootstrap_metric_columns(6) == 19 and lib.mmskin_bootstrap_metric_columns(65) == -1
    for N_, K_, B_, word in ((16385, 2, 4, "MAX_ROWS"), (0, 2, 4, "MAX_ROWS"), (10, 65, 4, "MAX_CLASSES"), (10, 1, 4, "MAX_CLASSES"),
                             (10, 2, 8193, "MAX_RESAMPLES"), (10, 2, 0, "MAX_RESAMPLES")):
        refused(lib.mmskin_bootstrap_weights(0, 0, N_, K_, B_, None, None, None, 0, min(B_, 1), one, None), word)
        refused(lib.mmskin_bootstrap_replicates(0, 0, N_, K_, B_, one, one, None, None, one, one, one, 0, min(B_, 1), one, one, None), word)
    refused(lib.mmskin_bootstrap_finalize(one, one, 8193, 3, 0.025, 0.975, one, one, None), "MAX_RESAMPLES")
    refused(lib.mmskin_bootstrap_finalize(one, one, 8, 65, 0.025, 0.975, one, one, None), "MAX_CLASSES")
    refused(lib.mmskin_bootstrap_finalize(one, one, 8, 3, 0.9, 0.1, one, one, None), "quantiles")
    refused(lib.mmskin_bootstrap_compare(one, one, 0, 13, 0.025, 0.975, one, one, one, None), "MAX_RESAMPLES")
    refused(lib.mmskin_bootstrap_compare(one, one, 8, 0, 0.025, 0.975, one, one, one, None), "columns")
    refused(lib.mmskin_bootstrap_weights(0, 7, 10, 2, 4, None, None, None, 0, 1, one, None), "mode")
    refused(lib.mmskin_bootstrap_weights(0, 0, 10, 2, 4, None, None, None, 2, 5, one, None), "range")
    refused(lib.mmskin_bootstrap_weights(0, 1, 10, 2, 4, None, None, None, 0, 1, one, None), "stratified")
    refused(lib.mmskin_bootstrap_replicates(0, 0, 10, 2, 4, one, one, None, None, one, None, one, 0, 1, one, one, None), "null")
