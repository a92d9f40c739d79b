"""Calibration without a GPU: tests/calibration_oracle.py (the numpy restatement the kernels are held to by
tests/test_gpu_calibration_ops.py and tests/test_gpu_calibration.py) against tables worked by hand and against sklearn's
brier_score_loss and log_loss, the host path of mmskin.calibration.Calibration against the oracle (exactly), and the argument
errors and limits of the classes and of the C entry points (the refusals need no device)."""
import ctypes

import numpy as np
import pytest
import torch

import calibration_oracle as co
from mmskin import _lib, ops
from mmskin._lib import MMSkinError
from mmskin.calibration import Calibration, TemperatureScaling, host_sums, host_tables, metrics_from_tables

S = co.S
TOL = 1e-12


def fold(N, K, seed=0, eighths=False):
    rng = np.random.default_rng(7 * N + K + seed)
    labels = rng.integers(0, K, N).astype(np.int64)
    raw = rng.random((N, K)) + 0.7 * np.eye(K)[labels]
    probs = raw / raw.sum(axis=1, keepdims=True)
    if eighths:
        probs = np.round(probs * 8) / 8
    return probs.astype(np.float32), labels


def test_worked_example():
    probs, labels = co.EXAMPLE_PROBS, co.EXAMPLE_LABELS
    edges = co.uniform_edges(2, 2)
    assert edges.tolist() == [[0.0, 0.5, 1.0]] * 3
    b, q, hit = co.codes(probs, labels, edges)
    assert b[0].tolist() == [1, 0, 1, 1] and hit[0].tolist() == [1, 0, 0, 1]
    assert q[0].tolist() == [3 * S // 4, S // 2, 3 * S // 4, S]
    tables = co.tables((b, q, hit), 2)
    assert np.array_equal(tables, co.EXAMPLE_TABLES)
    m = co.metrics(tables, co.sums(probs, labels))
    want = [0.25, 0.5, 0.1875, 0.25, 0.4375, -(np.log(0.75) + np.log(0.5) + np.log(0.25)) / 4, 0.125, 0.25]
    assert np.abs(m - np.array(want)).max() <= 1e-15
    assert np.array_equal(host_tables(probs, labels, edges), tables)                          # and the host path
    rep = Calibration(n_bins=2).evaluate(probs, labels)
    assert rep.point["ece"] == 0.25 and rep.point["mce"] == 0.5 and rep.point["per_class_ece"].tolist() == [0.125, 0.25]
    assert rep.reliability["count"].tolist() == [1, 3] and rep.reliability["accuracy"].tolist() == [0.0, 2 / 3]
    assert rep.reliability["confidence"].tolist() == [0.5, 2.5 / 3]


def test_edges_zero_one_and_an_empty_bin():
    # p = 0 -> bin 0; p on an edge -> the lower bin; p = 1 -> the last bin; bins 0 and 1 of the top-label table stay empty
    probs = np.array([[0.0, 1.0], [0.25, 0.75], [0.75, 0.25], [1.0, 0.0], [0.125, 0.875]], dtype=np.float32)
    labels = np.array([1, 1, 0, 1, 0], dtype=np.int64)
    edges = co.uniform_edges(2, 4)
    b, _, _ = co.codes(probs, labels, edges)
    assert b[1].tolist() == [0, 0, 2, 3, 0] and b[2].tolist() == [3, 2, 0, 0, 3] and b[0].tolist() == [3, 2, 2, 3, 3]
    tables = co.tables(co.codes(probs, labels, edges), 4)
    assert tables[0, 0].tolist() == [0, 0, 0] and tables[0, 1].tolist() == [0, 0, 0] and tables[1, 1].tolist() == [0, 0, 0]
    assert np.array_equal(host_tables(probs, labels, edges), tables)
    rep = Calibration(n_bins=4).evaluate(probs, labels)
    assert np.isnan(rep.reliability["accuracy"][:2]).all() and np.isnan(rep.reliability["confidence"][:2]).all()
    assert rep.reliability["count"].tolist() == [0, 0, 2, 3] and np.isfinite(rep.point["mce"])
    m = co.metrics(tables, co.sums(probs, labels))
    assert abs(m[1] - max(abs(2 - 1.5) / 2, abs(1 - 2.875) / 3)) <= 1e-15                    # bin 2: 2 rows, 2 hits; bin 3: 3 rows, 1 hit
    assert m[5] == pytest.approx(-(2 * np.log(0.75) + np.log(0.125) + np.log(co.FLT_MIN)) / 5, rel=1e-15)   # p = 0 at the label: clamped


@pytest.mark.parametrize("binning", ["uniform", "quantile"])
@pytest.mark.parametrize("N,K,n_bins", [(1, 2, 1), (50, 2, 10), (203, 6, 15), (64, 11, 64)])
def test_host_path_equals_the_oracle(N, K, n_bins, binning):
    probs, labels = fold(N, K, eighths=(n_bins == 10))
    edges = co.uniform_edges(K, n_bins) if binning == "uniform" else co.quantile_edges(probs, n_bins)
    assert np.array_equal(ops.calibration_edges(probs, labels, n_bins, binning), edges)
    assert np.array_equal(ops.calibration_edges(torch.from_numpy(probs), None, n_bins, binning).numpy(), edges)
    the_codes = co.codes(probs, labels, edges)
    tables = co.tables(the_codes, n_bins)
    assert np.array_equal(host_tables(probs, labels, edges), tables)
    want = co.metrics(tables, co.sums(probs, labels))
    got = metrics_from_tables(tables, host_sums(probs, labels))
    assert np.abs(got - want).max() <= TOL * np.abs(want).max()
    rep = Calibration(n_bins, binning).evaluate(torch.from_numpy(probs), torch.from_numpy(labels))
    assert np.array_equal(rep.tables, tables) and np.array_equal(rep.edges, edges)
    assert rep.point["ece"] == got[0] and np.array_equal(rep.point["per_class_ece"], got[6:])
    assert rep.low is None and rep.class_reliability["count"].shape == (K, n_bins)
    # the textbook form: each row's q is off by at most 2^-31
    assert abs(want[0] - co.ece_by_means(probs, labels, edges)) <= 2.0 ** -31
    if binning == "quantile" and N >= n_bins and n_bins != 10:                                # tie-free data
        assert (tables[0, :, 0] <= -(-N // n_bins) + 1).all() and (tables[0, :, 0] >= -(-N // n_bins) - 1).all()


def test_weighted_tables_are_the_repeated_rows():
    probs, labels = fold(40, 3)
    w = np.random.default_rng(1).integers(0, 4, 40)
    edges = co.uniform_edges(3, 5)
    rep = np.repeat(np.arange(40), w)
    assert np.array_equal(co.tables(co.codes(probs, labels, edges), 5, w), co.tables(co.codes(probs[rep], labels[rep], edges), 5))
    a, b = co.sums(probs, labels, w), co.sums(probs[rep], labels[rep])
    assert abs(a[0] - b[0]) <= TOL * b[0] and abs(a[1] - b[1]) <= TOL * b[1]


def test_brier_and_nll_match_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    K = 4
    probs, labels = fold(300, K)
    brier, nll = co.sums(probs, labels)
    p64 = probs.astype(np.float64)
    want = sum(metrics.brier_score_loss(labels == c, p64[:, c]) for c in range(K))
    assert abs(brier / 300 - want) <= TOL
    assert abs(nll / 300 - metrics.log_loss(labels, p64 / p64.sum(axis=1, keepdims=True), labels=list(range(K)))) <= 1e-6   # fp32 rows sum to 1 +- 2^-23
    h = host_sums(probs, labels)
    assert abs(h[0] - brier) <= TOL * brier and abs(h[1] - nll) <= TOL * nll


def test_temperature_oracle():
    rng = np.random.default_rng(3)
    z0 = rng.normal(0, 1, (400, 5))
    labels = np.array([rng.choice(5, p=np.exp(r) / np.exp(r).sum()) for r in z0])          # drawn from softmax(z0): beta(3 z0) = 1 / 3
    z = (3 * z0).astype(np.float32)
    beta, at_bound = co.fit_temperature(z, labels)
    assert not at_bound and 0.25 < beta < 0.45
    eps = 1e-6
    a, m, b = co.temperature_stats(z, labels, [beta - eps, beta, beta + eps])
    assert abs(m[1]) <= 1e-9 * m[2] * beta                                                   # the root of the derivative
    assert abs((b[0] - a[0]) / (2 * eps) - m[1]) <= 1e-5 * m[2] and abs((b[1] - a[1]) / (2 * eps) - m[2]) <= 1e-5 * m[2]
    assert co.fit_temperature(np.zeros((5, 3), dtype=np.float32), np.arange(5) % 3) == (1.0, False)
    sure = (10 * np.eye(3)[np.arange(6) % 3]).astype(np.float32)
    assert co.fit_temperature(sure, np.arange(6) % 3) == (64.0, True)
    p = co.softmax(z, 1.0).astype(np.float32)
    assert np.abs(co.temperature_stats(p, labels, [0.5], True) - co.temperature_stats(z, labels, [0.5])).max() <= 1e-4


# ------------------------------------------------------------------------------------------------------- arguments (no device)
def test_constructor_and_argument_errors_need_no_device():
    for bad in (0, ops.CALIBRATION_MAX_BINS + 1):
        with pytest.raises(MMSkinError, match="CALIBRATION_MAX_BINS"):
            Calibration(n_bins=bad)
    with pytest.raises(ValueError, match="binning"):
        Calibration(binning="isotonic")
    with pytest.raises(ValueError, match="replicates_per_call"):
        Calibration(replicates_per_call=0)
    for bad in ((0.0, 1.0), (2.0, 1.0), (1.0, float("inf"))):
        with pytest.raises(ValueError, match="bounds"):
            TemperatureScaling(bounds=bad)
    cal = Calibration(n_bins=5)
    probs, labels = fold(30, 3)
    with pytest.raises(ValueError, match="fp32"):
        cal.evaluate(probs.astype(np.float64), labels)
    with pytest.raises(ValueError, match="fp32"):
        cal.evaluate(probs[:, 0], labels)
    with pytest.raises(ValueError, match="labels"):
        cal.evaluate(probs, labels[:-1])
    with pytest.raises(ValueError, match="labels"):
        cal.evaluate(probs, labels.astype(np.float32))
    with pytest.raises(ValueError, match="one device"):
        cal.evaluate(torch.from_numpy(probs).to("meta"), torch.from_numpy(labels))
    bad = probs.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        cal.evaluate(bad, labels)
    bad[3, 1] = 1.5
    with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
        cal.evaluate(bad, labels)
    with pytest.raises(ValueError, match="confidence"):
        cal.evaluate(probs, labels, n_resamples=8, confidence=1.0)
    with pytest.raises(ValueError, match="infinite"):
        TemperatureScaling().fit(np.full((4, 2), np.inf, dtype=np.float32), np.zeros(4, dtype=np.int64), from_logits=True)
    with pytest.raises(ValueError, match="fit first"):
        TemperatureScaling().apply(probs)
    for shape, word in (((5, 1), "CALIBRATION_MAX_CLASSES"), ((5, 65), "CALIBRATION_MAX_CLASSES")):
        with pytest.raises(MMSkinError, match=word):
            cal.evaluate(np.ones(shape, dtype=np.float32), np.zeros(5, dtype=np.int64))
    with pytest.raises(MMSkinError, match="CALIBRATION_MAX_ROWS"):                      # every row dropped: no row is left
        cal.evaluate(probs, np.full(30, -1, dtype=np.int64))
    for bad in (0, ops.BOOTSTRAP_MAX_RESAMPLES + 1):
        with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_RESAMPLES"):
            cal.evaluate(probs, labels, n_resamples=bad)
    big = np.full((ops.BOOTSTRAP_MAX_ROWS + 1, 2), 0.5, dtype=np.float32)
    with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_ROWS"):
        cal.evaluate(big, np.zeros(len(big), dtype=np.int64), n_resamples=4)
    assert cal.evaluate(big, np.zeros(len(big), dtype=np.int64)).point["ece"] == 0.5    # the plain evaluation holds more rows


def test_check_limits_names_the_limit():
    for kw, word in ((dict(N=0), "MAX_ROWS"), (dict(N=(1 << 24) + 1), "MAX_ROWS"), (dict(K=1), "MAX_CLASSES"), (dict(K=65), "MAX_CLASSES"),
                     (dict(n_bins=0), "MAX_BINS"), (dict(n_bins=65), "MAX_BINS"), (dict(R=0), "MAX_RESAMPLES"), (dict(R=8193), "MAX_RESAMPLES")):
        with pytest.raises(MMSkinError, match=word):
            ops.calibration_check_limits("t", **kw)
    ops.calibration_check_limits("t", N=1 << 24, K=64, n_bins=64, R=8192)
    assert ops.CALIBRATION_METRICS == co.METRICS and ops.CALIBRATION_CLASS_METRICS == ("per_class_ece",)
    assert ops.CALIBRATION_CONF_SCALE_LOG2 == co.S_LOG2


def test_device_only_parts_refuse_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    probs, labels = fold(30, 3)
    with pytest.raises(MMSkinError, match="HIP device"):
        Calibration().evaluate(probs, labels, n_resamples=8)
    with pytest.raises(MMSkinError, match="HIP device"):
        TemperatureScaling().fit(probs, labels)


NAMES = ("mmskin_calibration_metric_columns", "mmskin_calibration_sums_scratch_doubles", "mmskin_temperature_scratch_doubles",
         "mmskin_calibration_codes", "mmskin_calibration_bins", "mmskin_calibration_sums", "mmskin_calibration_finalize",
         "mmskin_temperature_stats", "mmskin_temperature_apply")


def test_symbols_are_declared_bound_and_built():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for name in NAMES:
        assert name in _lib._SIGNATURES and name in declared and hasattr(lib, name), name


def test_c_entry_points_refuse_without_a_device():
    lib = _lib.load()
    one = ctypes.c_void_p(64)                                                         # never dereferenced: the checks come first
    betas = (ctypes.c_double * 2)(1.0, 2.0)

    def refused(rc, word):
        assert rc != 0
        assert word in lib.mmskin_last_error().decode()

    assert lib.mmskin_calibration_metric_columns(6) == 12 and lib.mmskin_calibration_metric_columns(65) == -1
    assert lib.mmskin_calibration_sums_scratch_doubles(4096, 3) == 6 and lib.mmskin_calibration_sums_scratch_doubles(4097, 3) == 12
    assert lib.mmskin_calibration_sums_scratch_doubles(1 << 24, 1) == 512 and lib.mmskin_calibration_sums_scratch_doubles(0, 1) == -1
    assert lib.mmskin_temperature_scratch_doubles(65, 33) == 198 and lib.mmskin_temperature_scratch_doubles(1 << 24, 64) == 3 * 64 * 1024
    assert lib.mmskin_temperature_scratch_doubles(10, 65) == -1
    for N_, K_, n_, R_, word in ((0, 2, 4, 1, "MAX_ROWS"), ((1 << 24) + 1, 2, 4, 1, "MAX_ROWS"), (10, 1, 4, 1, "MAX_CLASSES"),
                                 (10, 65, 4, 1, "MAX_CLASSES"), (10, 2, 0, 1, "MAX_BINS"), (10, 2, 65, 1, "MAX_BINS"),
                                 (10, 2, 4, 0, "MAX_RESAMPLES"), (10, 2, 4, 8193, "MAX_RESAMPLES")):
        if R_ == 1:
            refused(lib.mmskin_calibration_codes(one, one, N_, K_, one, n_, one, one, one, None), word)
        refused(lib.mmskin_calibration_bins(N_, K_, n_, one, one, one, one, R_, one, None), word)
        if word != "MAX_BINS":
            refused(lib.mmskin_calibration_sums(one, one, N_, K_, one, R_, one, one, None), word)
        if word != "MAX_ROWS":
            refused(lib.mmskin_calibration_finalize(one, one, R_, K_, n_, 0.025, 0.975, one, one, None), word)
        if R_ == 1 and word != "MAX_BINS":
            refused(lib.mmskin_temperature_stats(one, 0, one, N_, K_, betas, 2, one, one, None), word)
            refused(lib.mmskin_temperature_apply(one, 0, N_, K_, 1.0, one, None), word)
    refused(lib.mmskin_calibration_finalize(one, one, 8, 3, 15, 0.9, 0.1, one, one, None), "quantiles")
    refused(lib.mmskin_temperature_stats(one, 0, one, 10, 3, betas, 0, one, one, None), "MAX_CANDIDATES")
    refused(lib.mmskin_temperature_stats(one, 0, one, 10, 3, betas, 65, one, one, None), "MAX_CANDIDATES")
    refused(lib.mmskin_temperature_stats(one, 0, one, 10, 3, (ctypes.c_double * 2)(1.0, 0.0), 2, one, one, None), "beta")
    refused(lib.mmskin_temperature_apply(one, 0, 10, 3, float("inf"), one, None), "beta")
    refused(lib.mmskin_temperature_apply(one, 0, 10, 3, float("nan"), one, None), "beta")
    refused(lib.mmskin_calibration_codes(one, one, 10, 3, None, 4, one, one, one, None), "null")
    refused(lib.mmskin_calibration_bins(10, 3, 4, one, one, None, one, 1, one, None), "null")
    refused(lib.mmskin_calibration_sums(one, one, 10, 3, None, 1, None, one, None), "null")
    refused(lib.mmskin_calibration_finalize(one, None, 8, 3, 15, 0.025, 0.975, one, one, None), "null")
    refused(lib.mmskin_temperature_stats(one, 0, None, 10, 3, betas, 2, one, one, None), "null")
    refused(lib.mmskin_temperature_apply(one, 0, 10, 3, 1.0, None, None), "null")
