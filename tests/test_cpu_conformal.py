"""CPU: the restatement of mmskin.conformal on hand examples, the refusals of the library's entry points (no device: the checks come
before any launch), the workspace query, and the restatement alone against the coverage guarantee with the seeds the GPU test uses."""
import ctypes
import math

import numpy as np
import pytest

import conformal_oracle as co
from conformal_oracle import GUARANTEE, GUARANTEE_CASES, coverage_margin
from mmskin import ConformalPredictor, _lib, conformal
from mmskin._lib import MMSkinError

NAMES = ("mmskin_conformal_count_columns", "mmskin_conformal_metric_columns", "mmskin_conformal_workspace_bytes", "mmskin_conformal_score",
         "mmskin_conformal_apply", "mmskin_conformal_study", "mmskin_conformal_fit", "mmskin_conformal_finalize")


def test_hand_example_scores_ranks_and_the_tie_rule():
    p = np.array([[0.5, 0.25, 0.25], [0.25, 0.25, 0.5], [0.0, 1.0, 0.0]], dtype=np.float32)
    lac, rank = co.scores(p, "lac")
    assert np.array_equal(rank, [[1, 2, 3], [2, 3, 1], [2, 1, 3]])                          # a tie goes to the lower class
    assert np.array_equal(lac, [[0.5, 0.75, 0.75], [0.75, 0.75, 0.5], [1.0, 0.0, 1.0]])
    aps, _ = co.scores(p, "aps")                                                             # u = 1: the mass down to and with the class
    assert np.array_equal(aps, [[0.5, 0.75, 1.0], [0.75, 1.0, 0.5], [1.0, 1.0, 1.0]])
    raps, _ = co.scores(p, "raps", lam=0.125, k_reg=1)
    assert np.array_equal(raps, aps + 0.125 * np.maximum(rank - 1, 0))
    u = co.row_u(3, np.arange(3))
    assert ((u >= 0) & (u < 1)).all() and len(set(u)) == 3
    rand, _ = co.scores(p, "aps", randomized=True, seed=3)
    assert np.array_equal(rand[0], [u[0] * 0.5, 0.5 + u[0] * 0.25, 0.75 + u[0] * 0.25])
    assert np.array_equal(co.sets(aps, np.full(3, 0.75)), [[True, True, False], [True, False, True], [False, False, False]])
    assert np.array_equal(co.mask_of(co.sets(aps, np.full(3, 0.75))), [3, 5, 0])


def test_quantile_index_and_the_infinite_case():
    assert co.quantile_index(9, 0.1) == 9 and co.quantile_index(19, 0.1) == 18 and co.quantile_index(5, 0.1) is None
    assert co.quantile([0.3, 0.1, 0.2, 0.5, 0.4], 0.1) == math.inf and co.quantile([], 0.1) == math.inf
    assert co.quantile(np.arange(19, 0, -1) / 32.0, 0.1) == 18 / 32.0                       # an order statistic, not interpolated


def test_split_has_exactly_n_cal_rows_and_the_stratified_counts():
    labels = np.array([0] * 21 + [1] * 11 + [2] * 5)
    for r in (0, 1, 9):
        cal = co.split(4, r, labels, 3, 18)
        assert cal.sum() == 18 and (r > 0 or cal[:18].all())
        strat = co.split(4, r, labels, 3, 18, stratified=True)
        assert np.array_equal(np.bincount(labels[strat], minlength=3), co.cal_counts(labels, 3, 18))
    assert np.array_equal(co.cal_counts(labels, 3, 18), [10, 5, 3])                          # 10 r 8, 5 r 13, 2 r 16: the one left goes to class 2
    assert np.array_equal(conformal.cal_counts(labels, 3, 18), co.cal_counts(labels, 3, 18))
    assert not np.array_equal(co.split(4, 1, labels, 3, 18), co.split(4, 2, labels, 3, 18))
    assert not np.array_equal(co.split(4, 1, labels, 3, 18), co.split(5, 1, labels, 3, 18))


def test_symbols_are_declared_bound_and_built():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for name in NAMES:
        assert name in _lib._SIGNATURES and name in declared and hasattr(lib, name), name
    assert lib.mmskin_conformal_count_columns(6) == 38 and lib.mmskin_conformal_metric_columns(6) == 18
    assert lib.mmskin_conformal_count_columns(65) == -1 and lib.mmskin_conformal_metric_columns(1) == -1


def refused(rc, word):
    assert rc == 1, rc                                                                        # MMSKIN_ERR_ARG
    message = _lib.load().mmskin_last_error().decode()
    assert word in message, message


def test_c_entry_points_refuse_without_a_device():
    lib = _lib.load()
    one = ctypes.c_void_p(64)                                                                 # never dereferenced: the checks come first
    study = lambda N=100, C=6, R=8, n_cal=50, alpha=0.1, flags=0, r0=0, r1=8: lib.mmskin_conformal_study(
        1, N, C, R, n_cal, alpha, flags, one, one, one, one, one, r0, r1, one, one, one, None)
    score = lambda C=6, kind=1, lam=0.01, k_reg=1, N=10: lib.mmskin_conformal_score(one, 0, N, C, kind, 1, lam, k_reg, 1, 0, one, one, None, None)
    apply = lambda C=6, kind=1, lam=0.01, k_reg=1: lib.mmskin_conformal_apply(one, 0, 10, C, kind, 1, lam, k_reg, 1, 0, one, one, one, None)
    for C in (1, 65):
        refused(study(C=C), "num_classes")
        refused(score(C=C), "num_classes")
        refused(apply(C=C), "num_classes")
        refused(lib.mmskin_conformal_fit(100, C, 0.1, 0, one, one, one, one, one, None), "num_classes")
        refused(lib.mmskin_conformal_finalize(one, one, 100, C, 8, 0.025, 0.975, one, one, None), "num_classes")
    for alpha in (0.0, 1.0, -0.5, 1.5, math.nan):
        refused(study(alpha=alpha), "alpha")
        refused(lib.mmskin_conformal_fit(100, 6, alpha, 0, one, one, one, one, one, None), "alpha")
    for n_cal in (0, 100, -3, 101):
        refused(study(n_cal=n_cal), "n_cal")
    for kind in (-1, 3):
        refused(score(kind=kind), "score")
        refused(apply(kind=kind), "score")
    refused(score(k_reg=-1), "k_reg")
    refused(apply(k_reg=-1), "k_reg")
    refused(score(lam=-0.5), "lam")
    refused(score(lam=math.inf), "lam")
    for N in (0, conformal.MAX_ROWS + 1):
        refused(study(N=N, n_cal=1), "n_rows")
    refused(score(N=0), "n_rows")
    for R in (0, 8193):
        refused(study(R=R), "n_resamples")
    refused(study(flags=4), "flags")
    refused(study(r0=3, r1=2), "range")
    refused(study(r1=9), "range")
    refused(lib.mmskin_conformal_study(1, 100, 6, 8, 50, 0.1, 1, one, one, None, one, one, 0, 8, one, one, one, None), "stratified")
    refused(lib.mmskin_conformal_finalize(one, one, 100, 6, 8, 0.9, 0.1, one, one, None), "quantiles")
    refused(lib.mmskin_conformal_apply(one, 0, 10, 6, 1, 1, 0.01, 1, 1, 0, None, one, one, None), "null")
    assert study(r0=4, r1=4) == 0                                                             # an empty range launches nothing


def test_python_arguments_need_no_device():
    for kw, word in ((dict(alpha=0.0), "alpha"), (dict(alpha=1.0), "alpha"), (dict(score="top-k"), "score"), (dict(k_reg=-1), "k_reg"),
                     (dict(lam=-1.0), "lam")):
        with pytest.raises(ValueError, match=word):
            ConformalPredictor(**kw)
    cp = ConformalPredictor()
    probs, labels = co.fold(30, 3)
    with pytest.raises(ValueError, match="fp32 or fp64"):
        cp.study(probs.astype(np.float16), labels)
    with pytest.raises(ValueError, match="labels"):
        cp.study(probs, labels[:-1])
    for n_cal in (0, 30):
        with pytest.raises(ValueError, match="n_cal"):
            cp.study(probs, labels, n_cal=n_cal)
    with pytest.raises(MMSkinError, match="num_classes"):
        cp.study(np.full((5, 65), 1 / 65, dtype=np.float32), np.zeros(5, dtype=np.int64))
    with pytest.raises(MMSkinError, match="n_rows"):
        cp.study(np.full((conformal.MAX_ROWS + 1, 2), 0.5, dtype=np.float32), np.zeros(conformal.MAX_ROWS + 1, dtype=np.int64))
    with pytest.raises(MMSkinError, match="MAX_RESAMPLES"):
        cp.study(probs, labels, n_resamples=8193)
    with pytest.raises(ValueError, match="confidence"):
        cp.study(probs, labels, confidence=1.0)
    with pytest.raises(ValueError, match="replicates_per_call"):
        cp.study(probs, labels, replicates_per_call=0)
    bad = probs.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        cp.study(bad, labels)
    with pytest.raises(ValueError, match="fit first"):
        cp.predict_sets(probs)


def test_workspace_grows_with_the_rows_and_the_replicates():
    size = _lib.load().mmskin_conformal_workspace_bytes
    assert size(37, 6, 1) < size(256, 6, 1) < size(1000, 6, 1) < size(conformal.MAX_ROWS, 6, 1)
    assert size(256, 6, 1) < size(256, 6, 64) < size(256, 6, 2000) < size(256, 6, 8192)
    assert size(256, 2, 64) < size(256, 33, 64)
    assert size(256, 6, 64) >= 256 * 6 * 8 + 18 * 64 * 8                                     # the scores class-major and the metric columns
    for bad in ((0, 6, 1), (conformal.MAX_ROWS + 1, 6, 1), (10, 1, 1), (10, 65, 1), (10, 6, 0), (10, 6, 8193)):
        assert size(*bad) == -1


def test_metrics_from_counts_agree_with_the_restatement():
    probs, labels = co.fold(256, 6, "softmax", seed=2)
    qhat, counts = co.study(probs, labels, "aps", 0.1, 128, 3, seed=2, randomized=True, mondrian=True)
    for r in range(3):
        assert np.array_equal(conformal.metrics_from_counts(counts[r], qhat[r]), co.metrics(counts[r], qhat[r]), equal_nan=True)
        assert counts[r][0] == 128 and counts[r][6:13].sum() == 128 and counts[r][1] == counts[r][13:20].sum()


@pytest.mark.parametrize("kind,randomized", GUARANTEE_CASES)
def test_the_restatement_keeps_the_guarantee_with_the_shared_seed(kind, randomized):
    g = GUARANTEE
    probs, labels = co.fold(g["N"], g["C"], "softmax", seed=g["seed"])
    _, counts = co.study(probs, labels, kind, g["alpha"], g["n_cal"], g["R"], seed=g["seed"], randomized=randomized, lam=0.01, k_reg=1)
    mean = float(np.mean(counts[:, 1] / counts[:, 0]))
    margin = coverage_margin(g["n_cal"], g["N"] - g["n_cal"], g["R"], g["alpha"])
    print(f"{kind} randomized={randomized}: mean coverage {mean:.5f}, margin {margin:.5f}")
    assert margin < 0.01
    assert mean >= 1.0 - g["alpha"] - margin
    if kind == "aps" and randomized:
        assert mean <= 1.0 - g["alpha"] + 1.0 / (g["n_cal"] + 1) + margin
