"""mmskin.conformal on the GPU against tests/conformal_oracle.py: every integer of every replicate and qhat bit for bit, ties, the
infinite threshold, the coverage guarantee, repeatability and independence from the cut, fit / predict_sets, from_fold_dir."""
import os

import numpy as np
import pytest
import torch

import conformal_oracle as co
from gpu_util import DEV
from helpers import SMALL
from mmskin import ConformalPredictor, evaluate as ev
from models import multimodalIntraInterModal as M
from oracle.detinit import det_init_, det_inputs
from oracle.model import OracleMultimodalModel
from conformal_oracle import GUARANTEE, GUARANTEE_CASES, coverage_margin

pytestmark = pytest.mark.gpu
SHAPES = ((37, 2, 1), (256, 6, 7), (1000, 33, 64))                                           # (N, C, R); 33 classes pass one 32-bit word
FOLDS = {}


def fold(N, C, kind):
    if (N, C, kind) not in FOLDS:
        FOLDS[N, C, kind] = co.fold(N, C, kind, seed=N + C)
    return FOLDS[N, C, kind]


def on_device(*arrays):
    return tuple(torch.from_numpy(a).to(DEV) for a in arrays)


def restated(cp, probs, labels, n_cal, R, seed, stratified=False):
    return co.study(probs, labels, cp.score, cp.alpha, n_cal, R, seed, cp.randomized, cp.lam, cp.k_reg, cp.mondrian, stratified)


@pytest.mark.parametrize("stratified", [False, True])
@pytest.mark.parametrize("mondrian", [False, True])
@pytest.mark.parametrize("randomized", [False, True])
@pytest.mark.parametrize("kind", co.KINDS)
def test_every_integer_and_qhat_equal_the_restatement(kind, randomized, mondrian, stratified):
    cp = ConformalPredictor(alpha=0.1, score=kind, randomized=randomized, lam=0.0625, k_reg=2, mondrian=mondrian)
    for N, C, R in SHAPES:
        for values in ("dyadic", "softmax"):                                                 # exact prefix sums, then ordinary rows: rtol = 0
            probs, labels = fold(N, C, values)
            rep = cp.study(*on_device(probs, labels), n_resamples=R, seed=7, stratified=stratified)
            qhat, counts = restated(cp, probs, labels, N // 2, R, 7, stratified)
            assert np.array_equal(rep.counts, counts), (N, C, R, values)
            assert np.array_equal(rep.qhat, qhat), (N, C, R, values)
            assert (rep.replicates["n_test"] == N - N // 2).all()
            want = co.metrics(counts[0], qhat[0])
            got = np.concatenate([[rep.point[m] for m in co.METRICS], rep.point["per_class_coverage"], rep.point["qhat"]])
            assert np.array_equal(got, want, equal_nan=True)


def test_scores_ranks_and_ties_follow_the_stated_rule():
    rows = np.array([[0.25, 0.25, 0.25, 0.25], [0.0, 0.5, 0.0, 0.5], [0.5, 0.0, 0.5, 0.0], [0.125, 0.5, 0.125, 0.25], [0.0, 0.0, 1.0, 0.0]],
                    dtype=np.float32)
    for kind in co.KINDS:
        for randomized in (False, True):
            cp = ConformalPredictor(score=kind, randomized=randomized, lam=0.125, k_reg=1)
            score, rank = cp.scores(torch.from_numpy(rows).to(DEV), seed=5)
            want_score, want_rank = co.scores(rows, kind, randomized, 5, 0.125, 1)
            assert np.array_equal(rank.cpu().numpy(), want_rank) and np.array_equal(score.cpu().numpy(), want_score), (kind, randomized)
    assert np.array_equal(want_rank, [[1, 2, 3, 4], [3, 1, 4, 2], [1, 3, 2, 4], [3, 1, 4, 2], [2, 3, 1, 4]])
    cp = ConformalPredictor(score="aps", randomized=False)
    cp.qhat_, cp.num_classes_, cp.seed_ = 0.5, 4, 0                                          # a threshold that sits on the ties
    mask, size = cp.predict_sets(rows)
    assert np.array_equal(mask.cpu().numpy(), [0b0011, 0b0010, 0b0001, 0b0010, 0b0000]) and np.array_equal(size.cpu().numpy(), [2, 1, 1, 1, 0])
    assert cp.predict_lists(rows, class_names=list("abcd")) == [["a", "b"], ["b"], ["a"], ["b"], []]
    big = fold(1000, 33, "dyadic")[0]                                                        # many exact zeros and ties per row
    score, rank = ConformalPredictor(score="raps", lam=0.01, k_reg=3).scores(torch.from_numpy(big).to(DEV), seed=1, row_offset=17)
    want_score, want_rank = co.scores(big, "raps", True, 1, 0.01, 3, row0=17)
    assert np.array_equal(rank.cpu().numpy(), want_rank) and np.array_equal(score.cpu().numpy(), want_score)


def test_a_calibration_set_too_small_gives_every_class():
    probs, labels = fold(256, 6, "softmax")
    rep = ConformalPredictor(alpha=0.1, score="aps").study(*on_device(probs, labels), n_cal=5, n_resamples=7, seed=1)
    assert np.isinf(rep.qhat).all() and (rep.qhat > 0).all()
    assert (rep.replicates["total_size"] == 6 * 251).all() and (rep.replicates["covered"] == 251).all()
    assert (rep.replicates["set_size_histogram"][:, 6] == 251).all() and rep.point["coverage"] == 1.0 and rep.point["mean_set_size"] == 6.0
    assert rep.summary["mean"]["coverage"] == 1.0 and np.isinf(rep.summary["mean"]["qhat"]).all()
    rare = labels.copy()
    rare[rare == 4] = 3
    rare[200] = 4                                                                            # class 4: one row, and it is a test row
    cp = ConformalPredictor(alpha=0.1, score="lac", mondrian=True)
    rep = cp.study(*on_device(probs, rare), n_cal=128, n_resamples=7, seed=1)
    qhat, counts = restated(cp, probs, rare, 128, 7, 1)
    assert np.array_equal(rep.qhat, qhat) and np.array_equal(rep.counts, counts)
    assert np.isinf(rep.qhat[0, 4]) and np.isfinite(rep.qhat[0, 0])
    assert (rep.replicates["class_in"][:, 4] == 128).all()                                   # always in the set


@pytest.mark.parametrize("kind,randomized", GUARANTEE_CASES)
def test_mean_coverage_keeps_the_guarantee(kind, randomized):
    """The mean coverage over R splits is at least 1 - alpha - margin and, for randomised APS, at most 1 - alpha + 1 / (n_cal + 1) +
    margin.  The margin (conformal_oracle.coverage_margin): the coverage of one split has mean k / (n_cal + 1), k = ceil((n_cal + 1)
    (1 - alpha)), and variance at most that of a Beta(k, n_cal + 1 - k) coverage probability, a b / ((a + b)^2 (a + b + 1)), plus the
    binomial mu (1 - mu) / n_test of its test rows; with distinct scores the R splits of one fold are draws from one distribution, so
    their mean has that variance over R, and the margin is 4 such standard deviations (6e-5 two-sided): 0.0095 at n_cal = n_test =
    500, R = 64.  tests/test_cpu_conformal.py holds the restatement alone to the same bounds with the same seed."""
    g = GUARANTEE
    probs, labels = co.fold(g["N"], g["C"], "softmax", seed=g["seed"])
    cp = ConformalPredictor(alpha=g["alpha"], score=kind, randomized=randomized, lam=0.01, k_reg=1)
    rep = cp.study(*on_device(probs, labels), n_cal=g["n_cal"], n_resamples=g["R"], seed=g["seed"])
    mean = float(np.mean(rep.replicates["covered"] / rep.replicates["n_test"]))
    margin = coverage_margin(g["n_cal"], g["N"] - g["n_cal"], g["R"], g["alpha"])
    print(f"{kind} randomized={randomized}: mean coverage {mean:.5f}, margin {margin:.5f}")
    assert abs(rep.summary["mean"]["coverage"] - mean) <= 1e-12
    assert mean >= 1.0 - g["alpha"] - margin
    if kind == "aps" and randomized:
        assert mean <= 1.0 - g["alpha"] + 1.0 / (g["n_cal"] + 1) + margin


@pytest.mark.parametrize("mondrian,stratified", [(False, False), (True, True)])
def test_repeatable_and_independent_of_the_cut(mondrian, stratified):
    probs, labels = on_device(*fold(1000, 33, "softmax"))
    cp = ConformalPredictor(score="raps", mondrian=mondrian)
    study = lambda R, **kw: cp.study(probs, labels, n_resamples=R, seed=3, stratified=stratified, **kw)
    whole = study(64)
    again = study(64)
    assert np.array_equal(whole.counts, again.counts) and np.array_equal(whole.qhat, again.qhat)
    for name in whole.summary:
        for m in whole.summary[name]:
            assert np.array_equal(whole.summary[name][m], again.summary[name][m], equal_nan=True), (name, m)
    for step in (1, 5, 64):
        cut = study(64, replicates_per_call=step)
        assert np.array_equal(cut.counts, whole.counts) and np.array_equal(cut.qhat, whole.qhat), step
        assert np.array_equal(cut.summary["low"]["coverage"], whole.summary["low"]["coverage"])
    short = study(7)
    assert np.array_equal(short.counts, whole.counts[:7]) and np.array_equal(short.qhat, whole.qhat[:7])


@pytest.mark.parametrize("kind,mondrian", [("lac", False), ("aps", True), ("raps", False)])
def test_fit_and_predict_sets_reproduce_replicate_zero(kind, mondrian):
    N, C = 256, 33
    probs, labels = fold(N, C, "softmax")
    n_cal = N // 2
    cp = ConformalPredictor(alpha=0.3, score=kind, randomized=True, mondrian=mondrian)           # 0.3: finite thresholds with 4 rows a class
    rep = cp.study(*on_device(probs, labels), n_resamples=1, seed=9)
    assert cp.fit(probs[:n_cal], labels[:n_cal], seed=9) is cp and cp.n_cal_ == n_cal
    assert np.array_equal(np.broadcast_to(cp.qhat_, (C,)), rep.qhat[0])
    mask, size = cp.predict_sets(torch.from_numpy(probs[n_cal:]).to(DEV), row_offset=n_cal)
    assert mask.dtype == torch.int64 and size.dtype == torch.int32 and mask.is_cuda
    bits = mask.cpu().numpy().view(np.uint64)
    member = ((bits[:, None] >> np.arange(C, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    assert np.array_equal(size.cpu().numpy(), member.sum(axis=1))                            # size == popcount(mask)
    assert np.array_equal(co.counts(np.concatenate([np.zeros((n_cal, C), dtype=bool), member]), labels, np.arange(N) >= n_cal), rep.counts[0])
    wide, wide_size = cp.predict_sets(torch.from_numpy(probs[n_cal:].astype(np.float64)).to(DEV), row_offset=n_cal)
    assert torch.equal(wide, mask) and torch.equal(wide_size, size)                          # fp32 and fp64 rows of the same values
    assert cp.predict_lists(probs[n_cal:n_cal + 3], row_offset=n_cal) == [list(np.flatnonzero(m)) for m in member[:3]]


def test_temperature_composes():
    probs, labels = fold(256, 6, "softmax")
    from mmskin import ops
    cp = ConformalPredictor(score="aps")
    cooled = ops.temperature_apply(torch.from_numpy(probs).to(DEV), 1.0 / 1.5, from_probs=True)
    a = cp.study(probs, labels, n_resamples=7, seed=2, temperature=1.5)
    b = cp.study(cooled, torch.from_numpy(labels).to(DEV), n_resamples=7, seed=2)
    assert np.array_equal(a.counts, b.counts) and np.array_equal(a.qhat, b.qhat)


def test_from_fold_dir_equals_study_on_the_tensors(tmp_path):
    kw = dict(SMALL, attention_mecanism="crossattention")
    cpu = det_init_(OracleMultimodalModel(**dict(kw, device="cpu")))
    hip = M.MultimodalModel(**dict(kw, device=DEV))
    hip.load_state_dict(cpu.state_dict(), strict=True)
    hip = hip.to(DEV)
    img, meta, lab = det_inputs(13, 32, 20, 6)
    names = [f"lesion_{i}.png" for i in range(13)]
    loader = [(names[a:b], img[a:b], meta[a:b], lab[a:b]) for a, b in ((0, 5), (5, 10), (10, 13))]
    metrics, labels, preds, probs = ev.evaluate_model(hip, loader, None, DEV, 2, str(tmp_path), "custom-cnn", extras=True)
    folder = os.path.join(str(tmp_path), "custom-cnn_fold_2")
    cp = ConformalPredictor(alpha=0.2, score="aps")
    from_dir = cp.from_fold_dir(folder, n_resamples=7, seed=4)
    direct = cp.study(torch.as_tensor(probs).float(), torch.as_tensor(labels), n_resamples=7, seed=4)
    assert np.array_equal(from_dir.counts, direct.counts) and np.array_equal(from_dir.qhat, direct.qhat)
    assert from_dir.options["n_rows"] == 13 and from_dir.options["n_cal"] == 6
    from_dir.save(os.path.join(folder, "conformal.json"))
    assert os.path.getsize(os.path.join(folder, "conformal.json")) > 0
