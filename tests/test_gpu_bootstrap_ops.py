"""The bootstrap kernels (csrc/bootstrap.hip) through mmskin.ops against tests/bootstrap_oracle.py: the weights, the replicate
integers (exact), the point estimate against ovr_auc_counts and the criterion meter, ranges, and finalize against the host
functions and numpy."""
import functools

import numpy as np
import pytest
import torch

import bootstrap_oracle as bo
from mmskin import ops
from mmskin.criterion import EpochMeter
from mmskin.evaluate import ovr_auc_counts

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11
TOL = 1e-12


def fold(N, K, kind, seed=0):
    """scores fp32 [N, K], labels int64 [N]: every class that fits gets a row; kind: continuous, eighths (quantised to 1/8), or
    constant (column 0 all ties)"""
    rng = np.random.default_rng(1000 * N + 10 * K + seed)
    labels = rng.integers(0, K, N)
    labels[:min(N, K)] = np.arange(min(N, K))
    labels = rng.permutation(labels).astype(np.int64)
    raw = rng.random((N, K)) + 0.7 * np.eye(K)[labels]
    scores = raw / raw.sum(axis=1, keepdims=True)
    if kind == "eighths":
        scores = np.round(scores * 8) / 8
    elif kind == "constant":
        scores[:, 0] = 0.25
    return scores.astype(np.float32), labels


@functools.lru_cache(maxsize=None)
def oracle_weights(N, K, B, stratified):
    return bo.weights(SEED, N, 0, B, fold(N, K, "continuous")[1] if stratified else None)


def device_tables(scores, labels, preds=None):
    p = None if preds is None else torch.from_numpy(preds).to(DEV)
    return ops.bootstrap_tables(torch.from_numpy(scores).to(DEV), torch.from_numpy(labels).to(DEV), p)


def run_replicates(tables, B, mode, seed=SEED, step=None, fill=0):
    conf, counts = ops.bootstrap_accumulators(B, tables["K"], DEV, fill=fill)
    step = step or B
    for b0 in range(0, B, step):
        ops.bootstrap_replicates(tables, seed, mode, conf, counts, b0, min(b0 + step, B))
    return conf, counts


@pytest.mark.parametrize("stratified", [False, True])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 1000])
def test_weights_equal_the_restatement(N, stratified):
    K, B = 3, 3
    scores, labels = fold(N, K, "continuous")
    tables = device_tables(scores, labels) if stratified else None
    w = ops.bootstrap_weights(SEED, N, B, DEV, tables=tables)
    assert w.dtype == torch.int32 and tuple(w.shape) == (B, N)
    assert np.array_equal(w.cpu().numpy(), oracle_weights(N, K, B, stratified))
    assert torch.equal(w, ops.bootstrap_weights(SEED, N, B, DEV, tables=tables))
    assert torch.equal(w[1:3], ops.bootstrap_weights(SEED, N, 8, DEV, b0=1, b1=3, tables=tables))    # not a function of B or of the cut
    if N > 2:
        assert not torch.equal(w, ops.bootstrap_weights(SEED + 1, N, B, DEV, tables=tables))


@pytest.mark.parametrize("kind", ["continuous", "eighths", "constant"])
@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("N,K", [(1, 2), (2, 2), (65, 3), (257, 11), (1000, 6)])
def test_replicate_integers_equal_the_restatement(N, K, B, kind):
    scores, labels = fold(N, K, kind)
    preds = bo.first_argmax(scores)
    tables = device_tables(scores, labels)
    assert np.array_equal(tables["preds"].cpu().numpy(), preds)
    for stratified in (False, True):
        w = oracle_weights(N, K, B, stratified)
        conf, counts = run_replicates(tables, B, ops.BOOTSTRAP_STRATIFIED if stratified else ops.BOOTSTRAP_PLAIN)
        conf, counts = conf.cpu().numpy(), counts.cpu().numpy()
        for b in range(B):
            want_conf, want = bo.integers(scores, labels, preds, w[b])
            assert np.array_equal(conf[b], want_conf), (stratified, b)
            assert np.array_equal(counts[b], np.concatenate([want["pos"], want["neg"], want["wins2"]])), (stratified, b)


def test_point_estimate_equals_auc_counts_and_the_meter():
    N, K = 300, 5
    rng = np.random.default_rng(4)
    logits = torch.from_numpy((np.round(rng.normal(0, 2, (N, K)) * 2) / 2).astype(np.float32)).to(DEV)   # ties among the logits
    labels = torch.from_numpy(rng.integers(0, K, N)).to(DEV)
    meter = EpochMeter(K, DEV)
    probs = meter.probs(N)
    meter.update(logits, labels)
    tables = ops.bootstrap_tables(probs, labels, logits.argmax(dim=1))                      # the meter predicts from the logits
    conf, counts = run_replicates(tables, 1, ops.BOOTSTRAP_POINT)
    want = ovr_auc_counts(probs, labels)
    got = counts.cpu().numpy()[0]
    assert want["nan"] == 0
    assert np.array_equal(got, np.concatenate([want["pos"], want["neg"], want["wins2"]]))
    assert np.array_equal(conf.cpu().numpy()[0], meter.compute()["confusion"])


def test_a_range_writes_only_its_slices_and_cuts_change_nothing():
    N, K, B = 257, 4, 13
    scores, labels = fold(N, K, "eighths")
    tables = device_tables(scores, labels)
    whole = run_replicates(tables, B, ops.BOOTSTRAP_PLAIN)
    for step in (1, 7):
        cut = run_replicates(tables, B, ops.BOOTSTRAP_PLAIN, step=step)
        assert torch.equal(whole[0], cut[0]) and torch.equal(whole[1], cut[1]), step
    conf, counts = ops.bootstrap_accumulators(B, K, DEV, fill=-7)
    ops.bootstrap_replicates(tables, SEED, ops.BOOTSTRAP_PLAIN, conf, counts, 3, 10)
    assert torch.equal(conf[3:10], whole[0][3:10]) and torch.equal(counts[3:10], whole[1][3:10])
    for part in (conf[:3], conf[10:], counts[:3], counts[10:]):
        assert bool((part == -7).all())
    again = run_replicates(tables, B, ops.BOOTSTRAP_PLAIN)
    assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1])


@pytest.mark.parametrize("K,B", [(2, 64), (6, 64), (6, 1), (3, 100)])
def test_finalize_matches_the_host_functions_and_numpy(K, B):
    N = 60
    scores, labels = fold(N, K, "eighths")
    labels[labels == K - 1] = 0                                       # a class with 2 rows: some replicates draw none of it
    labels[:2] = K - 1
    tables = device_tables(scores, labels)
    conf, counts = run_replicates(tables, B, ops.BOOTSTRAP_PLAIN)
    metrics, summary = (t.cpu().numpy() for t in ops.bootstrap_finalize(conf, counts, 0.9))
    conf, counts = conf.cpu().numpy(), counts.cpu().numpy()
    want = bo.metric_table([bo.metrics(conf[b], {"pos": counts[b, :K], "neg": counts[b, K:2 * K], "wins2": counts[b, 2 * K:], "nan": 0})
                            for b in range(B)], K)
    assert metrics.shape == want.shape == (7 + 2 * K, B)
    assert np.array_equal(np.isnan(metrics), np.isnan(want))
    assert np.nanmax(np.abs(metrics - want)) <= TOL
    want_summary = bo.summary(metrics, 0.9)
    assert np.array_equal(summary[0], want_summary[0])
    assert np.array_equal(np.isnan(summary), np.isnan(want_summary))
    assert np.nanmax(np.abs(summary - want_summary)) <= TOL
    for m in range(7 + 2 * K):                                        # and against numpy's own mean / std
        v = metrics[m][~np.isnan(metrics[m])]
        if len(v) > 1:
            assert abs(summary[1, m] - v.mean()) <= TOL and abs(summary[2, m] - v.std(ddof=1)) <= TOL
    if B == 1:
        assert np.isnan(summary[2]).all() and np.array_equal(summary[3], summary[4])


def test_compare_kernel():
    K, B, N = 3, 50, 80
    labels = fold(N, K, "continuous")[1]
    ta, tb = device_tables(fold(N, K, "continuous")[0], labels), device_tables(fold(N, K, "eighths", seed=1)[0], labels)
    ma = ops.bootstrap_finalize(*run_replicates(ta, B, ops.BOOTSTRAP_PLAIN))[0]
    mb = ops.bootstrap_finalize(*run_replicates(tb, B, ops.BOOTSTRAP_PLAIN))[0]
    delta, summary, signs = (t.cpu().numpy() for t in ops.bootstrap_compare(ma, mb))
    want_delta, want_summary, _ = bo.compare(ma.cpu().numpy(), mb.cpu().numpy())
    assert np.array_equal(delta, want_delta, equal_nan=True)
    assert np.array_equal(signs[:, 0], (want_delta <= 0).sum(axis=1)) and np.array_equal(signs[:, 1], (want_delta >= 0).sum(axis=1))
    assert np.array_equal(np.isnan(summary), np.isnan(want_summary)) and np.nanmax(np.abs(summary - want_summary)) <= TOL


def test_largest_fold_equals_the_restatement():
    N, K, B = ops.BOOTSTRAP_MAX_ROWS, 2, 2
    scores, labels = fold(N, K, "eighths")
    preds = bo.first_argmax(scores)
    tables = device_tables(scores, labels)
    for stratified in (False, True):
        w = bo.weights(SEED, N, 0, B, labels if stratified else None)
        assert np.array_equal(ops.bootstrap_weights(SEED, N, B, DEV, tables=tables if stratified else None).cpu().numpy(), w)
        conf, counts = run_replicates(tables, B, ops.BOOTSTRAP_STRATIFIED if stratified else ops.BOOTSTRAP_PLAIN)
        for b in range(B):
            want_conf, want = bo.integers(scores, labels, preds, w[b])
            assert np.array_equal(conf[b].cpu().numpy(), want_conf)
            assert np.array_equal(counts[b].cpu().numpy(), np.concatenate([want["pos"], want["neg"], want["wins2"]]))


def test_widest_study_runs_at_the_limits():
    # K = 64 and B = 8192 are the LDS limits of the confusion cells and of the sorted column
    N, K = 130, ops.BOOTSTRAP_MAX_CLASSES
    scores, labels = fold(N, K, "continuous")
    preds = bo.first_argmax(scores)
    tables = device_tables(scores, labels)
    conf, counts = run_replicates(tables, ops.BOOTSTRAP_MAX_RESAMPLES, ops.BOOTSTRAP_PLAIN)
    w = bo.weights(SEED, N, 8190, 8192)
    for k, b in enumerate((8190, 8191)):
        want_conf, want = bo.integers(scores, labels, preds, w[k])
        assert np.array_equal(conf[b].cpu().numpy(), want_conf)
        assert np.array_equal(counts[b].cpu().numpy(), np.concatenate([want["pos"], want["neg"], want["wins2"]]))
    metrics, summary = (t.cpu().numpy() for t in ops.bootstrap_finalize(conf, counts))
    want_summary = bo.summary(metrics[:7])
    assert np.array_equal(np.isnan(summary[:, :7]), np.isnan(want_summary)) and np.nanmax(np.abs(summary[:, :7] - want_summary)) <= TOL
