"""The subgroup kernels (csrc/subgroup.hip) through mmskin.ops against tests/subgroup_oracle.py: the per-group integers (exact) in
every mode, the ties to the bootstrap kernels (bit for bit), ranges and cuts, and the fp64 tables of finalize and gaps."""
import functools

import numpy as np
import pytest
import torch

import bootstrap_oracle as bo
import subgroup_oracle as so
from mmskin import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 13
TOL = 1e-12
MODES = {"plain": ops.BOOTSTRAP_PLAIN, "stratified": ops.BOOTSTRAP_STRATIFIED, "point": ops.BOOTSTRAP_POINT}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_tables(scores, labels, groups, G, preds=None):
    return ops.subgroup_tables(dev(scores), dev(labels), dev(groups), G, None if preds is None else dev(preds))


def run_replicates(tables, B, mode, seed=SEED, step=None, fill=0):
    conf, counts = ops.subgroup_accumulators(B, tables["G"], tables["K"], DEV, fill=fill)
    step = step or B
    for b0 in range(0, B, step):
        ops.subgroup_replicates(tables, seed, mode, conf, counts, b0, min(b0 + step, B))
    return conf, counts


def oracle_weights(mode, N, B, labels, seed=SEED):
    if mode == "point":
        return np.ones((B, N), dtype=np.int32)
    return bo.weights(seed, N, 0, B, labels if mode == "stratified" else None)


def check_integers(scores, labels, groups, G, B):
    preds = bo.first_argmax(scores)
    tables = device_tables(scores, labels, groups, G)
    N = len(labels)
    for name, mode in MODES.items():
        w = oracle_weights(name, N, B, labels)
        conf, counts = (t.cpu().numpy() for t in run_replicates(tables, B, mode))
        for b in range(1 if name == "point" else B):
            want_conf, want_counts = so.integers(scores, labels, preds, groups, G, w[b])
            assert np.array_equal(conf[b], want_conf), (name, b)
            assert np.array_equal(counts[b], want_counts), (name, b)


@pytest.mark.parametrize("K,G", [(2, 1), (3, 2), (8, 5), (3, 5), (2, 16), (8, 16)])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 130, 1000, 1023])
def test_group_integers_equal_the_restatement(N, K, G):
    scores, labels, groups = so.grouped_fold(N, K, G)
    check_integers(scores, labels, groups, G, 4)


@pytest.mark.parametrize("N,G,K", [(8192, 16, 8), (8192, 4, 64)])
def test_the_corners_of_the_limits(N, G, K):
    assert N == ops.SUBGROUP_MAX_ROWS
    scores, labels, groups = so.grouped_fold(N, K, G)
    check_integers(scores, labels, groups, G, 4)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("N,K", [(65, 3), (1000, 8), (4097, 2)])
def test_one_group_is_the_bootstrap_kernel_bit_for_bit(N, K, mode):
    scores, labels, _ = so.grouped_fold(N, K, 1)
    B = 5
    conf, counts = run_replicates(device_tables(scores, labels, np.zeros(N, dtype=np.int32), 1), B, MODES[mode])
    want_conf, want_counts = ops.bootstrap_accumulators(B, K, DEV)
    ops.bootstrap_replicates(ops.bootstrap_tables(dev(scores), dev(labels)), SEED, MODES[mode], want_conf, want_counts)
    assert torch.equal(conf[:, 0], want_conf) and torch.equal(counts[:, 0], want_counts)


@pytest.mark.parametrize("mode", list(MODES))
def test_groups_partition_the_bootstrap_confusion(mode):
    N, K, G, B = 1000, 3, 5, 6
    scores, labels, groups = so.grouped_fold(N, K, G)
    preds = bo.first_argmax(scores)
    conf, _ = run_replicates(device_tables(scores, labels, groups, G), B, MODES[mode])
    outside = np.where(groups < 0, K, preds)                          # a prediction out of range enters no cell of the bootstrap's
    want, counts = ops.bootstrap_accumulators(B, K, DEV)
    ops.bootstrap_replicates(ops.bootstrap_tables(dev(scores), dev(labels), dev(outside)), SEED, MODES[mode], want, counts)
    assert torch.equal(conf.sum(dim=1, dtype=torch.int32), want)


@pytest.mark.parametrize("mode", ["plain", "stratified"])
@pytest.mark.parametrize("N", [1, 63, 64])
def test_weights_are_those_of_bootstrap_weights_whatever_the_groups(N, mode):
    # one row per group: the group's row count IS the row's weight
    K, B = 2, 6
    scores, labels, _ = so.grouped_fold(N, K, 1)
    tables = device_tables(scores, labels, np.arange(N, dtype=np.int32), N)
    _, counts = run_replicates(tables, B, MODES[mode])
    w = ops.bootstrap_weights(SEED, N, B, DEV, tables=ops.bootstrap_tables(dev(scores), dev(labels)) if mode == "stratified" else None)
    assert torch.equal(counts[:, :, :K].sum(dim=2), w.long())
    # and other groupings see the same resample: their row counts are sums of the same weights
    for G, groups in ((3, np.arange(N) % 3), (2, np.where(np.arange(N) % 5 == 0, -1, np.arange(N) % 2))):
        _, c = run_replicates(device_tables(scores, labels, groups.astype(np.int32), G), B, MODES[mode])
        want = torch.stack([w[:, dev(np.flatnonzero(groups == g))].sum(dim=1) for g in range(G)], dim=1)
        assert torch.equal(c[:, :, :K].sum(dim=2), want.long()), G


def test_a_range_writes_only_its_slices_and_cuts_change_nothing():
    N, K, G, B = 257, 4, 5, 13
    scores, labels, groups = so.grouped_fold(N, K, G)
    tables = device_tables(scores, labels, groups, G)
    whole = run_replicates(tables, B, ops.BOOTSTRAP_PLAIN)
    for step in (1, 7):
        cut = run_replicates(tables, B, ops.BOOTSTRAP_PLAIN, step=step)
        assert torch.equal(whole[0], cut[0]) and torch.equal(whole[1], cut[1]), step
    conf, counts = ops.subgroup_accumulators(B, G, K, DEV, fill=-7)
    ops.subgroup_replicates(tables, SEED, ops.BOOTSTRAP_PLAIN, conf, counts, 3, 10)
    assert torch.equal(conf[3:10], whole[0][3:10]) and torch.equal(counts[3:10], whole[1][3:10])
    for part in (conf[:3], conf[10:], counts[:3], counts[10:]):
        assert bool((part == -7).all())
    again = run_replicates(tables, B, ops.BOOTSTRAP_PLAIN)
    assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1])


@functools.lru_cache(maxsize=None)
def studied(kind, stratified, min_rows, B=32, seed=5):
    scores, labels, groups = so.balanced_fold() if kind == "balanced" else so.rare_fold()
    return (scores, labels, groups) + so.study(scores, labels, None, groups, 3, seed, B, stratified, min_rows)[:4]


def same_table(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))             # position by position
    if (~np.isnan(want)).any():
        assert np.nanmax(np.abs(got - want)) <= TOL


@pytest.mark.parametrize("kind,stratified,min_rows", [("balanced", True, 1), ("balanced", False, 1), ("rare", False, 1), ("rare", False, 4)])
def test_finalize_and_gaps_match_the_restatement(kind, stratified, min_rows):
    B, G, K = 32, 3, 3
    scores, labels, groups, point, table, want_conf, want_counts = studied(kind, stratified, min_rows)
    if kind == "balanced" and stratified:
        assert not np.isnan(table).any()                              # n_valid == B for every column
    if kind == "rare":
        assert np.isnan(table).any()
        if min_rows > 1:
            blank = np.isnan(table[2, 0])
            assert blank.any() and not blank.all()                    # the small group is blank in some replicates, not all
    tables = device_tables(scores, labels, groups, G)
    conf, counts = run_replicates(tables, B, ops.BOOTSTRAP_STRATIFIED if stratified else ops.BOOTSTRAP_PLAIN, seed=5)
    assert np.array_equal(conf.cpu().numpy(), want_conf) and np.array_equal(counts.cpu().numpy(), want_counts)
    metrics, summary = ops.subgroup_finalize(conf, counts, 0.9, min_rows)
    assert tuple(metrics.shape) == (G, 7 + 4 * K, B) and tuple(summary.shape) == (G, 5, 7 + 4 * K)
    same_table(metrics.cpu().numpy(), table)
    for g in range(G):
        want = bo.summary(table[g], 0.9)
        assert np.array_equal(summary[g, 0].cpu().numpy(), want[0]), g
        same_table(summary[g].cpu().numpy(), want)
    if kind == "balanced" and stratified:
        assert bool((summary[:, 0] == B).all())
    pc, pn = run_replicates(tables, 1, ops.BOOTSTRAP_POINT)
    same_table(ops.subgroup_finalize(pc, pn, 0.9, min_rows)[0].cpu().numpy(), point)
    lowest, highest, gap, lowest_group, gsum = (t.cpu().numpy() for t in ops.subgroup_gaps(metrics, 0.9))
    want = so.gaps(table)
    for got, w in zip((lowest, highest, gap), want[:3]):
        same_table(got, w)
    assert np.array_equal(lowest_group, want[3])
    same_table(gsum, so.gap_summary(table, 0.9))
    a, b = metrics[0].contiguous(), metrics[2].contiguous()          # a paired difference of two groups
    delta, dsum, signs = (t.cpu().numpy() for t in ops.subgroup_compare(a, b, 0.9))
    want_delta, want_sum, _ = bo.compare(table[0], table[2], 0.9)
    same_table(delta, want_delta)
    same_table(dsum, want_sum)
    assert np.array_equal(signs[:, 0], (want_delta <= 0).sum(axis=1)) and np.array_equal(signs[:, 1], (want_delta >= 0).sum(axis=1))


def test_wide_tables_compare_in_blocks():
    M, B = 7 + 4 * 64, 9
    rng = np.random.default_rng(3)
    a, b = rng.random((M, B)), rng.random((M, B))
    a[5, 2] = np.nan
    delta, summary, signs = (t.cpu().numpy() for t in ops.subgroup_compare(dev(a), dev(b), 0.9))
    want_delta, want_sum, _ = bo.compare(a, b, 0.9)
    same_table(delta, want_delta)
    same_table(summary, want_sum)
    assert np.array_equal(signs[:, 0], (want_delta <= 0).sum(axis=1))
