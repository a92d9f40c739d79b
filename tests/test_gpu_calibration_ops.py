"""The calibration kernels (csrc/calibration.hip) through mmskin.ops against tests/calibration_oracle.py: the codes and the tables
exactly, weighted and unweighted; the single write of a weighted slice; repeatability; the fp64 sums, the finalize output and the
temperature statistics within 1e-12 relative (both sides are fp64 sums of non-negative terms: a fixed-order tree over N <= 2^14
terms errs by about log2(N) 2^-53, three orders below); temperature_apply within 2 fp32 ulp of the fp64 soft-max."""
import functools

import numpy as np
import pytest
import torch

import bootstrap_oracle as bo
import calibration_oracle as co
from mmskin import ops
from calibration_oracle import fold

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11
TOL = 1e-12


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def close(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    err = np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)) if got.size and not np.isnan(want).all() else 0.0
    exact = np.nanmax(np.abs(got - want)) if got.size and not np.isnan(want).all() else 0.0
    print(f"{what}: max relative difference {err:.3e}")
    assert err <= TOL or exact == 0.0, (what, err)


@functools.lru_cache(maxsize=None)
def case(N, K, n_bins, kind, binning="uniform"):
    """the fold, its edges and the oracle's codes, computed once per shape"""
    probs, labels = fold(N, K, kind)
    edges = co.uniform_edges(K, n_bins) if binning == "uniform" else co.quantile_edges(probs, n_bins)
    return probs, labels, edges, co.codes(probs, labels, edges)


def device_codes(probs, labels, edges):
    return ops.calibration_codes(dev(probs), dev(labels), dev(edges))


SHAPES = [(1, 2, 1, "continuous"), (2, 2, 8, "eighths"), (63, 3, 15, "continuous"), (64, 11, 8, "eighths"), (65, 3, 64, "constant"),
          (257, 11, 15, "continuous"), (257, 64, 64, "continuous"), (1000, 6, 15, "continuous"), (1000, 3, 8, "eighths"),
          (1000, 2, 64, "constant")]


@pytest.mark.parametrize("N,K,n_bins,kind", SHAPES)
def test_codes_and_tables_equal_the_oracle(N, K, n_bins, kind):
    probs, labels, edges, want = case(N, K, n_bins, kind)
    assert np.array_equal(ops.calibration_edges(dev(probs), dev(labels), n_bins).cpu().numpy(), edges)
    got = device_codes(probs, labels, edges)
    for g, w, name in zip(got, want, ("bin", "q", "hit")):
        assert np.array_equal(g.cpu().numpy().astype(np.int64), w), name
    tables = ops.calibration_bins(got, n_bins)
    assert tables.dtype == torch.int64 and tuple(tables.shape) == (1, K + 1, n_bins, 3)
    assert np.array_equal(tables.cpu().numpy()[0], co.tables(want, n_bins))
    assert torch.equal(tables, ops.calibration_bins(device_codes(probs, labels, edges), n_bins))     # two runs: the same bits
    ones = torch.ones((1, N), dtype=torch.int32, device=DEV)
    assert torch.equal(tables, ops.calibration_bins(got, n_bins, ones))                               # the weighted form on w = 1


def test_quantile_edges_and_codes_equal_the_oracle():
    for N, K, n_bins, kind in ((257, 3, 15, "continuous"), (1000, 6, 8, "eighths"), (65, 2, 64, "constant"), (2, 2, 8, "continuous")):
        probs, labels, edges, want = case(N, K, n_bins, kind, "quantile")
        assert np.array_equal(ops.calibration_edges(dev(probs), dev(labels), n_bins, "quantile").cpu().numpy(), edges), (N, K)
        got = device_codes(probs, labels, edges)
        assert np.array_equal(got[0].cpu().numpy().astype(np.int64), want[0]), (N, K)
        assert np.array_equal(ops.calibration_bins(got, n_bins).cpu().numpy()[0], co.tables(want, n_bins)), (N, K)


@pytest.mark.parametrize("N,K,n_bins,kind,R", [(1, 2, 1, "continuous", 1), (65, 3, 8, "eighths", 3), (257, 11, 15, "continuous", 64),
                                               (257, 64, 64, "continuous", 3), (1000, 6, 15, "continuous", 3), (1000, 3, 8, "eighths", 64)])
def test_weighted_tables_and_sums_equal_the_oracle(N, K, n_bins, kind, R):
    probs, labels, edges, want = case(N, K, n_bins, kind)
    w = bo.weights(SEED, N, 0, R)
    got = device_codes(probs, labels, edges)
    tables = ops.calibration_bins(got, n_bins, dev(w))
    assert tuple(tables.shape) == (R, K + 1, n_bins, 3)
    host = tables.cpu().numpy()
    for r in sorted({0, R // 2, R - 1}):
        assert np.array_equal(host[r], co.tables(want, n_bins, w[r])), r
    assert (host[:, :, :, 0].sum(axis=2) == N).all()                                                   # every row lands in every table
    assert torch.equal(tables, ops.calibration_bins(got, n_bins, dev(w)))
    sums = ops.calibration_sums(dev(probs), dev(labels), dev(w))
    assert torch.equal(sums, ops.calibration_sums(dev(probs), dev(labels), dev(w)))
    for r in sorted({0, R - 1}):
        close(sums[r].cpu().numpy(), co.sums(probs, labels, w[r]), f"sums N={N} K={K} r={r}")
    close(ops.calibration_sums(dev(probs), dev(labels)).cpu().numpy()[0], co.sums(probs, labels), f"sums N={N} K={K} unweighted")


def test_a_weighted_call_writes_its_slices_once_and_nothing_else():
    N, K, n_bins, B = 257, 4, 15, 13
    probs, labels, edges, _ = case(N, K, n_bins, "eighths")
    got = device_codes(probs, labels, edges)
    w = ops.bootstrap_weights(SEED, N, B, DEV)
    whole = ops.calibration_bins(got, n_bins, w)
    garbage = torch.full((B, K + 1, n_bins, 3), -7, dtype=torch.int64, device=DEV)
    ops.calibration_bins(got, n_bins, w[3:10].contiguous(), garbage, 3)
    assert torch.equal(garbage[3:10], whole[3:10])                                                     # over garbage: written, not added
    assert bool((garbage[:3] == -7).all()) and bool((garbage[10:] == -7).all())
    for step in (1, 7):
        cut = torch.full_like(garbage, 5)
        for b0 in range(0, B, step):
            ops.calibration_bins(got, n_bins, w[b0:b0 + step].contiguous(), cut, b0)
        assert torch.equal(cut, whole), step
    unweighted = torch.full((2, K + 1, n_bins, 3), -7, dtype=torch.int64, device=DEV)
    ops.calibration_bins(got, n_bins, None, unweighted, 1)                                            # zeroes its own slice
    assert torch.equal(unweighted[1:], ops.calibration_bins(got, n_bins)) and bool((unweighted[0] == -7).all())


def test_the_unweighted_form_spreads_rows_over_workgroups():
    N, K, n_bins = 20000, 3, 15                                                                       # three row chunks of 8192
    rng = np.random.default_rng(5)
    probs = rng.dirichlet(np.ones(K), N).astype(np.float32)
    labels = rng.integers(0, K, N).astype(np.int64)
    edges = co.uniform_edges(K, n_bins)
    from mmskin.calibration import host_sums, host_tables                                             # vectorised: the CPU tests hold it to the oracle
    got = device_codes(probs, labels, edges)
    tables = ops.calibration_bins(got, n_bins)
    assert np.array_equal(tables.cpu().numpy()[0], host_tables(probs, labels, edges))
    assert torch.equal(tables, ops.calibration_bins(got, n_bins))
    close(ops.calibration_sums(dev(probs), dev(labels)).cpu().numpy()[0], host_sums(probs, labels), "sums N=20000 (5 chunks)")


@pytest.mark.parametrize("K,n_bins,R", [(2, 8, 64), (6, 15, 64), (6, 15, 1), (11, 64, 100)])
def test_finalize_matches_the_oracle(K, n_bins, R):
    N = 60
    probs, labels, edges, want = case(N, K, n_bins, "eighths")
    w = bo.weights(SEED, N, 0, R)
    w[R // 2] = 0                                                                                      # a replicate without rows: NaN
    tables = ops.calibration_bins(device_codes(probs, labels, edges), n_bins, dev(w))
    sums = ops.calibration_sums(dev(probs), dev(labels), dev(w))
    metrics, summary = (t.cpu().numpy() for t in ops.calibration_finalize(tables, sums, 0.9))
    host_tables, host_sums = tables.cpu().numpy(), sums.cpu().numpy()
    table = np.stack([co.metrics(host_tables[r], host_sums[r]) for r in range(R)], axis=1)
    assert metrics.shape == table.shape == (6 + K, R) and np.isnan(metrics[:, R // 2]).all()
    close(metrics, table, f"metrics K={K}")
    want_summary = bo.summary(metrics, 0.9)
    assert np.array_equal(summary[0], want_summary[0]) and summary[0, 0] == R - 1
    close(summary, want_summary, f"summary K={K}")


@pytest.mark.parametrize("N,K,G", [(1, 2, 33), (65, 3, 1), (65, 3, 33), (65, 3, 64), (257, 11, 33), (1000, 6, 33), (130, 64, 1), (130, 64, 64)])
def test_temperature_stats_equal_the_oracle(N, K, G):
    probs, labels = fold(N, K, "continuous")
    z = (4 * np.random.default_rng(N + K).normal(0, 1, (N, K))).astype(np.float32)
    betas = np.exp(np.linspace(np.log(1 / 64), np.log(64), G)) if G > 1 else np.array([0.7])
    close(ops.temperature_stats(dev(z), dev(labels), betas).cpu().numpy(), co.temperature_stats(z, labels, betas), f"logits N={N} K={K} G={G}")
    got = ops.temperature_stats(dev(probs), dev(labels), betas, from_probs=True)
    close(got.cpu().numpy(), co.temperature_stats(probs, labels, betas, True), f"probs N={N} K={K} G={G}")
    assert torch.equal(got, ops.temperature_stats(dev(probs), dev(labels), betas, from_probs=True))


def test_temperature_stats_over_many_tiles():
    N, K = 70000, 3                                                                                   # 1094 tiles on 1024 workgroups
    rng = np.random.default_rng(2)
    z = rng.normal(0, 2, (N, K)).astype(np.float32)
    labels = rng.integers(0, K, N).astype(np.int64)
    betas = np.array([0.5, 2.0])
    z64 = z.astype(np.float64)
    d = z64 - z64.max(axis=1, keepdims=True)
    want = []
    for beta in betas:
        e = np.exp(beta * d)
        pi = e / e.sum(axis=1, keepdims=True)
        mean = (pi * d).sum(axis=1)
        dy = d[np.arange(N), labels]
        want.append([(np.log(e.sum(axis=1)) - beta * dy).sum(), (mean - dy).sum(), (pi * (d - mean[:, None]) ** 2).sum()])
    got = ops.temperature_stats(dev(z), dev(labels), betas).cpu().numpy()
    err = np.abs(got - np.array(want)) / np.abs(want)
    print("many tiles: max relative difference", err.max())
    assert err.max() <= 1e-11                                # numpy's pairwise sums of 70000 signed terms are the looser side here


@pytest.mark.parametrize("N,K", [(1, 2), (65, 3), (1000, 6), (130, 64)])
def test_temperature_apply_is_the_fp64_softmax(N, K):
    probs, _ = fold(N, K, "continuous")
    z = (4 * np.random.default_rng(N).normal(0, 1, (N, K))).astype(np.float32)
    for src, from_probs, beta in ((z, False, 0.37), (z, False, 3.0), (probs, True, 0.5), (probs, True, 1.0)):
        want = co.softmax(src, beta, from_probs)
        got = ops.temperature_apply(dev(src), beta, from_probs).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (N, K)
        ulp = np.spacing(np.maximum(np.abs(want), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want) <= 2 * ulp).all(), (from_probs, beta)
    assert np.abs(ops.temperature_apply(dev(probs), 1.0, True).cpu().numpy() - probs).max() <= 2 ** -22   # beta = 1 gives the rows back
