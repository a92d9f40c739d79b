"""The curve kernels (csrc/curves.hip) through mmskin.ops against tests/curves_oracle.py: thr, tp, fp, n_points, pos, neg and the NaN
count exactly; the AUC bit-equal to evaluate.per_class_auc of the separate AUC kernel; the indices and thresholds of the
operating points exactly; the other fp64 summaries within 1e-12 relative (both sides are fp64 sums or single ratios of
non-negative terms: a fixed-order tree over N <= 2^12 terms errs by about log2(N) 2^-53, three orders below -- the bound and the
reasoning of tests/test_gpu_calibration_ops.py).  The shapes are the smallest at which the layout changes: N around the wave
(64) and the workgroup (256), one N over several j chunks (1024 rows each), row blocks and compaction blocks; C around 32 and
at the limit."""
import functools

import numpy as np
import pytest
import torch

import curves_oracle as co
from mmskin import evaluate as ev, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
SPEC, SENS = (0.8, 0.9, 0.95), (0.8, 0.9, 0.95)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want) & np.isfinite(want)
    assert np.array_equal(got[~ok & ~np.isnan(want)], want[~ok & ~np.isnan(want)]), what          # infinities: exactly
    err = (np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)).max(initial=0.0)
    exact = np.abs(got[ok] - want[ok]).max(initial=0.0)
    print(f"{what}: max relative difference {err:.3e}")
    assert err <= TOL or exact == 0.0, (what, err)


@functools.lru_cache(maxsize=None)
def case(N, C, kind, dirty=False, nan=False):
    """the fold and the oracle's curves and summary, computed once per shape"""
    probs, labels = co.fold(N, C, kind)
    if dirty and N >= 4:
        labels = labels.copy()
        labels[::7], labels[3::11] = -1, C
    if nan:
        probs = probs.copy()
        valid = np.flatnonzero((labels >= 0) & (labels < C))
        probs[valid[len(valid) // 2], C - 1] = np.nan               # one NaN in a row that counts ...
        labels = labels.copy()
        labels[valid[0]] = -1
        probs[valid[0], 0] = np.nan                                 # ... and one in a dropped row
    want = co.curves(probs, labels)
    return probs, labels, want, co.summary(want, SPEC, SENS)


def check(got, summary, probs, labels, want, s):
    thr, tp, fp, n_points, counts = (t.cpu().numpy() for t in got)
    C = probs.shape[1]
    assert thr.dtype == np.float32 and tp.dtype == np.int32 and fp.dtype == np.int32 and n_points.dtype == np.int32
    assert np.array_equal(n_points, want["n_points"])
    assert np.array_equal(thr, want["thr"]) and np.array_equal(tp, want["tp"]) and np.array_equal(fp, want["fp"])
    assert np.array_equal(counts[:C], want["pos"]) and np.array_equal(counts[C:2 * C], want["neg"]) and counts[2 * C] == want["nan"]
    summary = summary.cpu().numpy()
    A = len(SPEC)
    assert summary.shape == (C, 5 + 3 * (A + len(SENS)))
    counts_auc = ev.ovr_auc_counts(dev(probs), dev(labels))           # the separate AUC kernel: no code shared with the curves
    assert np.array_equal(s["wins2"], counts_auc["wins2"])
    assert np.array_equal(summary[:, 0], ev.per_class_auc(counts_auc), equal_nan=True), "auc is not bit-equal to per_class_auc"
    close(summary[:, 1], s["average_precision"], "average_precision")
    index = lambda col: np.where(np.isnan(col), -1, col).astype(np.int64)
    for name, lo, n in (("youden", 2, 1), ("sens_at_spec", 5, A), ("spec_at_sens", 5 + 3 * A, len(SENS))):
        shape = s[name + "_index"].shape
        assert np.array_equal(index(summary[:, lo + 2:lo + 3 * n:3]).reshape(shape), s[name + "_index"]), name
        assert np.array_equal(summary[:, lo + 1:lo + 3 * n:3].reshape(shape), s[name + "_threshold"], equal_nan=True), name
        close(summary[:, lo:lo + 3 * n:3].reshape(shape), s[name + "_value"], name)


def run(probs, labels):
    got = ops.ovr_curves(dev(probs), dev(labels))
    return got, ops.ovr_curves_summary(got, SPEC, SENS)


ROWS = [1, 2, 63, 64, 65, 255, 256, 257]


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("kind", co.KINDS)
def test_every_row_count_around_the_wave_and_the_workgroup(N, kind):
    for C in (2, 3):
        probs, labels, want, s = case(N, C, kind, dirty=True)
        check(*run(probs, labels), probs, labels, want, s)


@pytest.mark.parametrize("N,C,kind", [(257, 11, "continuous"), (257, 11, "eighths"), (255, 32, "eighths"), (65, 33, "continuous"),
                                      (257, 33, "eighths"), (65, 1024, "eighths"), (65, 1024, "separable")])
def test_class_counts_up_to_the_limit(N, C, kind):
    probs, labels, want, s = case(N, C, kind, dirty=True)
    check(*run(probs, labels), probs, labels, want, s)


@pytest.mark.parametrize("N,C,kind", [(3001, 2, "continuous"), (3001, 3, "eighths"), (3001, 11, "continuous"), (2999, 6, "constant"),
                                      (3001, 6, "separable")])
def test_several_chunks_row_blocks_and_compaction_blocks(N, C, kind):
    probs, labels, want, s = case(N, C, kind, dirty=True)
    check(*run(probs, labels), probs, labels, want, s)


@pytest.mark.parametrize("N,C,kind", [(65, 3, "continuous"), (257, 6, "eighths"), (3001, 3, "eighths")])
def test_a_nan_is_counted_and_is_no_threshold(N, C, kind):
    probs, labels, want, s = case(N, C, kind, dirty=True, nan=True)
    assert want["nan"] == 1
    check(*run(probs, labels), probs, labels, want, s)


@pytest.mark.parametrize("N,C,kind", [(257, 6, "eighths"), (3001, 11, "continuous")])
def test_dirty_buffers_are_overwritten_and_two_calls_give_the_same_bytes(N, C, kind):
    probs, labels, want, s = case(N, C, kind, dirty=True)
    p, y = dev(probs), dev(labels)
    first = ops.ovr_curves(p, y)
    dirty = (torch.full((C, N), float("nan"), device=DEV), torch.full((C, N), -7, dtype=torch.int32, device=DEV),
             torch.full((C, N), -7, dtype=torch.int32, device=DEV), torch.full((C,), -7, dtype=torch.int32, device=DEV),
             torch.full((2 * C + 1,), -7, dtype=torch.int64, device=DEV))
    second = ops.ovr_curves(p, y, out=dirty)
    assert all(a is b for a, b in zip(second, dirty))
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    third = ops.ovr_curves(p, y, out=dirty)                           # a second call on the same buffers
    for a, b in zip(first, third):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    thr, tp, fp, n_points = (t.cpu().numpy() for t in second[:4])
    for c in range(C):
        n = n_points[c]
        assert n < N and not thr[c, n:].any() and not tp[c, n:].any() and not fp[c, n:].any()
    s1, s2 = ops.ovr_curves_summary(first, SPEC, SENS), ops.ovr_curves_summary(third, SPEC, SENS)
    assert torch.equal(s1.view(torch.uint8), s2.view(torch.uint8))


def test_argument_errors():
    p, y = dev(co.fold(8, 3, "continuous")[0]), dev(co.fold(8, 3, "continuous")[1])
    with pytest.raises(ValueError, match="contiguous fp32"):
        ops.ovr_curves(p.double(), y)
    with pytest.raises(ValueError, match="labels"):
        ops.ovr_curves(p, y.int())
    with pytest.raises(ValueError, match="thr"):
        ops.ovr_curves(p, y, out=(torch.empty((3, 7), device=DEV),) + ops.ovr_curves(p, y)[1:])
    got = ops.ovr_curves(p, y)
    with pytest.raises(ops._lib.MMSkinError, match="sensitivities"):
        ops.ovr_curves_summary(got, (), [0.5] * 9)
    assert tuple(ops.ovr_curves_summary(got).shape) == (3, 5)
