"""numpy fp64 restatement of csrc/uncertainty.hip (contract: include/mmskin.h): the dihedral views, the reduction of T passes to
per-row statistics, the risk-coverage counts and their summary, and the generators of the cases the GPU tests run.
tests/test_cpu_uncertainty.py holds it to closed forms; the kernels are held to it by tests/test_gpu_uncertainty_ops.py and
tests/test_gpu_uncertainty.py."""
import numpy as np

STATS = ("confidence", "margin", "predictive_entropy", "expected_entropy", "mutual_information", "variation_ratio", "predicted_std")
SUMMARY = ("aurc", "optimal_aurc", "e_aurc", "error_auroc", "error_rate", "n", "n_wrong", "n_distinct")
# |got - want| <= TOL max(|want|, 1): the figure tests/test_gpu_calibration_ops.py holds its fp64 device sums to.  The absolute floor
# is there because an entropy next to 0 is a difference of near-equal numbers, bounded by ln 64.
TOL = 1e-12


def close(got, want):
    """the tolerance above, element by element; a NaN must meet a NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and (np.abs(got - want)[~nan] <= TOL * np.maximum(np.abs(want[~nan]), 1.0)).all())


def worst(got, want):
    """max |got - want| / max(|want|, 1) over the entries that are no NaN (for the printed figures)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ok = ~np.isnan(want)
    return float((np.abs(got - want)[ok] / np.maximum(np.abs(want[ok]), 1.0)).max()) if ok.any() else 0.0


# --------------------------------------------------------------------------------------------------------------- views
def view_ids(mask):
    return [v for v in range(8) if (mask >> v) & 1]


def view(x, v):
    """view v of x [..., H, W]: a rotation by (v & 3) quarter turns, then a flip along W when v & 4"""
    y = np.rot90(x, k=v & 3, axes=(-2, -1))
    return np.ascontiguousarray(np.flip(y, axis=-1) if v & 4 else y)


def views(x, mask):
    return np.stack([view(x, v) for v in view_ids(mask)])


# --------------------------------------------------------------------------------------------------------------- reduce
def _entropy(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(p > 0.0, p * np.log(p), 0.0).sum(axis=-1)


def reduce(logits):
    """logits fp32 [T, N, C] -> dict(mean_prob [N, C], prob_std [N, C], votes int32 [N, C], pred int32 [N], stats [N, 7]); the
    passes are walked in order, twice, as the kernel walks them"""
    T, N, C = logits.shape
    x = logits.astype(np.float64)
    bad = ~np.isfinite(logits).all(axis=(0, 2))
    with np.errstate(invalid="ignore", over="ignore"):
        probs = []
        sum_p, sum_h = np.zeros((N, C)), np.zeros(N)
        votes = np.zeros((N, C), dtype=np.int32)
        for t in range(T):
            e = np.exp(x[t] - x[t].max(axis=1, keepdims=True))
            p = e / e.sum(axis=1, keepdims=True)
            probs.append(p)
            sum_p += p
            sum_h += _entropy(p)
            votes[np.arange(N), np.argmax(logits[t], axis=1)] += 1           # np.argmax: the first index among equals
        mean = sum_p / T
        sum_d2 = np.zeros((N, C))
        for t in range(T):
            d = probs[t] - mean
            sum_d2 += d * d
        sd = np.sqrt(sum_d2 / T)
    pred = np.argmax(np.where(bad[:, None], 0.0, mean), axis=1).astype(np.int32)
    rows = np.arange(N)
    conf = mean[rows, pred]
    rest = mean.copy()
    rest[rows, pred] = -1.0
    h_mean, h_exp = _entropy(np.where(bad[:, None], 1.0, mean)), sum_h / T
    stats = np.stack([conf, conf - rest.max(axis=1), h_mean, h_exp, np.maximum(h_mean - h_exp, 0.0), 1.0 - votes.max(axis=1) / float(T),
                      sd[rows, pred]], axis=1)
    mean, sd, stats = mean.copy(), sd.copy(), stats.copy()
    mean[bad], sd[bad], stats[bad], votes[bad], pred[bad] = np.nan, np.nan, np.nan, 0, -1
    return dict(mean_prob=mean, prob_std=sd, votes=votes, pred=pred, stats=stats)


REDUCE_SHAPES = [(1, 1, 2), (2, 3, 6), (5, 65, 7), (33, 64, 6), (7, 257, 64), (64, 5, 33)]


def reduce_case(T, N, C, seed=0):
    """Drawn logits with, where the rows allow, planted: row 0 at +-80 and row 1 at 1e4 scale (probabilities that underflow to 0),
    row 2 all equal, row 3 with two exactly equal maxima in every pass (the first index must win pred and every vote), row 4
    with a +inf in one pass (NaN statistics, pred -1); fewer rows keep the first of these."""
    rng = np.random.default_rng(1000 * T + 10 * N + C + seed)
    z = (rng.normal(0.0, 2.0, (T, N, C)) + 3.0 * rng.normal(0.0, 1.0, (1, N, C))).astype(np.float32)
    z[:, 0] = np.where(rng.random((T, C)) < 0.5, 80.0, -80.0).astype(np.float32)
    if N > 1:
        z[:, 1] = (1e4 * rng.integers(-1, 2, (T, C))).astype(np.float32)
    if N > 2:
        z[:, 2] = np.float32(0.375)
    if N > 3:
        hi = z[:, 3].max() + np.float32(1.0)
        z[:, 3, C - 1], z[:, 3, C // 2] = hi, hi
    if N > 4:
        z[T // 2, 4, C // 3] = np.inf
    return z


# --------------------------------------------------------------------------------------------------------------- risk-coverage
def risk_counts(score, wrong):
    """int32 [N, 4] = n_lt, n_eq, e_lt, e_eq per row, by a stable sort"""
    score, w = np.asarray(score, dtype=np.float64), np.asarray(wrong) != 0
    order = np.argsort(score, kind="stable")
    s, ws = score[order], w[order]
    cum_w = np.concatenate([[0], np.cumsum(ws)])
    lo, hi = np.searchsorted(s, score, side="left"), np.searchsorted(s, score, side="right")
    return np.stack([lo, hi - lo, cum_w[lo], cum_w[hi] - cum_w[lo]], axis=1).astype(np.int32)


def risk_summary(counts, wrong):
    """fp64 [8] = SUMMARY from the counts: tie groups by the expectation over the order of the ties"""
    counts, w = np.asarray(counts, dtype=np.int64), np.asarray(wrong) != 0
    N, E = len(w), int(w.sum())
    groups = {int(c[0]): c for c in counts}                                   # a tie group is known by the rank it starts at
    aurc = 0.0
    for n_lt in sorted(groups):
        _, n_eq, e_lt, e_eq = (int(v) for v in groups[n_lt])
        k = np.arange(n_lt + 1, n_lt + n_eq + 1, dtype=np.float64)
        aurc += float(((e_lt + (k - n_lt) * e_eq / n_eq) / k).sum())
    aurc /= N
    k = np.arange(N - E + 1, N + 1, dtype=np.float64)
    best = float(((k - (N - E)) / k).sum()) / N
    wins2 = int((2 * (counts[w, 0] - counts[w, 2]) + (counts[w, 1] - counts[w, 3])).sum())
    auroc = wins2 / (2.0 * E * (N - E)) if 0 < E < N else np.nan
    return np.array([aurc, best, aurc - best, auroc, E / N, N, E, len(groups)], dtype=np.float64)


def risk_curve(counts):
    """(coverage, risk) at the distinct scores, ascending"""
    counts = np.asarray(counts, dtype=np.int64)
    _, first = np.unique(counts[:, 0], return_index=True)
    c = counts[first]
    kept = c[:, 0] + c[:, 1]
    return kept / float(len(counts)), (c[:, 2] + c[:, 3]) / kept.astype(np.float64)


RISK_SIZES = [1, 2, 63, 64, 65, 257, 1025]
RISK_SCORES = ("distinct", "tied", "eighths")
RISK_WRONG = ("none", "all", "drawn")


def risk_case(N, scores, wrong, seed=0):
    """score fp64 [N] (all distinct / all tied / quantised to k / 8: the variation ratios of 8 passes) and wrong uint8 [N] (none /
    all / drawn, the errors more likely at the larger scores)"""
    rng = np.random.default_rng(17 * N + seed)
    if scores == "distinct":
        s = rng.permutation(N).astype(np.float64) / N + 0.125
    elif scores == "tied":
        s = np.full(N, 0.625)
    else:
        s = rng.integers(0, 8, N).astype(np.float64) / 8.0
    if wrong == "none":
        w = np.zeros(N, dtype=np.uint8)
    elif wrong == "all":
        w = np.ones(N, dtype=np.uint8)
    else:
        w = (rng.random(N) < 0.15 + 0.5 * (s - s.min())).astype(np.uint8)
    return s, w
