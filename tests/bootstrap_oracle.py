"""Plain numpy restatement of csrc/bootstrap.hip (bootstrap confidence intervals of a fold's metrics): the generator, the
resample weights, the weighted integers of a replicate, the metrics, the summary and the paired comparison, as include/mmskin.h
and DESIGN.md section 23 define them.  tests/test_cpu_bootstrap.py holds it to sklearn; tests/test_gpu_bootstrap_ops.py and
tests/test_gpu_bootstrap.py hold the kernels and mmskin.bootstrap.BootstrapMetrics to it.

The metrics go through the package's own host functions (metrics_from_confusion, auc_from_counts, per_class_auc) applied to each
replicate's integers."""
import numpy as np

from mmskin.criterion import metrics_from_confusion
from mmskin.evaluate import auc_from_counts, per_class_auc

METRICS = ("accuracy", "balanced_accuracy", "precision", "recall", "f1_score", "auc", "macro_auc")
CLASS_METRICS = ("per_class_recall", "per_class_auc")
_M64 = (1 << 64) - 1


# --------------------------------------------------------------------------------------------------------- generator
def mix64(x):
    """common.h's splitmix64 finaliser on Python ints"""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def draw(seed, b, t):
    """u of replicate b, draw t: the high 32 bits of mix64(mix64(seed) ^ (b << 32 | t))"""
    return mix64(mix64(int(seed) & _M64) ^ ((int(b) << 32) | int(t))) >> 32


def weights(seed, N, b0, b1, labels=None):
    """int32 [b1 - b0, N].  labels None: plain resampling, draw t hits row (u N) >> 32.  With labels (all in range): stratified,
    draw t hits the ((u n_c) >> 32)-th of the rows that share row t's label c, in ascending order."""
    w = np.zeros((b1 - b0, N), dtype=np.int32)
    members = None if labels is None else {c: np.flatnonzero(np.asarray(labels) == c) for c in np.unique(labels)}
    for b in range(b0, b1):
        for t in range(N):
            u = draw(seed, b, t)
            if labels is None:
                w[b - b0, (u * N) >> 32] += 1
            else:
                m = members[labels[t]]
                w[b - b0, m[(u * len(m)) >> 32]] += 1
    return w


# --------------------------------------------------------------------------------------------------------- integers
def first_argmax(scores):
    return np.argmax(np.asarray(scores), axis=1).astype(np.int64)


def wins2(s, i, j):
    """auc_pairs.h: 2 for a win, 1 for a tie, in fp32"""
    a, b = np.float32(s[i]), np.float32(s[j])
    return 2 if a > b else (1 if a == b else 0)


def integers(scores, labels, preds, w):
    """one replicate: (confusion int32 [K, K], dict(pos, neg, wins2 int64 [K], nan 0)) under the weights w int [N]"""
    scores = np.asarray(scores, dtype=np.float32)
    N, K = scores.shape
    confusion = np.zeros((K, K), dtype=np.int32)
    for i in range(N):
        confusion[labels[i], preds[i]] += w[i]
    pos = np.array([int(w[labels == c].sum()) for c in range(K)], dtype=np.int64)
    neg = int(w.sum()) - pos
    wins = np.zeros(K, dtype=np.int64)
    for c in range(K):
        col = scores[:, c]
        own, rest = np.flatnonzero(labels == c), np.flatnonzero(labels != c)
        if len(own) and len(rest):
            by_score = rest[np.argsort(col[rest], kind="stable")]
            below = np.concatenate([[0], np.cumsum(w[by_score].astype(np.int64))])     # below[k] = the weight of the k lowest negatives
            less = below[np.searchsorted(col[by_score], col[own], side="left")]
            not_above = below[np.searchsorted(col[by_score], col[own], side="right")]
            wins[c] = int((w[own].astype(np.int64) * (less + not_above)).sum())        # 2 less + ties = less + (less + ties)
    return confusion, {"pos": pos, "neg": neg, "wins2": wins, "nan": 0}


def integers_by_loops(scores, labels, preds, w):
    """the wins2 [K] of `integers` as literal O(N^2) pair loops, for small folds"""
    scores = np.asarray(scores, dtype=np.float32)
    N, K = scores.shape
    wins = np.zeros(K, dtype=np.int64)
    for c in range(K):
        for i in range(N):
            if labels[i] != c:
                continue
            for j in range(N):
                if labels[j] != c:
                    wins[c] += int(w[i]) * int(w[j]) * wins2(scores[:, c], i, j)
    return wins


# --------------------------------------------------------------------------------------------------------- metrics
def metrics(confusion, counts):
    """one replicate -> dict of the 7 scalar metrics (float, NaN where undefined) and the two per-class arrays [K]"""
    K = confusion.shape[0]
    out = dict(metrics_from_confusion(confusion))
    out["auc"] = auc_from_counts(counts, K)
    per_class = per_class_auc(counts)
    ok = ~np.isnan(per_class)
    out["macro_auc"] = float(per_class[ok].mean()) if ok.any() else float("nan")
    true_n = confusion.sum(axis=1).astype(np.float64)
    out["per_class_recall"] = np.divide(np.diag(confusion).astype(np.float64), true_n, out=np.full(K, np.nan), where=true_n > 0)
    out["per_class_auc"] = per_class
    return out


def metric_table(all_metrics, K):
    """list of B metric dicts -> float64 [7 + 2 K, B] in the column order of mmskin.h"""
    B = len(all_metrics)
    table = np.empty((7 + 2 * K, B), dtype=np.float64)
    for b, m in enumerate(all_metrics):
        table[:7, b] = [m[name] for name in METRICS]
        table[7:7 + K, b] = m["per_class_recall"]
        table[7 + K:, b] = m["per_class_auc"]
    return table


def study(scores, labels, preds, seed, B, stratified=False):
    """(point table [M, 1], table [M, B], confusion int32 [B, K, K], counts int64 [B, 3 K], weights [B, N])"""
    scores, labels = np.asarray(scores, dtype=np.float32), np.asarray(labels, dtype=np.int64)
    N, K = scores.shape
    preds = first_argmax(scores) if preds is None else np.asarray(preds, dtype=np.int64)
    w = weights(seed, N, 0, B, labels if stratified else None)
    ints = [integers(scores, labels, preds, w[b]) for b in range(B)]
    table = metric_table([metrics(c, n) for c, n in ints], K)
    point = metric_table([metrics(*integers(scores, labels, preds, np.ones(N, dtype=np.int32)))], K)
    confusion = np.stack([c for c, _ in ints])
    counts = np.stack([np.concatenate([n["pos"], n["neg"], n["wins2"]]) for _, n in ints])
    return point, table, confusion, counts, w


# --------------------------------------------------------------------------------------------------------- summary
def summary(table, confidence=0.95):
    """float64 [5, M]: n_valid, mean, std (ddof = 1), low, high over the non-NaN entries of each row of table [M, B]"""
    a = 1.0 - confidence
    out = np.full((5, table.shape[0]), np.nan)
    for m, row in enumerate(table):
        v = row[~np.isnan(row)]
        out[0, m] = len(v)
        if len(v) == 0:
            continue
        total = 0.0
        for x in v:                                                  # in replicate order
            total += x
        mean = total / len(v)
        out[1, m] = mean
        if len(v) > 1:
            sq = 0.0
            for x in v:
                sq += (x - mean) * (x - mean)
            out[2, m] = np.sqrt(sq / (len(v) - 1))
        out[3, m], out[4, m] = np.nanpercentile(row, [100 * a / 2, 100 * (1 - a / 2)])
    return out


def compare(table_a, table_b, confidence=0.95):
    """(delta [M, B], its summary [5, M], p [M]): p = min(1, 2 min((#{d <= 0} + 1) / (n + 1), (#{d >= 0} + 1) / (n + 1)))"""
    delta = table_a - table_b
    s = summary(delta, confidence)
    p = np.empty(delta.shape[0])
    for m, row in enumerate(delta):
        n = int((~np.isnan(row)).sum())
        le, ge = int((row <= 0).sum()), int((row >= 0).sum())
        p[m] = min(1.0, 2.0 * min((le + 1) / (n + 1), (ge + 1) / (n + 1)))
    return delta, s, p
