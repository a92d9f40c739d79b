"""Plain numpy restatement of csrc/subgroup.hip (the subgroup audit of a fold), as include/mmskin.h and DESIGN.md section 28 define
it.  It knows nothing of the kernel's tables or its scan: a group's integers in replicate b are bootstrap_oracle.integers on the
group's rows alone, under the weights bootstrap_oracle.weights drew on the WHOLE fold.  tests/test_cpu_subgroup.py holds it to hand
counts and to bootstrap_oracle.study; tests/test_gpu_subgroup_ops.py and tests/test_gpu_subgroup.py hold the kernels and
mmskin.subgroup.SubgroupAudit to it."""
import numpy as np

import bootstrap_oracle as bo

METRICS = bo.METRICS
CLASS_METRICS = bo.CLASS_METRICS + ("per_class_fpr", "per_class_predicted_rate")


def columns(K):
    return 7 + 4 * K


# --------------------------------------------------------------------------------------------------------- integers
def integers(scores, labels, preds, groups, G, w):
    """one replicate: (confusion int32 [G, K, K], counts int64 [G, 3 K] = pos, neg, wins2 within each group) under the weights w
    int [N] of the whole fold; a group id outside [0, G) is in no group"""
    scores = np.asarray(scores, dtype=np.float32)
    K = scores.shape[1]
    confusion, counts = np.zeros((G, K, K), dtype=np.int32), np.zeros((G, 3 * K), dtype=np.int64)
    for g in range(G):
        idx = np.flatnonzero(groups == g)
        if len(idx):
            confusion[g], n = bo.integers(scores[idx], labels[idx], preds[idx], w[idx])
            counts[g] = np.concatenate([n["pos"], n["neg"], n["wins2"]])
    return confusion, counts


# --------------------------------------------------------------------------------------------------------- metrics
def metrics(confusion, counts, min_rows=1):
    """one group of one replicate -> float64 [7 + 4 K]: the bootstrap columns, then the false-positive and predicted rates"""
    K = confusion.shape[0]
    pos = counts[:K]
    rows = int(pos.sum())
    out = np.full(columns(K), np.nan)
    if rows < max(int(min_rows), 1):
        return out
    parts = {"pos": counts[:K], "neg": counts[K:2 * K], "wins2": counts[2 * K:], "nan": 0}
    out[:7 + 2 * K] = bo.metric_table([bo.metrics(confusion, parts)], K)[:, 0]
    predicted = confusion.sum(axis=0).astype(np.float64)
    others = (rows - pos).astype(np.float64)
    false_pos = predicted - np.diag(confusion)
    out[7 + 2 * K:7 + 3 * K] = np.divide(false_pos, others, out=np.full(K, np.nan), where=others > 0)
    out[7 + 3 * K:] = predicted / rows
    return out


def study(scores, labels, preds, groups, G, seed, B, stratified=False, min_rows=1):
    """(point [G, M, 1], table [G, M, B], confusion int32 [B, G, K, K], counts int64 [B, G, 3 K], weights [B, N])"""
    scores, labels, groups = np.asarray(scores, dtype=np.float32), np.asarray(labels, dtype=np.int64), np.asarray(groups)
    N, K = scores.shape
    preds = bo.first_argmax(scores) if preds is None else np.asarray(preds, dtype=np.int64)
    w = bo.weights(seed, N, 0, B, labels if stratified else None)
    ints = [integers(scores, labels, preds, groups, G, w[b]) for b in range(B)]
    table = np.stack([np.stack([metrics(c[g], n[g], min_rows) for c, n in ints], axis=1) for g in range(G)])
    pc, pn = integers(scores, labels, preds, groups, G, np.ones(N, dtype=np.int32))
    point = np.stack([metrics(pc[g], pn[g], min_rows)[:, None] for g in range(G)])
    return point, table, np.stack([c for c, _ in ints]), np.stack([n for _, n in ints]), w


# --------------------------------------------------------------------------------------------------------- gaps
def gaps(table):
    """table [G, M, B] -> (lowest, highest, gap [M, B], lowest_group int64 [M, G]) over the groups that are not NaN"""
    G = table.shape[0]
    defined = ~np.isnan(table)
    count = defined.sum(axis=0)
    low_side, high_side = np.where(defined, table, np.inf), np.where(defined, table, -np.inf)
    lowest = np.where(count > 0, low_side.min(axis=0), np.nan)
    highest = np.where(count > 0, high_side.max(axis=0), np.nan)
    with np.errstate(invalid="ignore"):
        gap = np.where(count >= 2, highest - lowest, np.nan)
    first = low_side.argmin(axis=0)                                   # the first minimum: ties go to the smallest id
    lowest_group = np.stack([((first == g) & (count > 0)).sum(axis=1) for g in range(G)], axis=1).astype(np.int64)
    return lowest, highest, gap, lowest_group


def gap_summary(table, confidence=0.95):
    """float64 [3, 5, M]: bootstrap_oracle.summary of lowest, highest and gap"""
    return np.stack([bo.summary(t, confidence) for t in gaps(table)[:3]])


# --------------------------------------------------------------------------------------------------------- folds of the tests
def grouped_fold(N, K, G, seed=0):
    """scores fp32 [N, K] quantised to 1/8 (equal scores on both sides of group boundaries and inside tie groups), labels, groups
    int32 in -1 .. G-1 with uneven sizes: about a tenth of the rows in no group, group 1 (if G > 2) empty, the last group (if
    G > 1) holding rows of class 0 only"""
    rng = np.random.default_rng(7000 * N + 70 * K + 7 * G + seed)
    labels = rng.integers(0, K, N)
    labels[:min(N, K)] = np.arange(min(N, K))
    labels = rng.permutation(labels).astype(np.int64)
    raw = rng.random((N, K)) + 0.7 * np.eye(K)[labels]
    scores = (np.round(raw / raw.sum(axis=1, keepdims=True) * 8) / 8).astype(np.float32)
    share = rng.random(G) + 0.2
    groups = rng.choice(G, N, p=share / share.sum()).astype(np.int32)
    if G > 2:
        groups[groups == 1] = 0
    if G > 1:
        groups[(groups == G - 1) & (labels != 0)] = 0
    groups[rng.random(N) < 0.1] = -1
    return scores, labels, groups


def balanced_fold(per_cell=12, K=3, G=3, seed=0):
    """every group holds `per_cell` rows of every class, plus 9 rows in no group"""
    rng = np.random.default_rng(31 + seed)
    labels = np.concatenate([np.tile(np.repeat(np.arange(K), per_cell), G), rng.integers(0, K, 9)]).astype(np.int64)
    groups = np.concatenate([np.repeat(np.arange(G), per_cell * K), np.full(9, -1)]).astype(np.int32)
    mix = rng.permutation(len(labels))
    labels, groups = labels[mix], groups[mix]
    raw = rng.random((len(labels), K)) + (0.4 + 0.3 * (groups[:, None] + 1) / G) * np.eye(K)[labels]      # later groups score better
    return (np.round(raw / raw.sum(axis=1, keepdims=True) * 8) / 8).astype(np.float32), labels, groups


def rare_fold(seed=0):
    """N = 64, K = 3, G = 3: group 1 holds no row of class 2, group 2 holds 4 rows in all; 4 rows in no group"""
    rng = np.random.default_rng(57 + seed)
    labels = np.array([0] * 12 + [1] * 10 + [2] * 8 + [0] * 14 + [1] * 12 + [0, 1, 2, 2] + [0, 1, 2, 0], dtype=np.int64)
    groups = np.array([0] * 30 + [1] * 26 + [2] * 4 + [-1] * 4, dtype=np.int32)
    mix = rng.permutation(64)
    labels, groups = labels[mix], groups[mix]
    raw = rng.random((64, 3)) + 0.6 * np.eye(3)[labels]
    return (np.round(raw / raw.sum(axis=1, keepdims=True) * 8) / 8).astype(np.float32), labels, groups
