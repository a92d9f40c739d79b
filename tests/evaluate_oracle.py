"""A numpy restatement of the evaluation metrics, independent of mmskin/evaluate.py and of csrc/auc.hip: the one-vs-rest AUC
counts by sorting, the reference's AUC rule (utils/model_metrics.py:106-119) and its discrete metrics (:91-101) from labels and
predictions.  tests/test_cpu_evaluate.py pins it to tests/golden/evaluate.json, recorded from the reference's own
evaluate_model; the GPU tests then hold the kernel to it.

Counts, for every class c over the rows whose label lies in [0, C):
    pos[c]    rows labelled c                 neg[c]    the other rows
    wins2[c]  sum over (i labelled c, j not) of 2 [p[i, c] > p[j, c]] + [p[i, c] == p[j, c]]   (a NaN is neither)
    nan       NaN entries of those rows
"""
import json
import math
import os

import numpy as np
import torch

DISCRETE = ("accuracy", "balanced_accuracy", "precision", "recall", "f1_score")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluate.json")


def counts(probs, labels):
    probs, labels = np.asarray(probs), np.asarray(labels).astype(np.int64)
    N, C = probs.shape
    rows = np.flatnonzero((labels >= 0) & (labels < C))
    pos, neg, wins2 = np.zeros(C, np.int64), np.zeros(C, np.int64), np.zeros(C, np.int64)
    for c in range(C):
        mine, rest = rows[labels[rows] == c], rows[labels[rows] != c]
        pos[c], neg[c] = len(mine), len(rest)
        a, b = probs[mine, c], probs[rest, c]
        a, b = a[~np.isnan(a)], b[~np.isnan(b)]
        # rank the positives inside the sorted union: a stable merge sort keeps equal scores in input order, so with the
        # negatives first a positive's position counts the negatives <= it, with the positives first the negatives < it
        le = np.flatnonzero(np.argsort(np.concatenate([b, a]), kind="stable") >= len(b)) - np.arange(len(a))
        lt = np.flatnonzero(np.argsort(np.concatenate([a, b]), kind="stable") < len(a)) - np.arange(len(a))
        wins2[c] = int(le.sum()) + int(lt.sum())
    return {"pos": pos, "neg": neg, "wins2": wins2, "nan": int(np.isnan(probs[rows]).sum())}


def counts_brute(probs, labels):
    """the definition, pair by pair: O(N^2) memory per class, for small N only"""
    probs, labels = np.asarray(probs), np.asarray(labels).astype(np.int64)
    N, C = probs.shape
    rows = np.flatnonzero((labels >= 0) & (labels < C))
    out = {"pos": np.zeros(C, np.int64), "neg": np.zeros(C, np.int64), "wins2": np.zeros(C, np.int64), "nan": int(np.isnan(probs[rows]).sum())}
    for c in range(C):
        a, b = probs[rows[labels[rows] == c], c][:, None], probs[rows[labels[rows] != c], c][None, :]
        out["pos"][c], out["neg"][c] = a.shape[0], b.shape[1]
        out["wins2"][c] = 2 * int((a > b).sum()) + int((a == b).sum())
    return out


def same(got, want, tol=1e-12):
    """two metric values agree: None with None, NaN with NaN, numbers within tol"""
    if want is None or got is None:
        return got is None and want is None
    if math.isnan(want) or math.isnan(got):
        return math.isnan(got) and math.isnan(want)
    return abs(got - want) <= tol


def per_class_auc(cnt):
    with np.errstate(divide="ignore", invalid="ignore"):
        auc = cnt["wins2"].astype(np.float64) / (2.0 * cnt["pos"].astype(np.float64) * cnt["neg"].astype(np.float64))
    auc[(cnt["pos"] == 0) | (cnt["neg"] == 0)] = np.nan
    return auc


def auc(cnt):
    """None with a NaN probability; class 1 for two classes; else the pos-weighted mean over the classes with both kinds of row
    (NaN when there is none)"""
    if cnt["nan"]:
        return None
    a = per_class_auc(cnt)
    if len(a) == 2:
        return float(a[1])
    total, weight = 0.0, 0.0
    for c in range(len(a)):
        if not np.isnan(a[c]):
            total += a[c] * float(cnt["pos"][c])
            weight += float(cnt["pos"][c])
    return total / weight if weight else float("nan")


def discrete(labels, preds, C):
    """accuracy, balanced accuracy and precision / recall / F1 (two classes: of class 1; more: weighted by support,
    zero_division=0) from labels and predictions, class by class"""
    labels, preds = np.asarray(labels), np.asarray(preds)
    n = len(labels)
    prec, rec, f1, support = [], [], [], []
    for c in range(C):
        tp = int(((labels == c) & (preds == c)).sum())
        fp = int(((labels != c) & (preds == c)).sum())
        fn = int(((labels == c) & (preds != c)).sum())
        prec.append(tp / (tp + fp) if tp + fp else 0.0)
        rec.append(tp / (tp + fn) if tp + fn else 0.0)
        f1.append(2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0)
        support.append(tp + fn)
    present = [c for c in range(C) if support[c]]
    out = {"accuracy": float((labels == preds).sum() / n), "balanced_accuracy": float(np.mean([rec[c] for c in present]))}
    if C == 2:
        out.update(precision=prec[1], recall=rec[1], f1_score=f1[1])
    else:
        avg = lambda v: float(sum(v[c] * support[c] for c in range(C)) / n)
        out.update(precision=avg(prec), recall=avg(rec), f1_score=avg(f1))
    return out


def metrics(labels, preds, probs):
    C = np.asarray(probs).shape[1]
    out = discrete(labels, preds, C)
    out["auc"] = auc(counts(probs, labels))
    return out


# ---------------------------------------------------------------------------------------------- the golden cases
GOLDEN_CASES = ("c6_n97", "c2_n64", "c6_class_absent", "c3_single_class", "c6_ties")
BATCHES = {"c6_n97": (40, 40, 17)}                       # the others: one batch of 32, then the rest


def golden_inputs(name):
    """seeded logits (fp32-representable float64 -> float32) and int64 labels of a golden case"""
    rng = np.random.default_rng(GOLDEN_CASES.index(name) + 20)
    N, C = {"c6_n97": (97, 6), "c2_n64": (64, 2), "c6_class_absent": (50, 6), "c3_single_class": (20, 3), "c6_ties": (60, 6)}[name]
    logits = rng.normal(0.0, 1.5, (N, C)).astype(np.float32)
    labels = rng.integers(0, C, N)
    logits[np.arange(N), labels] += 0.8                               # better than chance, far from perfect
    if name == "c6_class_absent":
        labels[labels == 4] = 1
    if name == "c3_single_class":
        labels[:] = 2
    if name == "c6_ties":
        logits[20:40] = logits[0:20]                                  # duplicated rows under other labels: equal scores across classes
        logits[40:50] = logits[0:10]
    return logits, labels.astype(np.int64)


def batch_sizes(name, N):
    if name in BATCHES:
        return BATCHES[name]
    return (32, N - 32) if N > 32 else (N,)


class StoredLogits(torch.nn.Module):
    """model(images, metadata) -> the stored logits of the rows whose indices `images` carries"""

    def __init__(self, logits):
        super().__init__()
        self.register_buffer("logits", logits)

    def forward(self, images, metadata):
        return self.logits[images]


def loader_for(labels, sizes):
    """a plain list of (image_names, images, metadata, labels) batches; `images` holds the row indices"""
    batches, row = [], 0
    for n in sizes:
        idx = torch.arange(row, row + n)
        batches.append(([f"img_{i:04d}.png" for i in idx.tolist()], idx, torch.zeros(n, 1), torch.from_numpy(labels[row:row + n])))
        row += n
    return batches


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
