"""The one-vs-rest curves of include/mmskin.h (csrc/curves.hip, mmskin/curves.py) restated from the definitions in plain numpy with
int64, fp64 and Python integers, by direct counting (no sort, no cumulative sums) and independent of mmskin/curves.py.

    fold(N, C, kind)                               probs fp32 [N, C], labels int64 [N]
    curves(probs, labels)                          dict: thr fp32 [C, N], tp / fp int32 [C, N], n_points, pos, neg, nan
    summary(cv, specificities, sensitivities)      dict: auc, average_precision, youden_*, sens_at_spec_*, spec_at_sens_*
"""
import numpy as np

KINDS = ("continuous", "eighths", "constant", "separable")


def fold(N, C, kind, seed=0):
    """continuous: soft-max of Gaussians, the label's logit raised; eighths: those scores quantised to k / 8, so ties fall within
    and across the positives and the negatives; constant: every score equal (one threshold per class); separable: the label's
    column always the largest of the row.  Every class that fits gets a row."""
    assert kind in KINDS, kind
    rng = np.random.default_rng(1000 * N + 10 * C + seed)
    labels = rng.integers(0, C, N)
    labels[:min(N, C)] = np.arange(min(N, C))
    labels = rng.permutation(labels).astype(np.int64)
    logits = rng.standard_normal((N, C)) + (8.0 if kind == "separable" else 1.5) * np.eye(C)[labels]
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    probs = e / e.sum(axis=1, keepdims=True)
    if kind == "eighths":
        probs = np.round(probs * 8) / 8
    elif kind == "constant":
        probs[:] = 1.0 / C
    return probs.astype(np.float32), labels


def curves(probs, labels):
    N, C = probs.shape
    labels = np.asarray(labels, dtype=np.int64)
    valid = (labels >= 0) & (labels < C)
    p, y = probs[valid], labels[valid]
    out = {"thr": np.zeros((C, N), dtype=np.float32), "tp": np.zeros((C, N), dtype=np.int32), "fp": np.zeros((C, N), dtype=np.int32),
           "n_points": np.zeros(C, dtype=np.int32), "pos": np.zeros(C, dtype=np.int64), "neg": np.zeros(C, dtype=np.int64),
           "nan": int(np.isnan(p).sum())}
    for c in range(C):
        s, own = p[:, c], y == c
        out["pos"][c], out["neg"][c] = own.sum(), (~own).sum()
        thr = np.unique(s[~np.isnan(s)])[::-1]                       # the distinct values under ==, descending; never a NaN
        n = len(thr)
        ge = s[None, :] >= thr[:, None]                              # [n, rows]; a NaN row is >= nothing
        out["n_points"][c], out["thr"][c, :n] = n, thr
        out["tp"][c, :n], out["fp"][c, :n] = (ge & own).sum(axis=1), (ge & ~own).sum(axis=1)
    return out


def summary(cv, specificities=(), sensitivities=()):
    """Python-integer restatement of mmskin_ovr_curves_summary; an undefined value is NaN, an undefined index -1"""
    C, A, B = len(cv["pos"]), len(specificities), len(sensitivities)
    out = {"auc": np.full(C, np.nan), "average_precision": np.full(C, np.nan), "wins2": np.zeros(C, dtype=np.int64)}
    for name, n in (("youden", None), ("sens_at_spec", A), ("spec_at_sens", B)):
        shape = (C,) if n is None else (C, n)
        out[name + "_value"], out[name + "_threshold"] = np.full(shape, np.nan), np.full(shape, np.nan)
        out[name + "_index"] = np.full(shape, -1, dtype=np.int64)
    for c in range(C):
        pos, neg, n = int(cv["pos"][c]), int(cv["neg"][c]), int(cv["n_points"][c])
        tp, fp, thr = [int(v) for v in cv["tp"][c, :n]], [int(v) for v in cv["fp"][c, :n]], cv["thr"][c]
        area, tp_prev, fp_prev = 0, 0, 0
        for k in range(n):
            area += (fp[k] - fp_prev) * (tp[k] + tp_prev)
            tp_prev, fp_prev = tp[k], fp[k]
        out["wins2"][c] = area
        if pos == 0 or neg == 0:
            continue
        out["auc"][c] = np.float64(area) / (2.0 * np.float64(pos) * np.float64(neg))
        ap, tp_prev = 0.0, 0
        for k in range(n):
            ap += ((tp[k] - tp_prev) / pos) * (tp[k] / (tp[k] + fp[k]))
            tp_prev = tp[k]
        out["average_precision"][c] = ap

        def put(name, at, k, value):
            out[name + "_value"][at], out[name + "_index"][at] = value, k
            out[name + "_threshold"][at] = thr[k] if k >= 0 else np.inf

        best = None
        for k in range(n):                                           # exact: the numerators of J over the common pos neg
            if best is None or tp[k] * neg - fp[k] * pos > tp[best] * neg - fp[best] * pos:
                best = k
        if best is not None:
            put("youden", c, best, (tp[best] * neg - fp[best] * pos) / (pos * neg))
        for a, q in enumerate(specificities):
            best = None
            for k in range(n):
                if float(neg - fp[k]) >= float(q) * float(neg) and (best is None or tp[k] > tp[best]):
                    best = k
            put("sens_at_spec", (c, a), -1 if best is None else best, 0.0 if best is None else tp[best] / pos)
        for b, t in enumerate(sensitivities):
            best = None
            for k in range(n):
                if float(tp[k]) >= float(t) * float(pos) and (best is None or fp[k] < fp[best]):
                    best = k
            if best is not None:
                put("spec_at_sens", (c, b), best, (neg - fp[best]) / neg)
    return out
