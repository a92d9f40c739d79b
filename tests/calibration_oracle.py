"""The calibration definitions of include/mmskin.h restated in plain numpy (fp64, int64 and Python integers): what
csrc/calibration.hip and mmskin.calibration are held to.  Loops over rows and bins on purpose: nothing here is clever.

A 4-row, 2-bin, 2-class example, worked by hand (edges 0, 0.5, 1; S = 2^30):

    row   p            label   pred   top-label confidence   hit
    0     (0.75, 0.25)   0       0      0.75  -> bin 1         1
    1     (0.5,  0.5)    1       0      0.5   -> bin 0 (on the edge: the lower bin)   0
    2     (0.25, 0.75)   0       1      0.75  -> bin 1         0
    3     (1.0,  0.0)    0       0      1.0   -> bin 1         1

    table 0:  bin 0: count 1, hits 0, conf 0.5 S        bin 1: count 3, hits 2, conf 2.5 S
    ece  = (|0 - 0.5| + |2 - 2.5|) / 4 = 0.25;   mce = max(0.5 / 1, 0.5 / 3) = 0.5;   confidence_gap = (3.0 - 2) / 4 = 0.25
    table 1 (class 0, p[:, 0] = 0.75, 0.5, 0.25, 1.0; hits 1, 0, 1, 1):  bin 0: count 2, hits 1, conf 0.75 S;  bin 1: count 2,
    hits 2, conf 1.75 S;  ece = (0.25 + 0.25) / 4 = 0.125
    table 2 (class 1, p[:, 1] = 0.25, 0.5, 0.75, 0.0; hits 0, 1, 0, 0):  bin 0: count 3, hits 1, conf 0.75 S;  bin 1: count 1,
    hits 0, conf 0.75 S;  ece = (0.25 + 0.75) / 4 = 0.25;   classwise_ece = 0.1875
    brier = (0.125 + 0.5 + 1.125 + 0) / 4 = 0.4375;   nll = -(ln 0.75 + ln 0.5 + ln 0.25 + ln 1) / 4
"""
import numpy as np

S_LOG2 = 30
S = 1 << S_LOG2
METRICS = ("ece", "mce", "classwise_ece", "confidence_gap", "brier", "nll")
FLT_MIN = float(np.finfo(np.float32).tiny)

EXAMPLE_PROBS = np.array([[0.75, 0.25], [0.5, 0.5], [0.25, 0.75], [1.0, 0.0]], dtype=np.float32)
EXAMPLE_LABELS = np.array([0, 1, 0, 0], dtype=np.int64)
EXAMPLE_TABLES = np.array([[[1, 0, S // 2], [3, 2, 5 * S // 2]],
                           [[2, 1, 3 * S // 4], [2, 2, 7 * S // 4]],
                           [[3, 1, 3 * S // 4], [1, 0, 3 * S // 4]]], dtype=np.int64)


def fold(N, K, kind, seed=0):
    """probs fp32 [N, K], labels int64 [N], built like the folds of test_gpu_bootstrap_ops.py: every class that fits gets a row;
    kind: continuous, eighths (quantised to 1/8: confidences exactly on the edges of 8 bins), or constant (column 0 all ties)"""
    rng = np.random.default_rng(1000 * N + 10 * K + seed)
    labels = rng.integers(0, K, N)
    labels[:min(N, K)] = np.arange(min(N, K))
    labels = rng.permutation(labels).astype(np.int64)
    raw = rng.random((N, K)) + 0.7 * np.eye(K)[labels]
    probs = raw / raw.sum(axis=1, keepdims=True)
    if kind == "eighths":
        probs = np.round(probs * 8) / 8
    elif kind == "constant":
        probs[:, 0] = 0.25
    return probs.astype(np.float32), labels


def first_argmax(probs):
    out = np.zeros(len(probs), dtype=np.int64)
    for i, row in enumerate(probs):
        for k in range(1, len(row)):
            if row[k] > row[out[i]]:
                out[i] = k
    return out


def uniform_edges(K, n_bins):
    row = np.array([np.float32(j / n_bins) for j in range(n_bins + 1)], dtype=np.float32)
    return np.tile(row, (K + 1, 1))


def confidences(probs):
    """fp32 [K + 1, N]"""
    pred = first_argmax(probs)
    return np.concatenate([probs[np.arange(len(probs)), pred][None], probs.T], axis=0).astype(np.float32)


def quantile_edges(probs, n_bins):
    N, K = probs.shape
    edges = np.zeros((K + 1, n_bins + 1), dtype=np.float32)
    edges[:, n_bins] = 1.0
    for t, conf in enumerate(confidences(probs)):
        ordered = np.sort(conf)
        for j in range(1, n_bins):
            edges[t, j] = ordered[(j * N + n_bins - 1) // n_bins - 1]
    return edges


def codes(probs, labels, edges):
    """(bin, q, hit), each int64 [K + 1, N]"""
    N, K = probs.shape
    n_bins = edges.shape[1] - 1
    pred = first_argmax(probs)
    conf = confidences(probs)
    b, q, hit = (np.zeros((K + 1, N), dtype=np.int64) for _ in range(3))
    for t in range(K + 1):
        for i in range(N):
            p = conf[t, i]
            b[t, i] = sum(1 for j in range(1, n_bins) if edges[t, j] < p)       # an fp32 compare
            q[t, i] = int(np.rint(np.float64(p) * S))
            hit[t, i] = (pred[i] == labels[i]) if t == 0 else (labels[i] == t - 1)
    return b, q, hit


def tables(the_codes, n_bins, w=None):
    """int64 [K + 1, n_bins, 3]: count, hits, conf of one replicate (w None: all ones)"""
    b, q, hit = the_codes
    T, N = b.shape
    w = np.ones(N, dtype=np.int64) if w is None else np.asarray(w, dtype=np.int64)
    out = np.zeros((T, n_bins, 3), dtype=np.int64)
    for t in range(T):
        for i in range(N):
            out[t, b[t, i]] += (w[i], w[i] * hit[t, i], w[i] * q[t, i])
    return out


def sums(probs, labels, w=None):
    """(Brier sum, NLL sum) in fp64, math.fsum: the correctly rounded sums"""
    import math
    N, K = probs.shape
    w = np.ones(N) if w is None else np.asarray(w, dtype=np.float64)
    p = probs.astype(np.float64)
    brier = [w[i] * sum((p[i, k] - (labels[i] == k)) ** 2 for k in range(K)) for i in range(N)]
    nll = [w[i] * -math.log(max(float(probs[i, labels[i]]), FLT_MIN)) for i in range(N)]
    return math.fsum(brier), math.fsum(nll)


def metrics(table, the_sums):
    """float64 [6 + K] from one replicate's integers, in exact Python integers up to the last division"""
    import math
    K = table.shape[0] - 1
    out = np.full(6 + K, np.nan)
    W = int(table[0, :, 0].sum())
    if W == 0:
        return out
    eces = []
    for t in range(K + 1):
        gaps = [abs(int(h) * S - int(c)) for _, h, c in table[t]]
        eces.append(sum(gaps) / (S * W))
        if t == 0:
            out[1] = max(g / (S * int(n)) for g, (n, _, _) in zip(gaps, table[t]) if n > 0)
            out[3] = (sum(int(c) for c in table[0, :, 2]) - S * sum(int(h) for h in table[0, :, 1])) / (S * W)
    out[0] = eces[0]
    out[2] = math.fsum(eces[1:]) / K
    out[4], out[5] = the_sums[0] / W, the_sums[1] / W
    out[6:] = eces[1:]
    return out


def ece_by_means(probs, labels, edges):
    """the textbook form of the top-label ECE: sum_b (n_b / N) |acc_b - conf_b|, in fp64"""
    b, _, hit = codes(probs, labels, edges)
    conf = confidences(probs)[0].astype(np.float64)
    total = 0.0
    for k in range(edges.shape[1] - 1):
        m = b[0] == k
        if m.any():
            total += m.sum() / len(labels) * abs(hit[0][m].mean() - conf[m].mean())
    return total


# ------------------------------------------------------------------------------------------------ temperature scaling
def logits_of(src, from_probs):
    return np.log(np.maximum(src, np.float32(FLT_MIN)).astype(np.float64)) if from_probs else src.astype(np.float64)


def temperature_stats(src, labels, betas, from_probs=False):
    """float64 [G, 3]: the NLL sum of softmax(beta z), its first and second derivative in beta"""
    import math
    z = logits_of(src, from_probs)
    out = np.zeros((len(betas), 3))
    for g, beta in enumerate(betas):
        rows = [[], [], []]
        for zi, y in zip(z, labels):
            d = zi - zi.max()
            e = np.exp(beta * d)
            pi = e / e.sum()
            mean = float((pi * d).sum())
            rows[0].append(math.log(e.sum()) - beta * d[y])
            rows[1].append(mean - d[y])
            rows[2].append(float((pi * (d - mean) ** 2).sum()))
        out[g] = [math.fsum(r) for r in rows]
    return out


def softmax(src, beta, from_probs=False):
    z = beta * logits_of(src, from_probs)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def fit_temperature(src, labels, from_probs=False, bounds=(1.0 / 64, 64.0)):
    """(beta, at_bound): bisection on the sign of the derivative, in log beta"""
    grad = lambda beta: temperature_stats(src, labels, [beta], from_probs)[0]
    lo, hi = 1.0 / bounds[1], 1.0 / bounds[0]
    g_lo, g_hi = grad(lo), grad(hi)
    if g_lo[1] == 0.0 and g_hi[1] == 0.0 and g_lo[2] == 0.0 and g_hi[2] == 0.0:
        return 1.0, False
    if g_lo[1] >= 0.0:
        return lo, True
    if g_hi[1] <= 0.0:
        return hi, True
    for _ in range(200):
        mid = np.sqrt(lo * hi)
        if not lo < mid < hi:
            break
        if grad(mid)[1] < 0.0:
            lo = mid
        else:
            hi = mid
    return float(np.sqrt(lo * hi)), False
