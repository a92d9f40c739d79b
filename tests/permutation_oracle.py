"""Plain numpy restatement of csrc/permute.hip (permutation importance of the metadata on a validation fold): the generator, the
argsort permutation, the row mixing, the scores of a cell, the metrics and the finalize step.  tests/test_cpu_permutation.py holds
it to sklearn; tests/test_gpu_permutation.py holds the kernels and mmskin.permutation.MetadataPermutationImportance to it.

Three knobs exist only so that the CPU tests can show that a wrong restatement is caught: `shift_group` (rows: shuffle the columns
of another group), `ddof` (finalize) and `count_absent` (metrics: divide the AUC sum by all K classes)."""
import numpy as np

METRICS = ("accuracy", "balanced_accuracy", "auc")
MAX_SAMPLES = 4096
_M64 = (1 << 64) - 1


# --------------------------------------------------------------------------------------------------------- generator
def mix64(x):
    """common.h's splitmix64 finaliser on uint64 arrays (wrapping arithmetic)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def keys(seed, r, g, lo, hi):
    """the 64-bit sort keys of positions lo .. hi-1 of cell (r, g): (h >> 32) << 32 | i, h = mix64(mix64(seed) ^ (r << 40 | g << 20 | i))"""
    i = np.arange(lo, hi, dtype=np.uint64)
    counter = np.uint64((int(r) << 40) | (int(g) << 20)) | i
    h = mix64(mix64(np.uint64(int(seed) & _M64)) ^ counter)
    return ((h >> np.uint64(32)) << np.uint64(32)) | i


def indices(seed, R, G, S, chunk=None):
    """int32 [R, G, S]: perm[r, g] = the positions in ascending order of their keys.  `chunk`: draw the keys that many positions at
    a time (the result does not depend on it: a key is a function of its own position)."""
    chunk = S if chunk is None else int(chunk)
    perm = np.empty((R, G, S), dtype=np.int32)
    for r in range(R):
        for g in range(G):
            k = np.concatenate([keys(seed, r, g, lo, min(lo + chunk, S)) for lo in range(0, S, chunk)])
            perm[r, g] = (np.sort(k) & np.uint64(0xFFFFFFFF)).astype(np.int32)
    return perm


# --------------------------------------------------------------------------------------------------------- rows
def rows(x, group, perm, row0=0, row1=None, shift_group=0):
    """x fp32 [S, W], group int [W] (-1: never shuffled), perm int [R, G, S] -> rows [row0, row1) of the study, row = (r G + g) S + s:
    x[s] with the columns of group g taken from x[perm[r, g, s]]"""
    x, group = np.asarray(x, dtype=np.float32), np.asarray(group)
    R, G, S = perm.shape
    row1 = R * G * S if row1 is None else row1
    out = np.empty((row1 - row0, x.shape[1]), dtype=np.float32)
    for n, row in enumerate(range(row0, row1)):
        cell, s = divmod(row, S)
        r, g = divmod(cell, G)
        p = int(perm[r, g, s])
        src = p if 0 <= p < S else s
        out[n] = np.where(group == (g + shift_group) % G, x[src], x[s])
    return out


# --------------------------------------------------------------------------------------------------------- scores of a cell
def softmax32(logits):
    """the kernel's soft-max: e = exp(x - max) taken in fp64 and rounded to fp32, summed over c = 0 .. K-1 in fp32, e / sum in fp32"""
    x = np.asarray(logits, dtype=np.float32)
    top = x.max(axis=-1, keepdims=True)
    e = np.exp((x - top).astype(np.float64)).astype(np.float32)
    total = np.zeros(x.shape[:-1], dtype=np.float32)
    for c in range(x.shape[-1]):
        total = total + e[..., c]
    return e / total[..., None]


def cell_counts(logits, labels, probs=None):
    """logits fp32 [S, K], labels int [S] -> (confusion int32 [K, K] = [true][first arg-max of the logits], counts int64 [3 K + 1] =
    pos, neg, wins2, nan of the soft-max, the block of mmskin_ovr_auc_counts).  Labels outside [0, K) count nowhere.  `probs`
    replaces the soft-max (float64 scores in the tests against sklearn)."""
    logits, y = np.asarray(logits), np.asarray(labels).astype(np.int64)
    S, K = logits.shape
    p = softmax32(logits) if probs is None else np.asarray(probs)
    valid = (y >= 0) & (y < K)
    pred = logits.argmax(axis=1)
    confusion = np.zeros((K, K), dtype=np.int32)
    np.add.at(confusion, (y[valid], pred[valid]), 1)
    counts = np.zeros(3 * K + 1, dtype=np.int64)
    for c in range(K):
        own, other = p[valid & (y == c), c], p[valid & (y != c), c]
        counts[c], counts[K + c] = len(own), len(other)
        counts[2 * K + c] = int((2 * (own[:, None] > other[None, :]) + (own[:, None] == other[None, :])).sum())
    counts[3 * K] = int(np.isnan(p[valid]).sum())
    return confusion, counts


def per_class_auc(counts):
    K = (len(counts) - 1) // 3
    pairs = 2.0 * counts[:K].astype(np.float64) * counts[K:2 * K].astype(np.float64)
    return np.divide(counts[2 * K:3 * K].astype(np.float64), pairs, out=np.full(K, np.nan), where=pairs > 0)


def metrics(confusion, counts, count_absent=False):
    """float64 [3]: accuracy, balanced accuracy (mean recall over the classes that occur), macro one-vs-rest AUC (mean over the
    classes with a positive and a negative row; NaN when there is none or a probability is NaN); sums in ascending class order"""
    cm = np.asarray(confusion, dtype=np.int64)
    K = cm.shape[0]
    n, hits = int(cm.sum()), int(np.trace(cm))
    recall_sum, present = 0.0, 0
    for a in range(K):
        true_n = int(cm[a].sum())
        if true_n > 0:
            recall_sum += float(cm[a, a]) / float(true_n)
            present += 1
    auc, auc_sum, ranked = per_class_auc(np.asarray(counts)), 0.0, 0
    for c in range(K):
        if not np.isnan(auc[c]):
            auc_sum += auc[c]
            ranked += 1
    nan = float("nan")
    divisor = K if count_absent else ranked
    return np.array([hits / n if n > 0 else nan, recall_sum / present if present > 0 else nan,
                     auc_sum / divisor if ranked > 0 and counts[3 * K] == 0 else nan], dtype=np.float64)


# --------------------------------------------------------------------------------------------------------- finalize
def finalize(cell_metrics, baseline, ddof=0):
    """cell_metrics float64 [R, G, 3], baseline [3] -> dict(metrics, importances [3, G, R], mean, std [3, G]): importances =
    baseline - metric; mean and deviation over r = 0 .. R-1 summed in that order, std = sqrt(sum (v - mean)^2 / (R - ddof))"""
    m = np.ascontiguousarray(np.transpose(np.asarray(cell_metrics, dtype=np.float64), (2, 1, 0)))
    R = m.shape[2]
    imp = np.asarray(baseline, dtype=np.float64)[:, None, None] - m
    total = np.zeros(m.shape[:2])
    for r in range(R):
        total = total + imp[:, :, r]
    mean = total / float(R)
    sq = np.zeros(m.shape[:2])
    for r in range(R):
        sq = sq + (imp[:, :, r] - mean) * (imp[:, :, r] - mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        std = np.sqrt(sq / float(R - ddof))
    return dict(metrics=m, importances=imp, mean=mean, std=std)


def study(base_logits, cube_logits, labels, ddof=0, count_absent=False):
    """base_logits [S, K] of the unshuffled fold and cube_logits [R, G, S, K] of the study -> finalize's dict + baseline [3]"""
    baseline = metrics(*cell_counts(base_logits, labels), count_absent=count_absent)
    R, G = cube_logits.shape[:2]
    cells = np.array([[metrics(*cell_counts(cube_logits[r, g], labels), count_absent=count_absent) for g in range(G)] for r in range(R)])
    out = finalize(cells, baseline, ddof=ddof)
    out["baseline"] = baseline
    return out


# --------------------------------------------------------------------------------------------------------- fixtures
def onehot_case(S, blocks, seed, pad_to=None):
    """encoded rows fp32 [S, W] of one-hot blocks of the given widths (plus zero columns up to pad_to), and the column -> group map
    with one group per block (-1 on the padding)"""
    rng = np.random.default_rng(seed)
    W = sum(blocks)
    x = np.zeros((S, pad_to or W), dtype=np.float32)
    group = np.full(pad_to or W, -1, dtype=np.int32)
    at = 0
    for g, width in enumerate(blocks):
        x[np.arange(S), at + rng.integers(0, width, S)] = 1.0
        group[at:at + width] = g
        at += width
    return x, group


def scores_case(R, G, S, K, seed):
    """logits [R G S, K] and labels [S] with planted structure: rows whose logits are exact copies of another row's (tied scores in
    every column), rows with two equal top logits (the first index must predict), the last class absent from the labels, and one
    label outside [0, K)"""
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 2, (R * G * S, K)).astype(np.float32)
    labels = rng.integers(0, K - 1, S).astype(np.int64)                # class K - 1 never occurs
    if S >= 4:
        labels[0], labels[1] = 0, min(1, K - 2)                         # a tied pair with different labels where K allows it
        labels[S - 1] = -3
    for cell in range(R * G):
        rows_ = logits[cell * S:(cell + 1) * S]
        if S >= 4:
            rows_[1] = rows_[0]
            rows_[S // 2] = rows_[S // 2 - 1]
            rows_[2, 1] = rows_[2, 0] = rows_[2].max() + 1.0            # two equal top logits: class 0 is predicted
    return logits, labels
