"""Host restatement of mmskin.conformal (csrc/conformal.hip; the contract is in include/mmskin.h) in plain numpy / fp64: the order of
a row and its ranks, the three scores, the rows' u, the counter-based split draw bit for bit, the quantile index, the sets and every
count.  Independent of the library: the tests hold the kernels to it, exactly."""
import math

import numpy as np

KINDS = ("lac", "aps", "raps")
METRICS = ("coverage", "mean_set_size", "singleton_rate", "singleton_accuracy", "empty_rate", "worst_class_coverage")
_U_STREAM = np.uint64(0xFFFFFFFF)


# --------------------------------------------------------------------------------------------------------- generator
def mix64(x):
    """common.h's splitmix64 finaliser on uint64 arrays (the arithmetic wraps)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def row_hash(seed, r, rows):
    """mix64(mix64(seed) ^ (r << 32 | row)) for an array of rows"""
    key = mix64(np.uint64(int(seed) & ((1 << 64) - 1)))
    return mix64(key ^ ((np.uint64(r) << np.uint64(32)) | (np.asarray(rows, dtype=np.uint64) & np.uint64(0xFFFFFFFF))))


def row_u(seed, rows):
    """fp64 u in [0, 1) of every row: the top 53 bits of the hash of stream 0xFFFFFFFF"""
    return (row_hash(seed, _U_STREAM, rows) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


# --------------------------------------------------------------------------------------------------------- scores
def ranks(probs):
    """int [N, C], 1-based: descending, stable, a tie goes to the lower class index (a literal count of the classes above)"""
    p = np.asarray(probs, dtype=np.float64)
    N, C = p.shape
    idx = np.arange(C)
    above = (p[:, None, :] > p[:, :, None]) | ((p[:, None, :] == p[:, :, None]) & (idx[None, None, :] < idx[None, :, None]))
    return above.sum(axis=2) + 1


def scores(probs, kind, randomized=False, seed=0, lam=0.0, k_reg=0, row0=0):
    """(score fp64 [N, C], rank int [N, C]); the prefix sums run in rank order, one addition at a time"""
    assert kind in KINDS
    p = np.asarray(probs).astype(np.float64)
    N, C = p.shape
    rank = ranks(p)
    if kind == "lac":
        return 1.0 - p, rank
    order = np.argsort(rank, axis=1)                                   # the class at rank j + 1
    u = row_u(seed, row0 + np.arange(N)) if randomized else np.ones(N)
    out = np.empty_like(p)
    above = np.zeros(N)
    rows = np.arange(N)
    for j in range(C):
        c = order[:, j]
        pc = p[rows, c]
        s = above + u * pc
        if kind == "raps":
            s = s + lam * float(max(0, j + 1 - k_reg))
        out[rows, c] = s
        above = above + pc
    return out, rank


# --------------------------------------------------------------------------------------------------------- the split
def cal_counts(labels, C, n_cal):
    """int [C]: floor(n_cal n_c / N) each, one more for the classes with the largest remainder (a tie: the lower class)"""
    n = np.bincount(labels, minlength=C).astype(np.int64)
    N = int(n.sum())
    base, rem = (n_cal * n) // N, (n_cal * n) % N
    extra = n_cal - int(base.sum())
    for c in sorted(range(C), key=lambda c: (-int(rem[c]), c))[:extra]:
        base[c] += 1
    return base


def split(seed, r, labels, C, n_cal, stratified=False):
    """bool [N]: the calibration rows of replicate r"""
    labels = np.asarray(labels)
    N = len(labels)
    cal = np.zeros(N, dtype=bool)
    groups = [(np.arange(N), n_cal)]
    if stratified:
        take = cal_counts(labels, C, n_cal)
        groups = [(np.flatnonzero(labels == c), int(take[c])) for c in range(C)]
    u = None if r == 0 else (row_hash(seed, r, np.arange(N)) >> np.uint64(32))
    for rows, take in groups:
        if r == 0:
            cal[rows[:take]] = True                                    # the identity order
        else:
            keys = (u[rows] << np.uint64(16)) | rows.astype(np.uint64)
            cal[rows[np.argsort(keys, kind="stable")[:take]]] = True
    return cal


# --------------------------------------------------------------------------------------------------------- the threshold
def quantile_index(n, alpha):
    """the 1-based index of the conformal quantile among n calibration scores, or None for +inf"""
    k = math.ceil((n + 1) * (1.0 - alpha))
    return None if k > n else int(k)


def quantile(values, alpha):
    k = quantile_index(len(values), alpha)
    return math.inf if k is None else float(np.sort(np.asarray(values, dtype=np.float64))[k - 1])


def thresholds(score, labels, cal, alpha, mondrian=False):
    """fp64 [C]: qhat (the same value C times unless mondrian)"""
    C = score.shape[1]
    true = score[np.arange(len(labels)), labels]
    if not mondrian:
        return np.full(C, quantile(true[cal], alpha))
    return np.array([quantile(true[cal & (labels == c)], alpha) for c in range(C)])


# --------------------------------------------------------------------------------------------------------- sets and counts
def sets(score, qhat):
    """bool [N, C]"""
    return score <= np.asarray(qhat)[None, :]


def mask_of(member):
    C = member.shape[1]
    return (member.astype(np.uint64) << np.arange(C, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def counts(member, labels, test):
    """int64 [8 + 5 C]: the layout of mmskin_conformal_study"""
    C = member.shape[1]
    m, y = member[test], labels[test]
    size = m.sum(axis=1)
    covered = m[np.arange(len(y)), y]
    hist = np.bincount(size, minlength=C + 1)
    size_cov = np.bincount(size[covered], minlength=C + 1)
    head = [len(y), int(covered.sum()), int(size.sum()), hist[0], hist[1], size_cov[1]]
    return np.concatenate([head, hist, size_cov, np.bincount(y, minlength=C), np.bincount(y[covered], minlength=C), m.sum(axis=0)]).astype(np.int64)


def metrics(cnt, qhat):
    """float64 [6 + 2 C] from one replicate's integers: the columns of mmskin_conformal_finalize"""
    C = len(qhat)
    n, cov, total, empty, single, single_hit = (int(v) for v in cnt[:6])
    rows, hit = cnt[6 + 2 * (C + 1):6 + 2 * (C + 1) + C], cnt[6 + 2 * (C + 1) + C:6 + 2 * (C + 1) + 2 * C]
    with np.errstate(invalid="ignore", divide="ignore"):
        per_class = np.where(rows > 0, hit / rows, np.nan)
    head = [cov / n, total / n, single / n, single_hit / single if single else np.nan, empty / n,
            np.nanmin(per_class) if (rows > 0).any() else np.nan] if n else [np.nan] * 6
    return np.concatenate([head, per_class, qhat])


def study(probs, labels, kind, alpha, n_cal, R, seed=0, randomized=False, lam=0.0, k_reg=0, mondrian=False, stratified=False, r0=0):
    """(qhat fp64 [R, C], counts int64 [R, 8 + 5 C]) of replicates r0 .. r0 + R"""
    labels = np.asarray(labels)
    score, _ = scores(probs, kind, randomized, seed, lam, k_reg)
    C = score.shape[1]
    qs, cs = [], []
    for r in range(r0, r0 + R):
        cal = split(seed, r, labels, C, n_cal, stratified)
        q = thresholds(score, labels, cal, alpha, mondrian)
        qs.append(q)
        cs.append(counts(sets(score, q), labels, ~cal))
    return np.array(qs), np.array(cs)


# --------------------------------------------------------------------------------------------------------- the guarantee
GUARANTEE = dict(N=1000, C=6, R=64, n_cal=500, alpha=0.1, seed=11)             # the guarantee tests, CPU and GPU
GUARANTEE_CASES = (("lac", False), ("aps", True), ("aps", False), ("raps", True))


def coverage_margin(n_cal, n_test, R, alpha, z=4.0):
    """z standard deviations of the mean coverage over R splits.  With distinct scores the coverage of a split depends on the ranks of
    the N true-label scores only, so the R splits of one fold are draws from one distribution whose mean is exactly k / (n_cal + 1),
    k = ceil((n_cal + 1)(1 - alpha)).  Given the calibration set the coverage probability is Beta(k, n_cal + 1 - k) distributed
    (variance a b / ((a + b)^2 (a + b + 1))), and the n_test test rows add the binomial mu (1 - mu) / n_test; sampling without
    replacement from a finite fold only shrinks both.  The mean of R splits has that variance over R; z = 4 leaves 6e-5."""
    a = math.ceil((n_cal + 1) * (1.0 - alpha))
    b = n_cal + 1 - a
    mu = a / (a + b)
    var = a * b / ((a + b) ** 2 * (a + b + 1)) + mu * (1.0 - mu) / n_test
    return z * math.sqrt(var / R)


# --------------------------------------------------------------------------------------------------------- folds
def fold(N, C, kind="dyadic", seed=0):
    """(probs fp32 [N, C], labels int64 [N]).  "dyadic": small integers over 64 that sum to one, so every prefix sum is exact, with
    ties and exact zeros, a one-hot row and an all-equal row.  "softmax": ordinary soft-max rows, labels drawn from them."""
    rng = np.random.default_rng(seed)
    if kind == "dyadic":
        cuts = np.sort(rng.integers(0, 65, size=(N, C - 1)), axis=1)
        parts = np.diff(np.concatenate([np.zeros((N, 1), dtype=np.int64), cuts, np.full((N, 1), 64)], axis=1), axis=1)
        parts[1] = 0
        parts[1, C // 2] = 64                                          # a one-hot row: C - 1 exact zeros, all tied
        probs = (parts / 64.0).astype(np.float32)
        probs[0] = np.float32(1.0 / C)                                 # an all-equal row (its sums round, the same way on both sides)
        labels = rng.integers(0, C, size=N)
        labels[:C] = np.arange(C) % C
    else:
        z = rng.normal(size=(N, C)) * 2.0
        e = np.exp(z - z.max(axis=1, keepdims=True))
        probs = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
        labels = (rng.random(N)[:, None] > np.cumsum(probs.astype(np.float64), axis=1)).sum(axis=1).clip(0, C - 1)
    return probs, labels.astype(np.int64)
