"""float64 restatement of the three criteria of csrc/criterion.hip and of their gradients (numpy).

tests/test_cpu_criterion.py pins it to tests/golden/criterion.json, which holds what torch's CrossEntropyLoss and the
reference's own FocalLoss / SoftTargetCrossEntropy classes gave in float64; tests/test_gpu_criterion.py holds the kernels to it.
A label outside [0, C) is ignored: no loss, no gradient, not counted in cross-entropy's weighted mean."""
import numpy as np

GOLDEN_SHAPES = [(3, 2), (7, 6), (5, 9)]
GOLDEN_GAMMAS = [0.0, 1.5, 2.0]


def golden_inputs(B, C):
    """the seeded inputs of one fixture shape (the generator and the tests build them the same way; the fixture records them too)"""
    rng = np.random.default_rng(1000 * B + C)
    return {"logits": rng.normal(0.0, 3.0, (B, C)), "labels": rng.integers(0, C, B), "weight": rng.uniform(0.3, 3.0, C),
            "soft": rng.dirichlet(np.ones(C), B), "upstream": rng.normal(0.0, 1.0, B)}


def log_softmax(z):
    z = np.asarray(z, dtype=np.float64)
    shifted = z - z.max(axis=1, keepdims=True)
    return shifted - np.log(np.exp(shifted).sum(axis=1, keepdims=True))


def softmax(z):
    return np.exp(log_softmax(z))


def hard(z, y, w=None, kind="ce", reduction="mean", gamma=0.0, upstream=None, alpha_last=False):
    """-> (loss, dlogits).  kind "ce": w[y] ce, `mean` divides by the valid rows' weights.  kind "focal": (1 - pt)^gamma (w[y] ce),
    pt = exp(-ce), `mean` divides by B; alpha_last multiplies by w[y] AFTER the modulating factor (train_milk10K.py:84-98), which
    differs in the last bit only.  upstream: d(final scalar) / d(loss), a scalar, or [B] for reduction "none" (default ones)."""
    z = np.asarray(z, dtype=np.float64)
    y = np.asarray(y, dtype=np.int64)
    B, C = z.shape
    lsm = log_softmax(z)
    valid = (y >= 0) & (y < C)
    ys = np.where(valid, y, 0)
    ce = np.where(valid, -lsm[np.arange(B), ys], 0.0)
    wy = np.where(valid, 1.0 if w is None else np.asarray(w, dtype=np.float64)[ys], 0.0)
    if kind == "focal" and gamma != 0:
        omp = -np.expm1(-ce)
        rows = wy * (omp ** gamma * ce) if alpha_last else omp ** gamma * (wy * ce)
        slope = wy * (gamma * omp ** (gamma - 1) * np.exp(-ce) * ce + omp ** gamma)
    else:
        rows, slope = wy * ce, wy
    onehot = np.zeros((B, C))
    onehot[np.arange(B), ys] = 1.0
    drows = np.where(valid, slope, 0.0)[:, None] * (np.exp(lsm) - onehot)           # d rows_i / d z_ij
    if reduction == "none":
        up = np.ones(B) if upstream is None else np.asarray(upstream, dtype=np.float64)
        return rows, up[:, None] * drows
    up = 1.0 if upstream is None else float(upstream)
    if reduction == "sum":
        return rows.sum(), up * drows
    denom = wy.sum() if kind == "ce" else float(B)
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = rows.sum() / denom
        dz = np.where(valid[:, None], up / denom * drows, 0.0)
    return loss, dz


def soft(z, t, w=None, upstream=1.0):
    """-> (loss, dlogits) of mean_i -sum_c t[i, c] log_softmax(z)[i, c] w[c]"""
    z, t = np.asarray(z, dtype=np.float64), np.asarray(t, dtype=np.float64)
    B = z.shape[0]
    tw = t if w is None else t * np.asarray(w, dtype=np.float64)[None, :]
    lsm = log_softmax(z)
    return -(tw * lsm).sum() / B, float(upstream) / B * (np.exp(lsm) * tw.sum(axis=1, keepdims=True) - tw)


def case_key(kind, reduction, weighted, gamma=0.0):
    return f"{kind}|{reduction}|{'w' if weighted else '-'}|{gamma:g}"


def golden_cases():
    """every (kind, reduction, weighted, gamma) the fixture records per shape"""
    out = [("ce", r, wt, 0.0) for r in ("none", "sum", "mean") for wt in (False, True)]
    out += [("focal", r, wt, g) for g in GOLDEN_GAMMAS for r in ("none", "sum", "mean") for wt in (False, True)]
    out += [("soft", "mean", wt, 0.0) for wt in (False, True)]
    return out


def run_case(inp, kind, reduction, weighted, gamma, **kw):
    """the oracle on the inputs of golden_inputs(): `none` is weighted by the recorded upstream vector"""
    w = inp["weight"] if weighted else None
    if kind == "soft":
        return soft(inp["logits"], inp["soft"], w)
    return hard(inp["logits"], inp["labels"], w, kind, reduction, gamma, upstream=inp["upstream"] if reduction == "none" else None, **kw)
