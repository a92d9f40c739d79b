"""numpy float64 restatement of mmskin.lime / csrc/lime.hip: the counter-based normal generator, the neighbourhood rows and their
kernel weights, the soft-max as the kernel takes it, and lime's explain_instance for mode="regression",
discretize_continuous=False, feature_selection "highest_weights": sklearn's Ridge with sample weights in closed form.
tests/test_cpu_lime.py holds this file to sklearn and to literal transcriptions; tests/test_gpu_lime.py holds the kernels to it."""
import numpy as np

PROB, LOGIT = 0, 1
ALPHA_SELECT, ALPHA_FIT = 0.01, 1.0
MAX_FEATURES = 128
U64 = np.uint64


# ------------------------------------------------------------------------------------------- generator
def mix64(x):
    """the splitmix64 finaliser of csrc/common.h on a uint64 array (wrapping arithmetic)"""
    x = np.asarray(x, dtype=U64)
    with np.errstate(over="ignore"):
        x = x + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
    return x ^ (x >> U64(31))


def uniforms(seed, sample, s, f):
    """(u1, u2) float64, each an odd multiple of 2^-24 inside (0, 1) -- exact in float32 too -- for the broadcast of the counters"""
    sample, s, f = (np.asarray(a, dtype=U64) for a in (sample, s, f))
    key = mix64(np.array([seed & (2 ** 64 - 1)], dtype=U64))[0]
    h = mix64(key ^ ((sample << U64(40)) | (s << U64(8)) | f))
    hi, lo = h >> U64(32), h & U64(0xFFFFFFFF)
    return ((hi >> U64(9)).astype(np.float64) + 0.5) * 2.0 ** -23, ((lo >> U64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normals(seed, sample, s, f, dt=np.float64):
    """Box-Muller on the two uniforms, every operation in dt (float32: the kernel's formula)"""
    u1, u2 = (u.astype(dt) for u in uniforms(seed, sample, s, f))
    two_pi = dt(np.float32(6.2831855)) if dt == np.float32 else dt(2.0 * np.pi)
    return (np.sqrt(dt(-2.0) * np.log(u1)) * np.cos(two_pi * u2)).astype(dt)


# ------------------------------------------------------------------------------------------- scaler, rows, weights
def fit_scaler(rows):
    """sklearn's StandardScaler: mean and population deviation, 0 replaced by 1"""
    rows = np.asarray(rows, dtype=np.float64)
    mean, scale = rows.mean(axis=0), rows.std(axis=0)
    scale[scale == 0.0] = 1.0
    return mean, scale


def neighbourhood(x, mean, scale, N, seed, sample0=0, around=False, out_width=None, dt=np.float32):
    """rows [B, N, out_width]: row 0 = x, row s = n * scale + centre.  dt float32: the device's rows bit for bit up to its log / cos;
    float64: the same draws with nothing rounded"""
    x = np.asarray(x, dtype=np.float32)
    B, F = x.shape
    b, s, f = np.meshgrid(np.arange(B), np.arange(N), np.arange(F), indexing="ij")
    n = normals(seed, sample0 + b, s, f, dt)
    centre = x[:, None, :].astype(dt) if around else np.broadcast_to(np.asarray(mean).astype(dt), (B, N, F))
    rows = (n * np.asarray(scale).astype(dt)).astype(dt) + centre
    rows = rows.astype(dt)
    rows[:, 0, :] = x
    width = F if out_width is None else out_width
    out = np.zeros((B, N, width), dtype=dt)
    out[..., :F] = rows
    return out


def standardise(rows, mean, scale):
    F = len(mean)
    return (np.asarray(rows)[..., :F].astype(np.float64) - mean) / scale


def kernel_weights(rows, mean, scale):
    """rows [B, N, >= F] -> w float64 [B, N] = sqrt(exp(-d^2 / kernel_width^2)), d the distance to row 0 in standardised space"""
    z = standardise(rows, mean, scale)
    d2 = ((z - z[:, :1]) ** 2).sum(-1)
    return np.sqrt(np.exp(-d2 / (0.75 * np.sqrt(len(mean))) ** 2))


def softmax32(logits):
    """the kernel's soft-max: x - max in float32, exp in float64 rounded to float32, the sum over c = 0 .. C-1 in float32, e / sum"""
    x = np.asarray(logits, dtype=np.float32)
    e = np.exp((x - x.max(-1, keepdims=True)).astype(np.float64)).astype(np.float32)
    total = np.zeros(x.shape[:-1], dtype=np.float32)
    for c in range(x.shape[-1]):
        total = (total + e[..., c]).astype(np.float32)
    return (e / total[..., None]).astype(np.float32)


def targets(logits, output):
    return (softmax32(logits) if output == PROB else np.asarray(logits, dtype=np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------- ridge
def centred_sums(z, y, w):
    """z [N, F], y [N], w [N] -> (zbar, ybar, G = Zc^T W Zc, R = Zc^T W yc, Syy)"""
    W = w.sum()
    zbar, ybar = (w[:, None] * z).sum(0) / W, (w * y).sum() / W
    zc, yc = z - zbar, y - ybar
    return zbar, ybar, zc.T @ (w[:, None] * zc), zc.T @ (w * yc), (w * yc * yc).sum()


def ridge_fit(z, y, w, alpha, keep=None):
    """Ridge(alpha, fit_intercept=True).fit(z[:, keep], y, sample_weight=w) in closed form -> (coef, intercept, score)"""
    keep = np.arange(z.shape[1]) if keep is None else np.asarray(keep)
    zbar, ybar, G, R, syy = centred_sums(z[:, keep], y, w)
    beta = np.linalg.solve(G + alpha * np.eye(len(keep)), R)
    rss = syy - 2.0 * beta @ R + beta @ G @ beta
    score = 1.0 - rss / syy if syy > 0 else (1.0 if rss == 0 else 0.0)
    return beta, ybar - zbar @ beta, score


def select(beta0, z0, K):
    """(the K features with the largest |beta0 z0|, ties to the lower index, ascending; the relative gap between the K-th and the
    (K+1)-th value, inf when all are kept)"""
    v = np.abs(beta0 * z0)
    order = np.argsort(-v, kind="stable")
    gap = np.inf if K >= len(v) else (v[order[K - 1]] - v[order[K]]) / max(v[order[K - 1]], 1e-300)
    return np.sort(order[:K]), gap


def explain(z, y, w, K, alpha_select=ALPHA_SELECT, alpha_fit=ALPHA_FIT):
    """one sample: z [N, F] (row 0 the explained one), y [N, C], w [N] -> dict of feature / coef [C, K] in descending |coef|,
    intercept, score, local_pred [C], dense [C, F], gap [C]"""
    (N, F), C = z.shape, y.shape[1]
    K = min(K, F)
    out = dict(feature=np.zeros((C, K), dtype=np.int32), coef=np.zeros((C, K)), intercept=np.zeros(C), score=np.zeros(C),
               local_pred=np.zeros(C), dense=np.zeros((C, F)), gap=np.zeros(C))
    for c in range(C):
        beta0, _, _ = ridge_fit(z, y[:, c], w, alpha_select)
        keep, out["gap"][c] = select(beta0, z[0], K)
        beta, icpt, score = ridge_fit(z, y[:, c], w, alpha_fit, keep)
        order = np.argsort(-np.abs(beta), kind="stable")
        out["feature"][c], out["coef"][c] = keep[order], beta[order]
        out["intercept"][c], out["score"][c], out["local_pred"][c] = icpt, score, icpt + z[0, keep] @ beta
        out["dense"][c, keep] = beta
    return out


def explain_batch(rows, logits, mean, scale, K, output):
    """rows [B, N, >= F] (the device's own), logits [B, N, C] -> the per-sample dicts stacked on a leading B axis"""
    z, w, y = standardise(rows, mean, scale), kernel_weights(rows, mean, scale), targets(logits, output)
    per = [explain(z[b], y[b], w[b], K) for b in range(z.shape[0])]
    return {k: np.stack([p[k] for p in per]) for k in per[0]}


# ------------------------------------------------------------------------------------------- the GPU tests' cases
def case_stats(F, seed):
    """(mean, scale, x fp32 [3, F]) like an encoder's columns, F >= 3: one-hot cells (mean p, deviation sqrt(p (1 - p))), then three
    standardised numerics"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.05, 0.95, F)
    mean, scale = p.copy(), np.sqrt(p * (1 - p))
    mean[-3:], scale[-3:] = rng.normal(0, 0.01, 3), 1.0
    x = (rng.random((3, F)) < p).astype(np.float32)
    x[:, -3:] = rng.normal(0, 1, (3, 3)).astype(np.float32)
    return mean, scale, x
