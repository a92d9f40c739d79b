"""numpy restatement of the metadata-sweep kernels (csrc/sweep.hip) and the shared inputs of their tests.

`variants` and `reduce` state in numpy fp32 what the two kernels compute; tests/test_cpu_sweep.py holds them to sklearn / pandas
semantics and to float64 formulas, tests/test_gpu_sweep.py holds the kernels to them.  `reduce64` is the float64 statement of
the same quantities, row by row, in the form of the reference's helper functions (analyze_prediction_uncertainty.py:166-189,
flip_rate.py:251-254).  `e2e_case` / `oracle_loop` are the end-to-end inputs and the reference's loop (batch-1 forwards, one
per variant) on the CPU oracle model.
"""
import numpy as np
import torch

NONE, CAT_SET, CAT_TOGGLE, NUM_ADD, NUM_SET = 0, 1, 2, 3, 4
VARIANT_DTYPE = np.dtype([("op", "<i4"), ("column", "<i4"), ("a", "<i4"), ("b", "<i4"), ("value", "<f4"), ("reserved", "<u4", (3,))])

# fp32 logits tolerance of the project for the small custom-cnn model (tests/test_gpu_model.py::test_mechanism_matches_
# reference_golden through helpers.check_record_against_golden): |got - want| <= ATOL + RTOL * |want|
LOGIT_RTOL, LOGIT_ATOL = 1e-3, 1e-5


def record(op=NONE, column=0, a=0, b=0, value=0.0):
    r = np.zeros((), dtype=VARIANT_DTYPE)
    r["op"], r["column"], r["a"], r["b"], r["value"] = op, column, a, b, value
    return r


def table(records):
    return np.array(records, dtype=VARIANT_DTYPE)


def variants(codes, numeric, col_offset, mean, scale, nan_fill, tab, out_width, mask=None, missing_code=None):
    """codes int32 [B, n_cat], numeric fp32 [B, n_num] (NaN = missing), col_offset int [n_cat + 1], mean / scale fp32 [n_num],
    tab VARIANT_DTYPE [V], mask uint8 [V, B, n_cat + n_num] or None, missing_code int [n_cat] -> fp32 [V, B, out_width]"""
    codes, numeric = np.asarray(codes, dtype=np.int32), np.asarray(numeric, dtype=np.float32)
    mean, scale = np.asarray(mean, dtype=np.float32), np.asarray(scale, dtype=np.float32)
    B, n_cat = codes.shape
    n_num = numeric.shape[1]
    onehot = int(col_offset[-1])
    width = onehot + n_num
    out = np.zeros((len(tab), B, max(width, out_width)), dtype=np.float32)
    for v, r in enumerate(tab):
        c, x = codes.copy(), numeric.copy()
        op, col = int(r["op"]), int(r["column"])
        if op == CAT_SET:
            c[:, col] = r["a"]
        elif op == CAT_TOGGLE:
            c[:, col] = np.where(c[:, col] == r["a"], r["b"], r["a"])
        elif op == NUM_ADD:
            x[:, col - n_cat] = x[:, col - n_cat] + np.float32(r["value"])
        elif op == NUM_SET:
            x[:, col - n_cat] = np.float32(r["value"])
        if mask is not None:
            blank = np.asarray(mask[v]).astype(bool)
            for j in range(n_cat):
                c[blank[:, j], j] = missing_code[j]
            x[blank[:, n_cat:]] = np.nan
        x = np.where(np.isnan(x), np.float32(nan_fill), x).astype(np.float32)
        for j in range(n_cat):
            hit = c[:, j] >= 0
            out[v, np.nonzero(hit)[0], col_offset[j] + c[hit, j]] = 1.0
        out[v, :, onehot:width] = (x - mean) / scale
    return np.ascontiguousarray(out[:, :, :out_width])


def _row_quantities(x, dt):
    """x [..., C] logits -> soft-max p, safe probabilities q, first arg-max, top-1 minus top-2; arithmetic in dtype dt"""
    x = x.astype(dt)
    top = x.max(axis=-1, keepdims=True)
    e = np.exp(x - top)
    p = e / e.sum(axis=-1, keepdims=True)
    q = np.clip(p, dt(1e-12), dt(1.0))
    q = q / q.sum(axis=-1, keepdims=True)
    pred = x.argmax(axis=-1)                                     # numpy: the first index of the maximum
    second = np.where(np.arange(x.shape[-1]) == pred[..., None], -np.inf, x).max(axis=-1)
    return p, q, pred.astype(np.int32), (top[..., 0] - second).astype(dt)


def reduce(logits, base, labels=None, dt=np.float32):
    """logits [V, B, C] and base [B, C] (fp32 values) -> dict of probs, pred, margin, stats [V, B, 4], flips [V], transitions
    [V, C, C], confusion [V, C, C] (with labels).  dt = np.float64 gives the same quantities in double precision."""
    logits, base = np.asarray(logits, dtype=np.float32), np.asarray(base, dtype=np.float32)
    V, B, C = logits.shape
    p, q, pred, margin = _row_quantities(logits, dt)
    _, qb, bpred, _ = _row_quantities(base, dt)
    qb = np.broadcast_to(qb, q.shape)
    m = dt(0.5) * (q + qb)
    ent = -(q * np.log(q)).sum(axis=-1)
    kl = (q * np.log(q / qb)).sum(axis=-1)
    js = dt(0.5) * (q * np.log(q / m)).sum(axis=-1) + dt(0.5) * (qb * np.log(qb / m)).sum(axis=-1)
    rows = np.arange(B)
    dconf = q[:, rows, bpred] - qb[:, rows, bpred]
    out = dict(probs=p, pred=pred, margin=margin, stats=np.stack([ent, kl, js, dconf], axis=-1).astype(dt),
               flips=(pred != bpred[None]).sum(axis=1).astype(np.int32), transitions=np.zeros((V, C, C), dtype=np.int32), confusion=None)
    for v in range(V):
        np.add.at(out["transitions"][v], (bpred, pred[v]), 1)
    if labels is not None:
        labels = np.asarray(labels)
        ok = (labels >= 0) & (labels < C)                        # a label outside [0, C) counts nowhere
        out["confusion"] = np.zeros((V, C, C), dtype=np.int32)
        for v in range(V):
            np.add.at(out["confusion"][v], (labels[ok], pred[v][ok]), 1)
    return out


# ---- the float64 formulas, one row at a time, in the reference's own form
def _safe_probs(p, eps=1e-12):
    p = np.clip(np.asarray(p, dtype=np.float64), eps, 1.0)
    return p / p.sum()


def _kl(p, q):
    p, q = _safe_probs(p), _safe_probs(q)
    return float(np.sum(p * np.log(p / q)))


def reduce64(logits, base, labels=None):
    logits, base = np.asarray(logits, dtype=np.float64), np.asarray(base, dtype=np.float64)
    V, B, C = logits.shape
    softmax = lambda x: np.exp(x - x.max()) / np.exp(x - x.max()).sum()
    out = dict(probs=np.zeros((V, B, C)), pred=np.zeros((V, B), dtype=np.int32), margin=np.zeros((V, B)), stats=np.zeros((V, B, 4)),
               flips=np.zeros(V, dtype=np.int32), transitions=np.zeros((V, C, C), dtype=np.int32),
               confusion=None if labels is None else np.zeros((V, C, C), dtype=np.int32))
    for b in range(B):
        pb = softmax(base[b])
        c0 = int(np.argmax(base[b]))
        for v in range(V):
            p = softmax(logits[v, b])
            c1 = int(np.argmax(logits[v, b]))
            srt = np.sort(logits[v, b])
            sp, sb = _safe_probs(p), _safe_probs(pb)
            m = 0.5 * (sp + sb)
            out["probs"][v, b], out["pred"][v, b], out["margin"][v, b] = p, c1, srt[-1] - srt[-2]
            out["stats"][v, b] = (-np.sum(sp * np.log(sp)), _kl(p, pb), 0.5 * _kl(sp, m) + 0.5 * _kl(sb, m), sp[c0] - sb[c0])
            out["transitions"][v, c0, c1] += 1
            out["flips"][v] += c1 != c0
            if labels is not None and 0 <= labels[b] < C:
                out["confusion"][v, labels[b], c1] += 1
    return out


# ---- shared inputs of the reduce tests
REDUCE_SHAPES = [(V, B, C) for V in (1, 3, 16) for B in (1, 63, 64, 65, 300) for C in (2, 6, 7, 64)]
ROWWISE_SHAPES = [(1, 1, 2), (3, 63, 6), (16, 64, 7), (3, 65, 64), (16, 1, 6), (1, 300, 64), (3, 64, 2)]      # for the row-by-row float64 loop


def reduce_case(V, B, C, seed=0):
    """logits [V, B, C], base [B, C], labels [B] with planted structure: variant 0 IS the baseline (zero KL / JS, no flip); row 0
    of every variant has an exact tie between its two largest logits (the first index must win); the last variant's last row
    equals its baseline; one label is out of range (skipped in the confusion matrix only); spreads from 0.5 to 12 so that
    probabilities below the 1e-12 clip occur."""
    rng = np.random.default_rng(1000 * V + 10 * B + C + seed)
    base = (rng.standard_normal((B, C)) * rng.uniform(0.5, 12.0, (B, 1))).astype(np.float32)
    logits = (base[None] + rng.standard_normal((V, B, C)) * rng.uniform(0.0, 3.0, (V, B, 1))).astype(np.float32)
    logits[0] = base
    for v in range(1, V):
        hi = logits[v, 0].max() + np.float32(0.25)
        a, b = sorted(rng.choice(C, 2, replace=False))
        logits[v, 0, a] = logits[v, 0, b] = hi
    if V > 1:
        logits[-1, B - 1] = base[B - 1]
    if B > 1:
        base[1, :2] = base[1].max() + np.float32(1.0)           # a tie in a baseline row
        logits[0, 1] = base[1]
    labels = rng.integers(0, C, B).astype(np.int32)
    if B > 2:
        labels[2] = C + 3
    return logits, base, labels


CONTINUOUS = ("probs", "stats")


def continuous_errors(got, want64):
    """max |got - want64| of the soft-max and of each of the four statistics"""
    err = {"probs": float(np.abs(got["probs"].astype(np.float64) - want64["probs"]).max())}
    for i, name in enumerate(("entropy", "kl", "js", "dconf")):
        err[name] = float(np.abs(got["stats"][..., i].astype(np.float64) - want64["stats"][..., i]).max())
    return err


# ---- end to end
E2E_CATEGORIES = [["EMPTY", "False", "True"], ["EMPTY", "False", "True"], ["FEMALE", "MALE"], ["ARM", "EMPTY", "FACE", "FOREARM"],
                  ["False", "True", "UNK"]]                                  # sorted, as OneHotEncoder fits them; 15 one-hot slots
E2E_CAT_NAMES = ["itch", "grew", "gender", "region", "bleed"]
E2E_NUM_NAMES = ["age", "diameter_1", "diameter_2"]
E2E_MEAN, E2E_SCALE = np.array([55.0, 9.0, 7.0]), np.array([4.0, 1.5, 1.25])
E2E_FLIPS = [("itch", ("toggle", "True", "False")), ("gender", ("toggle", "FEMALE", "MALE")), ("region", ("toggle", "FACE", "FOREARM")),
             ("region", ("set", "SCALP")), ("itch", ("set", "EMPTY")), ("bleed", ("set", "UNK")), ("age", ("set", 80.0)),
             ("age", ("add", -30.0)), ("diameter_1", ("add", 5.0)), ("diameter_2", ("add", 5.0)), ("diameter_1", ("set", 1.0)),
             ("diameter_2", ("set", 30.0)), ("age", ("set", 20.0)), ("age", ("add", 25.0)), ("diameter_1", ("set", 25.0)),
             ("diameter_2", ("add", -6.0))]                                  # 16 mutations + the baseline = 17 head evaluations
E2E_SALT = 1        # oracle.detinit salt of the weights: one at which the random-init heads react to the metadata (test_cpu_sweep.py)
E2E_RATES, E2E_SEEDS = [0.1, 0.5, 0.9], [100, 500, 900]
E2E_MECHS = ["gfcam", "concatenation", "metablock", "att-intramodal+residual+cross-attention-metadados"]
E2E_BATCHES = [(0, 5), (5, 8)]                                               # a batch of 5, then one of 3


def e2e_encoder():
    from mmskin.preprocess import MetadataEncoder
    enc = MetadataEncoder()
    enc.categories_ = [np.array(c, dtype=object) for c in E2E_CATEGORIES]
    enc.mean_, enc.scale_ = E2E_MEAN.copy(), E2E_SCALE.copy()
    return enc


def e2e_case():
    """8 rows: images [8, 3, 32, 32], categorical strings [8, 5], numerics [8, 3] with gaps"""
    from oracle.detinit import det_inputs
    rng = np.random.default_rng(7)
    img = det_inputs(8, 32, 20, 6)[0]
    cats = np.stack([rng.choice(c + (["SCALP"] if i == 3 else []), 8) for i, c in enumerate(E2E_CATEGORIES)], axis=1).astype(object)
    num = np.stack([rng.integers(20, 90, 8).astype(float), rng.uniform(2, 16, 8), rng.uniform(2, 12, 8)], axis=1)
    num[1, 1] = num[4, 0] = num[6, 2] = np.nan
    return img, cats, num


def oracle_loop(model, images, metas):
    """the reference's loop: one batch-1 forward per (row, variant); metas fp32 [V, B, W] -> logits fp32 [V, B, C]"""
    V, B = metas.shape[:2]
    out = []
    with torch.no_grad():
        for v in range(V):
            out.append(torch.cat([model(images[b:b + 1], torch.from_numpy(metas[v, b:b + 1])) for b in range(B)], dim=0))
    return torch.stack(out).float().numpy()


def margin_threshold(logits):
    """twice the project's fp32 logits tolerance at the row's largest logit: below it, the HIP model may rank the top two the
    other way round"""
    return 2.0 * (LOGIT_ATOL + LOGIT_RTOL * np.abs(logits).max(axis=-1))
