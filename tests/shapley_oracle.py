"""numpy restatement of the metadata-Shapley kernels (csrc/shapley.hip) and of mmskin.shapley.MetadataShapley, sharing nothing
with either, and the shared inputs of their tests.

The estimator: players are the M = n_cat + n_num metadata COLUMNS (categorical first); v(S) is the mean over G background rows
of out(model(image, mix(x, b_g, S))); P permutations are each walked from both ends,
    phi_j = (1/2P) sum_p [ v(S_{q+1}) - v(S_q) + v(T_{M-q}) - v(T_{M-q-1}) ],   q = position of j in pi_p,
S_n = the first n entries of pi_p, T_n = its last n.

`walk_masks` / `row_plan` state the row order, `coalition_rows` the encoded rows (through sweep_oracle.variants, the encoder the
sweep tests hold to sklearn), `reduce` what the reduce kernels compute from logits, `values` the walk on any value function,
`exact` brute-force Shapley values over all 2^M coalitions, `oracle_loop` the end-to-end loop on the CPU oracle model.
"""
import itertools
import math

import numpy as np
import torch

import sweep_oracle as so

PROB, LOGIT = 0, 1


def mix(x_codes, x_num, b_codes, b_num, mask):
    """one explained row and one background row -> the raw row of coalition `mask` (bool [M], True = the column is x's)"""
    n_cat = len(x_codes)
    mask = np.asarray(mask, dtype=bool)
    return np.where(mask[:n_cat], x_codes, b_codes).astype(np.int32), np.where(mask[n_cat:], x_num, b_num).astype(np.float32)


def walk_masks(perms):
    """bool [K + 2, M] for int perms [P, M]: the K = 2 P (M - 1) interior coalitions in the order (permutation, walk side, step) --
    side 0 takes the first n entries of the permutation, side 1 its last n, n = 1 .. M - 1 -- then the empty coalition (index K),
    then all columns (index K + 1)"""
    perms = np.asarray(perms)
    P, M = perms.shape
    masks = []
    for p in range(P):
        for side in (0, 1):
            for n in range(1, M):
                m = np.zeros(M, dtype=bool)
                m[perms[p, :n] if side == 0 else perms[p, M - n:]] = True
                masks.append(m)
    masks.append(np.zeros(M, dtype=bool))
    masks.append(np.ones(M, dtype=bool))
    return np.array(masks).reshape(-1, M)


def n_rows(B, G, P, M):
    return B * (1 + G + P * 2 * (M - 1) * G)


def row_plan(B, G, P, M):
    """(sample, coalition, background row) of every row of a batch's walk: first (b, k, g) for b < B, k <= K, g < G with g the
    fastest index, then B rows (b, K + 1, 0), the explained rows themselves"""
    K = 2 * P * (M - 1)
    plan = [(b, k, g) for b in range(B) for k in range(K + 1) for g in range(G)] + [(b, K + 1, 0) for b in range(B)]
    assert len(plan) == n_rows(B, G, P, M)
    return plan


def coalition_rows(codes, numeric, bg_codes, bg_numeric, col_offset, mean, scale, nan_fill, perms, out_width):
    """the encoded metadata rows fp32 [n_rows, out_width] of the whole walk: every row is the encoding of the mixed raw row"""
    codes, numeric = np.asarray(codes, dtype=np.int32), np.asarray(numeric, dtype=np.float32)
    bg_codes, bg_numeric = np.asarray(bg_codes, dtype=np.int32), np.asarray(bg_numeric, dtype=np.float32)
    masks = walk_masks(perms)
    P, M = np.asarray(perms).shape
    plan = row_plan(len(codes), len(bg_codes), P, M)
    raw = [mix(codes[b], numeric[b], bg_codes[g], bg_numeric[g], masks[k]) for b, k, g in plan]
    raw_codes = np.stack([r[0] for r in raw]).reshape(len(plan), codes.shape[1])
    raw_num = np.stack([r[1] for r in raw]).reshape(len(plan), numeric.shape[1])
    return so.variants(raw_codes, raw_num, col_offset, mean, scale, nan_fill, so.table([so.record()]), out_width)[0]


def _out(logits, output, dt):
    x = logits.astype(dt)
    if output == LOGIT:
        return x
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def phi_from_v(v, perms):
    """v [B, K + 2, C] (walk_masks order) -> phi float64 [B, M, C], the four-term marginals summed over p in order"""
    perms = np.asarray(perms)
    P, M = perms.shape
    K = 2 * P * (M - 1)
    v = np.asarray(v, dtype=np.float64)

    def at(p, side, n):
        return v[:, K] if n == 0 else v[:, K + 1] if n == M else v[:, (p * 2 + side) * (M - 1) + n - 1]

    phi = np.zeros((v.shape[0], M, v.shape[2]))
    for j in range(M):
        for p in range(P):
            q = int(np.flatnonzero(perms[p] == j)[0])
            phi[:, j] += (at(p, 0, q + 1) - at(p, 0, q)) + (at(p, 1, M - q) - at(p, 1, M - q - 1))
    return phi / (2 * P)


def reduce(logits, B, G, perms, output=PROB, dt=np.float32):
    """logits [n_rows, C] (fp32 values) -> dict of v [B, K + 2, C], phi [B, M, C], base and full [B, C]: `out` in dtype dt, the
    means over the background and the sums over the permutations in float64, as the kernels hold them"""
    perms = np.asarray(perms)
    P, M = perms.shape
    K = 2 * P * (M - 1)
    logits = np.asarray(logits, dtype=np.float32)
    C = logits.shape[1]
    vals = _out(logits, output, dt).astype(np.float64)
    A = B * (K + 1) * G
    v = np.concatenate([vals[:A].reshape(B, K + 1, G, C).mean(axis=2), vals[A:].reshape(B, 1, C)], axis=1)
    phi = phi_from_v(v, perms)
    return dict(v=v, phi=phi.astype(dt), base=v[:, K].astype(dt), full=v[:, K + 1].astype(dt))      # the kernel's outputs are fp32


# ---- the walk and brute force on an arbitrary value function
def values(v_fn, M, perms):
    """phi float64 [M, ...] of value function v_fn(mask bool [M]) by the antithetic walk over int perms [P, M]"""
    perms = np.asarray(perms)
    P = len(perms)
    phi = None
    for p in range(P):
        for order in (perms[p], perms[p][::-1]):                 # the walk from the front, then from the back
            mask = np.zeros(M, dtype=bool)
            prev = np.asarray(v_fn(mask), dtype=np.float64)
            if phi is None:
                phi = np.zeros((M,) + prev.shape)
            for j in order:
                mask[j] = True
                cur = np.asarray(v_fn(mask), dtype=np.float64)
                phi[j] += cur - prev
                prev = cur
    return phi / (2 * P)


def exact(v_fn, M):
    """the Shapley values over all 2^M coalitions: phi_j = sum_S |S|! (M - |S| - 1)! / M! (v(S + j) - v(S))"""
    phi = None
    for j in range(M):
        rest = [i for i in range(M) if i != j]
        for size in range(M):
            w = math.factorial(size) * math.factorial(M - size - 1) / math.factorial(M)
            for S in itertools.combinations(rest, size):
                mask = np.zeros(M, dtype=bool)
                mask[list(S)] = True
                without = np.asarray(v_fn(mask), dtype=np.float64)
                mask[j] = True
                d = np.asarray(v_fn(mask), dtype=np.float64) - without
                if phi is None:
                    phi = np.zeros((M,) + d.shape)
                phi[j] += w * d
    return phi


def polynomial_value(M, order, seed, n_out=3):
    """a seeded value function on masks with constant, linear, ... up to `order`-th order interaction terms, n_out outputs"""
    rng = np.random.default_rng(seed)
    terms = [(S, rng.standard_normal(n_out)) for k in range(order + 1) for S in itertools.combinations(range(M), k)]

    def v_fn(mask):
        return sum(w for S, w in terms if all(mask[i] for i in S))
    return v_fn


# ---- shared inputs of the reduce tests
REDUCE_CASES = [(B, G, P, M, C) for (B, M) in ((1, 1), (5, 8), (2, 3)) for G in (1, 3, 33) for P in (1, 3) for C in (2, 6, 64)]


def reduce_case(B, G, P, M, C, seed=0):
    """seeded logits fp32 [n_rows, C] with spreads from 0.5 to 12 (probabilities down to the underflow of exp) and permutations"""
    rng = np.random.default_rng(10000 * B + 1000 * G + 100 * P + 10 * M + C + seed)
    N = n_rows(B, G, P, M)
    logits = (rng.standard_normal((N, C)) * rng.uniform(0.5, 12.0, (N, 1))).astype(np.float32)
    perms = np.stack([rng.permutation(M) for _ in range(P)]).astype(np.int32)
    return logits, perms


def reduce_errors(got, want64):
    """max |got - want64| of v, phi, and of the efficiency residual sum_j phi_j - (full - base) of `got` itself"""
    g = {k: np.asarray(got[k], dtype=np.float64) for k in ("phi", "base", "full")}
    return {"phi": float(np.abs(g["phi"] - want64["phi"]).max()),
            "ends": float(max(np.abs(g["base"] - want64["base"]).max(), np.abs(g["full"] - want64["full"]).max())),
            "efficiency": float(np.abs(g["phi"].sum(axis=1) - (g["full"] - g["base"])).max())}


# ---- end to end (the fixtures of sweep_oracle: SMALL models, 8 rows, 5 categorical + 3 numeric columns)
E2E_G, E2E_P, E2E_SEED = 3, 2, 11
E2E_BACKGROUND_ROWS = [6, 1, 3]          # rows of the fixture that serve as the background (row 1 and row 6 hold a NaN)


def e2e_permutations(M):
    rng = np.random.default_rng(E2E_SEED)
    return np.stack([rng.permutation(M) for _ in range(E2E_P)]).astype(np.int32)


def oracle_loop(model, images, codes, numeric, bg_codes, bg_numeric, col_offset, mean, scale, nan_fill, perms, out_width):
    """the straightforward loop on the CPU oracle model: one call per (sample, coalition) on the G mixed rows of that coalition
    (one row for v(all)) -> the logits, a list over samples of lists over coalitions (walk_masks order) of float64 [G or 1, C]"""
    masks = walk_masks(perms)
    none = so.table([so.record()])
    table = []
    with torch.no_grad():
        for b in range(len(codes)):
            table.append([])
            for k, mask in enumerate(masks):
                bgs = range(len(bg_codes)) if k < len(masks) - 1 else range(1)
                raw = [mix(codes[b], numeric[b], bg_codes[g], bg_numeric[g], mask) for g in bgs]
                metas = so.variants(np.stack([r[0] for r in raw]), np.stack([r[1] for r in raw]), col_offset, mean, scale, nan_fill, none,
                                    out_width)[0]
                table[-1].append(model(images[b:b + 1].expand(len(raw), *images.shape[1:]), torch.from_numpy(metas)).double().numpy())
    return table


def oracle_values(logit_table, perms, output):
    """oracle_loop's logits -> dict of phi [B, M, C], base, full [B, C] in float64, and the largest |logit|"""
    v = np.stack([np.stack([_out(l, output, np.float64).mean(axis=0) for l in row]) for row in logit_table])
    K = v.shape[1] - 2
    return dict(phi=phi_from_v(v, perms), base=v[:, K], full=v[:, K + 1], logit_max=max(float(np.abs(l).max()) for row in logit_table for l in row))
