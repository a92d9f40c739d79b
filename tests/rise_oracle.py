"""numpy restatement of csrc/rise.hip and of mmskin.rise.RISE.generate_batch: the counter-based generator (mix64), the cell
grids and shifts of the masks, the mask value in exact integers (rounded to fp32 where the kernel rounds), the masked rows in
fp32 with every operation rounded on its own, and the weights and sums in fp64 in ascending mask order.
tests/test_cpu_rise.py holds it to torch's bilinear interpolate; tests/test_gpu_rise_ops.py holds the kernels to it."""
import numpy as np

import faithfulness_oracle as fo

F = np.float32
MASK64 = (1 << 64) - 1


def mix64(x):
    """splitmix64 finaliser on Python ints"""
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def word(key, j, q):
    return mix64(key ^ (j * 1024 + q))


def cell_size(H, W, g):
    return -(-H // g), -(-W // g)


def threshold(p1):
    return int(np.floor(float(p1) * 2.0 ** 24 + 0.5))


def cells(seed, j, g, p1):
    """G_j: int64 [g + 1, g + 1] of 0 / 1"""
    key, thr = mix64(seed), threshold(p1)
    return np.asarray([[1 if (word(key, j, r * (g + 1) + c) >> 40) < thr else 0 for c in range(g + 1)] for r in range(g + 1)],
                      dtype=np.int64)


def shift(seed, j, H, W, g):
    key = mix64(seed)
    ch, cw = cell_size(H, W, g)
    return ((word(key, j, 1022) >> 32) * ch) >> 32, ((word(key, j, 1023) >> 32) * cw) >> 32


def mask_exact(G, dy, dx, H, W):
    """(numerator int64 [H, W], denominator 4 ch cw): the mask as an exact rational"""
    g = G.shape[0] - 1
    ch, cw = cell_size(H, W, g)
    ty = 2 * (np.arange(H, dtype=np.int64) + dy) + 1 - ch
    tx = 2 * (np.arange(W, dtype=np.int64) + dx) + 1 - cw
    iy, ix = np.floor_divide(ty, 2 * ch), np.floor_divide(tx, 2 * cw)
    ry, rx = (ty - iy * 2 * ch)[:, None], (tx - ix * 2 * cw)[None, :]
    iy0, iy1 = np.clip(iy, 0, g)[:, None], np.clip(iy + 1, 0, g)[:, None]
    ix0, ix1 = np.clip(ix, 0, g)[None, :], np.clip(ix + 1, 0, g)[None, :]
    num = (2 * ch - ry) * (2 * cw - rx) * G[iy0, ix0] + (2 * ch - ry) * rx * G[iy0, ix1] \
        + ry * (2 * cw - rx) * G[iy1, ix0] + ry * rx * G[iy1, ix1]
    return num, 4 * ch * cw


def mask_unrounded(G, dy, dx, H, W):
    """fp64 [H, W]: the exact rational to one fp64 rounding"""
    num, den = mask_exact(G, dy, dx, H, W)
    return num.astype(np.float64) / np.float64(den)


def mask(seed, j, g, p1, H, W):
    """fp32 [H, W]: mask j as the kernels compute it -- numerator and denominator are exact in fp32, one fp32 division (the fp64
    quotient of two integers below 2^24 rounds to the same fp32: 53 >= 2 * 24 + 2)"""
    dy, dx = shift(seed, j, H, W, g)
    return mask_unrounded(cells(seed, j, g, p1), dy, dx, H, W).astype(F)


def masks(seed, j0, n, g, p1, H, W):
    return np.stack([mask(seed, j0 + i, g, p1, H, W) for i in range(n)])


def apply_formula(images, baseline, m, dtype):
    """baseline + m * (image - baseline) with every operation rounded to dtype; images, baseline [.., 3, H, W], m [.., H, W]"""
    x, b, m = images.astype(dtype), baseline.astype(dtype), m.astype(dtype)[..., None, :, :]
    d = x - b
    t = m * d
    return b + t


def apply(images, baseline, seed, g, p1, n_masks, r0, n, n_pad, dtype=F, mask_set=None):
    """-> [n_pad, 3, H, W]: rows r0 .. r0 + n - 1 of the image-major row space, zero rows from n on.  dtype fp32 = the kernel;
    fp64 = the reference it is judged against (the mask itself is the fp32 number in both)."""
    N, _, H, W = images.shape
    if mask_set is None:
        mask_set = masks(seed, 0, n_masks, g, p1, H, W)
    out = np.zeros((n_pad, 3, H, W), dtype=dtype)
    for i in range(n):
        img, j = divmod(r0 + i, n_masks)
        out[i] = apply_formula(images[img], baseline[img], mask_set[j], dtype)
    return out


def probabilities(logits, target):
    """fp64 soft-max probability of class target[r] of every row of logits [R, K]: the maximum, then the sum of exp(l - max) in
    ascending class order"""
    l64 = np.asarray(logits, dtype=F).astype(np.float64)
    e = np.exp(l64 - l64.max(axis=1, keepdims=True))
    den = np.zeros(len(l64), dtype=np.float64)
    for c in range(l64.shape[1]):
        den = den + e[:, c]
    return e[np.arange(len(l64)), target] / den


def accumulate(logits, clean_logits, mask_set, target=None):
    """logits [>= N * n_masks, K], clean_logits [N, K], mask_set fp32 [n_masks, H, W] -> dict of saliency_sum [N, H, W],
    coverage [H, W], clean_prob [N] (fp64), target int32 [N] and the weights w [N, n_masks]"""
    clean_logits = np.asarray(clean_logits, dtype=F)
    N, K = clean_logits.shape
    n_masks, H, W = mask_set.shape
    if target is None:
        tgt = clean_logits.argmax(axis=1).astype(np.int32)
    else:
        tgt = np.clip(np.asarray(target), 0, K - 1).astype(np.int32)
    w = probabilities(np.asarray(logits)[:N * n_masks], np.repeat(tgt, n_masks)).reshape(N, n_masks)
    m64 = mask_set.astype(np.float64)
    total, coverage = np.zeros((N, H, W), dtype=np.float64), np.zeros((H, W), dtype=np.float64)
    for j in range(n_masks):
        coverage = coverage + m64[j]
        total = total + w[:, j, None, None] * m64[j][None]
    return {"saliency_sum": total, "coverage": coverage, "clean_prob": probabilities(clean_logits, tgt), "target": tgt, "w": w}


def masked_rows(images, seed, g, p1, n_masks, baseline="zero", ksize=11, sigma=5.0):
    """every model input generate_batch builds, [N * n_masks, 3, H, W] fp32, in its row order, and the mask set"""
    images = np.ascontiguousarray(images, dtype=F)
    N, _, H, W = images.shape
    mask_set = masks(seed, 0, n_masks, g, p1, H, W)
    base = fo.baseline_images(images, baseline, ksize, sigma)
    return apply(images, base, seed, g, p1, n_masks, 0, N * n_masks, N * n_masks, mask_set=mask_set), mask_set
