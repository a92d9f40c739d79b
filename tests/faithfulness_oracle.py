"""numpy restatement of csrc/faithfulness.hip and of mmskin.faithfulness.CamFaithfulness.evaluate, in the kernels' own
operation order: rank by a stable argsort on the transformed key, blur and perturb in fp32 with every multiply and add rounded
on its own (the kernels are compiled with contraction switched off), mean and curves in fp64.  tests/test_cpu_faithfulness.py
holds it to independent forms (the O(n^2) rank definition, torch's conv2d on a reflect-padded fp64 input, numpy.trapz);
tests/test_gpu_faithfulness_ops.py holds the kernels to it."""
import numpy as np

F = np.float32
NT = 256                                   # the kernels' workgroup size: the stride of their fp64 partial sums
DELETION, INSERTION, EXPLANATION = 0, 1, 2


def rank_key(s):
    """uint32 key, descending saliency == descending key: NaN -> 0 (below -inf), -0.0 and +0.0 -> 0x80000000"""
    s = np.ascontiguousarray(s, dtype=F)
    u = s.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    key = np.where((u << np.uint32(1)) == 0, np.uint32(0x80000000), key)
    return np.where(np.isnan(s), np.uint32(0), key).astype(np.uint32)


def rank(saliency):
    """saliency [N, H, W] -> int32 [N, H, W]: position of every pixel in the stable descending order of its image"""
    saliency = np.ascontiguousarray(saliency, dtype=F)
    N = saliency.shape[0]
    key = rank_key(saliency).reshape(N, -1).astype(np.int64)
    out = np.empty(key.shape, dtype=np.int32)
    for n in range(N):
        order = np.argsort(-key[n], kind="stable")
        out[n, order] = np.arange(key.shape[1], dtype=np.int32)
    return out.reshape(saliency.shape)


def gaussian_taps(ksize, sigma):
    x = np.arange(ksize, dtype=np.float64) - ksize // 2
    w = np.exp(-0.5 * (x / float(sigma)) ** 2)
    return (w / w.sum()).astype(F)


def blur(x, taps):
    """x [..., H, W] fp32, taps fp32 [ksize] -> same shape: reflect padding, horizontal pass then vertical, ascending taps from an
    accumulator of zero, product and sum rounded to fp32 separately"""
    x = np.ascontiguousarray(x, dtype=F)
    taps = np.asarray(taps, dtype=F)
    r = len(taps) // 2
    H, W = x.shape[-2:]
    lead = [(0, 0)] * (x.ndim - 2)
    px = np.pad(x, lead + [(0, 0), (r, r)], mode="reflect")
    h = np.zeros_like(x)
    for t, w in enumerate(taps):
        h = h + w * px[..., :, t:t + W]
    py = np.pad(h, lead + [(r, r), (0, 0)], mode="reflect")
    v = np.zeros_like(x)
    for t, w in enumerate(taps):
        v = v + w * py[..., t:t + H, :]
    assert v.dtype == F
    return v


def _strided_tree_sum(values):
    """fp64 sum in the kernels' order: partial t = values[t] + values[t + NT] + ..., then a tree that halves NT"""
    values = np.asarray(values, dtype=np.float64).ravel()
    part = np.zeros(NT, dtype=np.float64)
    for t in range(min(NT, len(values))):
        acc = np.float64(0)
        for v in values[t::NT]:
            acc = acc + v
        part[t] = acc
    s = NT // 2
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0]


def mean_fill(x):
    """x [..., H, W] fp32 -> same shape, every plane filled with its mean (fp64 sum, one division, one rounding)"""
    x = np.ascontiguousarray(x, dtype=F)
    H, W = x.shape[-2:]
    flat = x.reshape(-1, H * W)
    out = np.empty_like(flat)
    for i, plane in enumerate(flat):
        out[i] = F(_strided_tree_sum(plane) / np.float64(H * W))
    return out.reshape(x.shape)


def perturb(images, baseline, ranks, saliency, rows, steps, n, n_pad):
    """-> [n_pad, 3, H, W] fp32: row j < n from entry rows[j] = (image, k, mode), clamped as the kernel clamps; zero rows from n on"""
    images, baseline = np.ascontiguousarray(images, dtype=F), np.ascontiguousarray(baseline, dtype=F)
    N, _, H, W = images.shape
    out = np.zeros((n_pad, 3, H, W), dtype=F)
    for j in range(n):
        img = int(np.clip(rows[j][0], 0, N - 1))
        k = int(np.clip(rows[j][1], 0, steps))
        mode = int(np.clip(rows[j][2], 0, 2))
        count = (k * H * W) // steps
        x, b = images[img], baseline[img]
        if mode == EXPLANATION:
            h = np.fmin(np.fmax(np.asarray(saliency[img], dtype=F), F(0)), F(1))[None]      # fmax / fmin: a NaN clamps to 0
            d = x - b
            m = h * d
            out[j] = b + m
        else:
            top = (np.asarray(ranks[img]) < count)[None]
            out[j] = np.where(top, b, x) if mode == DELETION else np.where(top, x, b)
    assert out.dtype == F
    return out


def row_table(n_images, steps):
    """int32 [N * (2 S + 3), 3], image-major: deletion k = 0 .. S, insertion k = 0 .. S, explanation"""
    rows = []
    for n in range(n_images):
        rows += [(n, k, DELETION) for k in range(steps + 1)] + [(n, k, INSERTION) for k in range(steps + 1)] + [(n, 0, EXPLANATION)]
    return np.asarray(rows, dtype=np.int32)


def trapezoid(curve):
    """area under curve[0 .. S] over x = k / S, in the kernel's order"""
    S = len(curve) - 1
    acc = np.float64(0)
    for k in range(S):
        acc = acc + (curve[k] + curve[k + 1])
    return acc * 0.5 / np.float64(S)


def curves(logits, steps, n_images, target=None):
    """logits [>= N * (2 S + 3), C] -> dict of the FaithfulnessResult fields (fp64; target int32)"""
    logits = np.asarray(logits, dtype=F)
    S, N, P = steps, n_images, 2 * steps + 3
    C = logits.shape[1]
    l64 = logits[:N * P].astype(np.float64).reshape(N, P, C)
    if target is None:
        tgt = np.asarray([int(np.argmax(l64[n, 0])) for n in range(N)], dtype=np.int32)
    else:
        tgt = np.clip(np.asarray(target), 0, C - 1).astype(np.int32)
    e = np.exp(l64 - l64.max(axis=2, keepdims=True))
    den = np.zeros((N, P), dtype=np.float64)
    for c in range(C):
        den = den + e[:, :, c]
    prob = np.stack([e[n, :, tgt[n]] / den[n] for n in range(N)])
    deletion, insertion, expl = prob[:, :S + 1], prob[:, S + 1:2 * S + 2], prob[:, 2 * S + 2]
    p = deletion[:, 0]
    out = {"deletion": deletion, "insertion": insertion,
           "deletion_auc": np.asarray([trapezoid(c) for c in deletion]), "insertion_auc": np.asarray([trapezoid(c) for c in insertion]),
           "average_drop": np.maximum(0.0, p - expl) / p, "increase": (expl > p).astype(np.float64), "target": tgt}
    for name in ("deletion_auc", "insertion_auc", "average_drop", "increase"):
        out["mean_" + name] = np.float64(out[name].sum() / N)
    return out


def baseline_images(images, baseline, ksize=11, sigma=5.0):
    images = np.ascontiguousarray(images, dtype=F)
    if baseline == "blur":
        return blur(images, gaussian_taps(ksize, sigma))
    if baseline == "mean":
        return mean_fill(images)
    assert baseline == "zero"
    return np.zeros_like(images)


def perturbed_rows(images, saliency, steps, baseline="blur", ksize=11, sigma=5.0):
    """every model input evaluate builds, [N * (2 S + 3), 3, H, W], in its row order"""
    images, saliency = np.ascontiguousarray(images, dtype=F), np.ascontiguousarray(saliency, dtype=F)
    rows = row_table(images.shape[0], steps)
    return perturb(images, baseline_images(images, baseline, ksize, sigma), rank(saliency), saliency, rows, steps, len(rows), len(rows))
