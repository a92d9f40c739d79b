"""Input side of the path on the GPU: what the reference's Dataset does on the host before
`model(image, metadata)` -- `A.Resize` of the val/test transform (skinLesionDatasets.py:116-120) and the
OneHotEncoder + StandardScaler metadata encoding (skinLesionDatasets.py:133-183).

    enc = MetadataEncoder().fit(categorical_rows, numeric_rows)      # or MetadataEncoder.from_sklearn(ohe, scaler)
    codes = enc.codes(categorical_rows)                              # host: strings -> int32 category indices
    meta = enc.transform(codes.cuda(), numeric.cuda())               # GPU: [B, onehot_width + n_num] fp32
    images = resize_u8(raw_u8_nhwc.cuda(), (224, 224))               # GPU: A.Resize; Normalize + ToTensor happen in the stem
    images = TrainAugment()(images)                                  # GPU: the train transform's augmentations, one kernel

Strings never reach the GPU: mapping a value to its index among the column's fitted categories stays on the host (one
dict lookup per cell); everything numeric runs through the C ABI.  No CPU fallback.
"""
import ctypes
import math

import numpy as np
import torch

from . import ops
from ._lib import call, ptr, stream


def resize_u8(images, size):
    """uint8 NHWC [N, Hs, Ws, 3] -> uint8 NHWC [N, size[0], size[1], 3] with cv2.resize(INTER_LINEAR) semantics."""
    ops._need_gpu(images, "resize_u8")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise ValueError(f"resize_u8 expects uint8 NHWC [N, H, W, 3], got {images.dtype} {tuple(images.shape)}")
    images = images.contiguous()
    n, hs, ws, _ = images.shape
    h, w = int(size[0]), int(size[1])
    if (hs, ws) == (h, w):
        return images
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=images.device)
    call("mmskin_resize_u8", ptr(images), n, hs, ws, ptr(out), h, w, stream())
    return out


class MetadataEncoder:
    """sklearn OneHotEncoder(sparse_output=False, handle_unknown='ignore') + StandardScaler, as the reference fits them
    (skinLesionDatasets.py:155-180): categories are the sorted unique strings of each column, the scaler uses the
    population standard deviation (ddof 0) with scale 1 for constant columns; missing numerics are filled with -1 BEFORE
    fitting and transforming (:148)."""

    nan_fill = -1.0

    def __init__(self):
        self.categories_ = None
        self.mean_ = None
        self.scale_ = None
        self._dev = {}

    # ---- fitting (host, once per dataset)
    def fit(self, categorical_rows, numeric_rows):
        cats = np.asarray(categorical_rows, dtype=object)
        cats = cats.reshape(len(cats), -1) if cats.size else np.empty((len(numeric_rows), 0), dtype=object)
        self.categories_ = [np.array(sorted({str(v) for v in cats[:, j]}), dtype=object) for j in range(cats.shape[1])]
        num = np.asarray(numeric_rows, dtype=np.float64).reshape(len(cats), -1)
        num = np.where(np.isnan(num), self.nan_fill, num)
        self.mean_ = num.mean(axis=0)
        var = num.var(axis=0)
        scale = np.sqrt(var)
        scale[scale < 10 * np.finfo(np.float64).eps * np.maximum(np.abs(self.mean_), 1.0)] = 1.0    # sklearn: _handle_zeros_in_scale
        self.scale_ = scale
        self._dev = {}
        return self

    @classmethod
    def from_sklearn(cls, ohe, scaler):
        """Adopt fitted sklearn objects (the reference pickles them under ./data/preprocess_data)."""
        self = cls()
        self.categories_ = [np.asarray(c, dtype=object) for c in ohe.categories_]
        self.mean_ = np.asarray(scaler.mean_, dtype=np.float64)
        self.scale_ = np.asarray(scaler.scale_, dtype=np.float64)
        return self

    @property
    def onehot_width(self):
        return int(sum(len(c) for c in self.categories_))

    @property
    def width(self):
        return self.onehot_width + len(self.mean_)

    # ---- per batch
    def codes(self, categorical_rows):
        """Host: [B, n_cat] int32 indices into the fitted categories; -1 for a value unseen at fit time."""
        rows = np.asarray(categorical_rows, dtype=object)
        rows = rows.reshape(len(rows), -1)
        lut = [{str(v): i for i, v in enumerate(c)} for c in self.categories_]
        out = np.full(rows.shape, -1, dtype=np.int32)
        for j, table in enumerate(lut):
            out[:, j] = [table.get(str(v), -1) for v in rows[:, j]]
        return torch.from_numpy(out)

    def col_offsets(self):
        """Host int32 [n_cat + 1]: the one-hot block of categorical column c is the slots [off[c], off[c + 1])."""
        return np.concatenate([[0], np.cumsum([len(c) for c in self.categories_])]).astype(np.int32)

    def _tables(self, device):
        t = self._dev.get(str(device))
        if t is None:
            t = (torch.from_numpy(self.col_offsets()).to(device), torch.tensor(self.mean_, dtype=torch.float32, device=device),
                 torch.tensor(self.scale_, dtype=torch.float32, device=device))
            self._dev[str(device)] = t
        return t

    def transform(self, codes, numeric):
        """GPU: codes int32 [B, n_cat], numeric fp32 [B, n_num] (NaN = missing) -> fp32 [B, width]."""
        ops._need_gpu(codes, "metadata_encode")
        codes = codes.to(torch.int32).contiguous()
        numeric = numeric.to(device=codes.device, dtype=torch.float32).contiguous()
        b, n_cat = codes.shape
        n_num = numeric.shape[1]
        if n_cat != len(self.categories_) or n_num != len(self.mean_):
            raise ValueError(f"metadata_encode: fitted for {len(self.categories_)} categorical + {len(self.mean_)} numeric "
                             f"columns, got {n_cat} + {n_num}")
        off, mean, scale = self._tables(codes.device)
        out = torch.empty((b, self.width), dtype=torch.float32, device=codes.device)
        call("mmskin_metadata_encode", ptr(codes), n_cat, ptr(off), self.onehot_width, ptr(numeric), n_num, ptr(mean),
             ptr(scale), float(self.nan_fill), ptr(out), b, stream())
        return out


# ---- training-time augmentation (skinLesionDatasets.py:74-113)
AUG_ROTATE, AUG_HFLIP, AUG_VFLIP, AUG_BLUR, AUG_DROPOUT, AUG_HSV, AUG_BC = 1, 2, 4, 8, 16, 32, 64     # MMSKIN_AUG_* of mmskin.h
AUG_MAX_HOLES = 8
# one record per sample: struct mmskin_augment_params of include/mmskin.h (160 bytes)
AUG_PARAMS_DTYPE = np.dtype([("minv", "<f8", (6,)), ("flags", "<u4"), ("ksize", "<i4"), ("taps", "<u2", (4,)), ("hue", "<i4"),
                             ("sat", "<i4"), ("val", "<i4"), ("alpha", "<f4"), ("beta255", "<f4"), ("n_holes", "<i4"),
                             ("holes", "<i2", (AUG_MAX_HOLES, 4)), ("reserved", "<u4", (2,))])
assert AUG_PARAMS_DTYPE.itemsize == 160
_AUG_KEYS = ("rotate", "angle", "hflip", "vflip", "blur", "ksize", "sigma", "dropout", "n_holes", "holes", "hsv", "hue_shift",
             "sat_shift", "val_shift", "bc", "alpha", "beta")


def _rotation_matrix_inv(angle, h, w):
    """cv2.getRotationMatrix2D about albumentations' centre (w/2 - 0.5, h/2 - 0.5), scale 1, then the float64 inversion
    cv2.warpAffine applies before it samples (dst -> src)."""
    cx, cy = w / 2 - 0.5, h / 2 - 0.5
    rad = angle * math.pi / 180.0
    a, b = math.cos(rad), math.sin(rad)
    m0, m1, m2, m3, m4, m5 = a, b, (1 - a) * cx - b * cy, -b, a, b * cx + (1 - a) * cy
    d = m0 * m4 - m1 * m3
    d = 1.0 / d if d != 0 else 0.0
    i0, i1, i3, i4 = m4 * d, m1 * -d, m3 * -d, m0 * d
    return (i0, i1, -i0 * m2 - i1 * m5, i3, i4, -i3 * m2 - i4 * m5)


def _gaussian_taps(k, sigma):
    """Half of cv2's 8-bit fixed-point Gaussian kernel, centre first: the float64 kernel exp(-x^2 / (2 sigma^2)) / sum is
    quantised to 8 fractional bits from the edge inwards, carrying the rounding error along, and the centre takes what is
    left of 256.  sigma <= 0 means cv2's 0.3 * ((k - 1) * 0.5 - 1) + 0.8."""
    if sigma <= 0:
        sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    scale = -0.5 / (sigma * sigma)
    t = [math.exp(scale * (i - (k - 1) * 0.5) ** 2) for i in range(k)]
    inv = 1.0 / sum(t)
    half, err = [], 0.0
    for i in range(k // 2):
        adj = t[i] * inv * 256.0 + err
        v = int(np.rint(adj))
        err = adj - v
        half.append(v)
    taps = [256 - 2 * sum(half)] + half[::-1]
    return taps + [0] * (4 - len(taps))


def pack_augment_params(params, height, width):
    """The per-sample parameter tensors of `TrainAugment.sample` (or hand-written ones) -> the table the kernel reads: a
    numpy array of AUG_PARAMS_DTYPE records.  Host work only: the float64 matrix inversion, the fixed-point blur taps and
    the floor of the HSV shifts (the LUTs albumentations builds, `(i + shift) mod 180` and `clip(i + shift, 0, 255)` cast to
    uint8, depend on floor(shift) alone)."""
    missing = [k for k in _AUG_KEYS if k not in params]
    if missing:
        raise ValueError(f"augmentation parameters lack {missing}")
    p = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in params.items()}
    n = len(p["rotate"])
    if any(len(p[k]) != n for k in _AUG_KEYS):
        raise ValueError("augmentation parameters disagree on the batch size")
    holes = p["holes"].reshape(n, -1, 4)[:, :AUG_MAX_HOLES]      # an n_holes beyond the table is reported by the library
    t = np.zeros(n, dtype=AUG_PARAMS_DTYPE)
    for name, bit in (("rotate", AUG_ROTATE), ("hflip", AUG_HFLIP), ("vflip", AUG_VFLIP), ("blur", AUG_BLUR),
                      ("dropout", AUG_DROPOUT), ("hsv", AUG_HSV), ("bc", AUG_BC)):
        t["flags"] |= np.where(p[name].astype(bool), bit, 0).astype(np.uint32)
    t["ksize"] = 1
    t["taps"][:, 0] = 256
    for i in range(n):
        if p["rotate"][i]:
            t["minv"][i] = _rotation_matrix_inv(float(p["angle"][i]), height, width)
        if p["blur"][i]:
            k = int(p["ksize"][i])
            t["ksize"][i] = k
            if k in (3, 5, 7):              # anything else is reported by the library
                t["taps"][i] = _gaussian_taps(k, float(p["sigma"][i]))
    t["hue"] = np.mod(np.floor(p["hue_shift"].astype(np.float64)), 180).astype(np.int32)
    t["sat"] = np.clip(np.floor(p["sat_shift"].astype(np.float64)), -255, 255).astype(np.int32)
    t["val"] = np.clip(np.floor(p["val_shift"].astype(np.float64)), -255, 255).astype(np.int32)
    t["alpha"] = p["alpha"].astype(np.float32)
    t["beta255"] = (p["beta"].astype(np.float32).astype(np.float64) * 255).astype(np.float32)
    t["n_holes"] = p["n_holes"].astype(np.int32)
    t["holes"][:, :holes.shape[1]] = np.clip(holes, -32768, 32767).astype(np.int16)
    return t


class TrainAugment:
    """The reference's training transform (skinLesionDatasets.py:74-113) batched on the GPU: `sample` draws every random
    parameter on the host into small per-sample tensors, `apply` runs the fused kernel (`mmskin_train_augment_u8`) on a raw
    uint8 NHWC batch.  The defaults reproduce the reference's A.Compose under albumentations 1.4.18:

        Rotate(limit=45, border_mode=BORDER_REFLECT, p=0.5)          angle ~ U(-45, 45), bilinear
        HorizontalFlip(p=0.5), VerticalFlip(p=0.2)
        GaussianBlur(sigma_limit=(0, 2), p=0.25)                     blur_limit = (3, 7): k = randrange(3, 8), an even draw
                                                                     moves to k + 1, so P(3, 5, 7) = (1, 2, 2) / 5;
                                                                     sigma ~ U(0, 2), 0 = cv2's 0.3*((k-1)*0.5 - 1) + 0.8
        CoarseDropout(max_holes=5, max_height=8, max_width=8, p=0.15)   fill 0
        HueSaturationValue(10, 15, 10, p=0.25)                       shifts ~ U(+-10), U(+-15), U(+-10)
        RandomBrightnessContrast(p=0.25)                             alpha = 1 + U(+-0.2), beta = U(+-0.2), by max

    albumentations' own random stream is not reproduced; the distributions and ranges are.

    `min_holes`, `min_height`, `min_width` (CoarseDropout's deprecated lower bounds): the reference passes only the `max_*`
    arguments.  albumentations documents "if None, min = max" for each of them, and 1.4.18 maps the deprecated pair to
    `num_holes_range = (min_holes or max_holes, max_holes)`, so the default None here means exactly `max_holes` holes of
    exactly `max_height` x `max_width` pixels (clipped to the image when it is smaller).  Pass integers to draw uniformly
    from [min, max] instead.

    Parameter tensors (all on the CPU, first dimension = batch): bool `rotate hflip vflip blur dropout hsv bc`; float64
    `angle` (degrees, counter-clockwise), `sigma`; int32 `ksize`, `n_holes`, `holes` [N, 8, 4] = x1, y1, x2, y2 (half
    open); float32 `hue_shift sat_shift val_shift alpha beta`.  Hand-written dicts of the same shape are accepted.
    """

    def __init__(self, rotate_limit=45.0, rotate_p=0.5, hflip_p=0.5, vflip_p=0.2, blur_limit=(3, 7), sigma_limit=(0.0, 2.0),
                 blur_p=0.25, max_holes=5, max_height=8, max_width=8, min_holes=None, min_height=None, min_width=None,
                 dropout_p=0.15, hue_shift_limit=10.0, sat_shift_limit=15.0, val_shift_limit=10.0, hsv_p=0.25,
                 brightness_limit=0.2, contrast_limit=0.2, brightness_contrast_p=0.25):
        lo, hi = int(blur_limit[0]), int(blur_limit[1])
        if not (3 <= lo <= hi <= 7 and lo % 2 == 1 and hi % 2 == 1):
            raise ValueError(f"blur_limit must be odd and within 3..7 (the kernel blurs with up to 7 taps), got {blur_limit}")
        if not 0 <= (max_holes if min_holes is None else min_holes) <= max_holes <= AUG_MAX_HOLES:
            raise ValueError(f"0 <= min_holes <= max_holes <= {AUG_MAX_HOLES} (the parameter table holds {AUG_MAX_HOLES} holes)")
        self.rotate_limit, self.blur_limit, self.sigma_limit = float(rotate_limit), (lo, hi), tuple(map(float, sigma_limit))
        self.holes_range = (max_holes if min_holes is None else int(min_holes), int(max_holes))
        self.height_range = (max_height if min_height is None else int(min_height), int(max_height))
        self.width_range = (max_width if min_width is None else int(min_width), int(max_width))
        self.hsv_limits = (float(hue_shift_limit), float(sat_shift_limit), float(val_shift_limit))
        self.brightness_limit, self.contrast_limit = float(brightness_limit), float(contrast_limit)
        self.p = dict(rotate=rotate_p, hflip=hflip_p, vflip=vflip_p, blur=blur_p, dropout=dropout_p, hsv=hsv_p,
                      bc=brightness_contrast_p)

    def sample(self, batch_size, height, width, generator=None):
        """Draw the parameters of `batch_size` samples of height x width pixels: one Bernoulli per transform and sample,
        then that transform's parameters.  The same `generator` state gives the same tensors."""
        n = int(batch_size)

        def uniform(lo, hi, *shape):
            return lo + (hi - lo) * torch.rand((n,) + shape, generator=generator, dtype=torch.float64)

        def randint(lo, hi, *shape):           # inclusive, lo / hi may be tensors
            return (lo + torch.floor(uniform(0.0, 1.0, *shape) * (hi - lo + 1))).to(torch.int32)

        out = {k: uniform(0.0, 1.0) < p for k, p in self.p.items()}
        out["angle"] = uniform(-self.rotate_limit, self.rotate_limit)
        k = randint(self.blur_limit[0], self.blur_limit[1])
        out["ksize"] = torch.where(k % 2 == 0, (k + 1) % (self.blur_limit[1] + 1), k)
        out["sigma"] = uniform(*self.sigma_limit)
        out["n_holes"] = randint(*self.holes_range)
        hole_h = randint(min(self.height_range[0], height), min(self.height_range[1], height), AUG_MAX_HOLES)
        hole_w = randint(min(self.width_range[0], width), min(self.width_range[1], width), AUG_MAX_HOLES)
        y1 = randint(0, height - hole_h, AUG_MAX_HOLES)
        x1 = randint(0, width - hole_w, AUG_MAX_HOLES)
        holes = torch.stack([x1, y1, x1 + hole_w, y1 + hole_h], dim=-1)
        used = torch.arange(AUG_MAX_HOLES)[None, :] < out["n_holes"][:, None]
        out["holes"] = torch.where(used[..., None], holes, torch.zeros_like(holes))
        for name, lim in zip(("hue_shift", "sat_shift", "val_shift"), self.hsv_limits):
            out[name] = uniform(-lim, lim).float()
        out["alpha"] = (1.0 + uniform(-self.contrast_limit, self.contrast_limit)).float()
        out["beta"] = uniform(-self.brightness_limit, self.brightness_limit).float()
        return out

    def apply(self, images, params):
        """uint8 NHWC [N, H, W, 3] on the GPU + parameters for N samples -> the augmented uint8 NHWC batch (a new tensor).
        No CPU fallback."""
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
            raise ValueError(f"TrainAugment expects uint8 NHWC [N, H, W, 3], got {getattr(images, 'dtype', type(images))} "
                             f"{tuple(getattr(images, 'shape', ()))}")
        ops._need_gpu(images, "train_augment")
        images = images.contiguous()
        n, h, w, _ = images.shape
        table = pack_augment_params(params, h, w)
        if len(table) != n:
            raise ValueError(f"TrainAugment: parameters for {len(table)} samples, batch of {n}")
        scratch = torch.empty(table.nbytes, dtype=torch.uint8, device=images.device)      # the library uploads the table into it
        out = torch.empty_like(images)
        call("mmskin_train_augment_u8", ptr(images), n, h, w, ctypes.c_void_p(table.ctypes.data), ptr(scratch), ptr(out),
             stream())
        return out

    def __call__(self, images, generator=None):
        if not isinstance(images, torch.Tensor) or images.dim() != 4:
            raise ValueError(f"TrainAugment expects uint8 NHWC [N, H, W, 3], got {type(images)}")
        return self.apply(images, self.sample(images.shape[0], images.shape[1], images.shape[2], generator))
