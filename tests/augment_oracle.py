"""numpy restatement of the training transform of skinLesionDatasets.py:74-113 on uint8 HWC images, one function per stage
plus the composed pipeline -- the semantics csrc/augment.hip is held to, bit for bit.  It follows the published algorithms of
OpenCV's 8-bit paths (fixed-point warpAffine INTER_LINEAR, fixed-point GaussianBlur, integer RGB2HSV, float HSV2RGB) and
albumentations 1.4.18's LUTs; cv2 and albumentations are not available to the tests, so parity with cv2 itself is unpinned.

Everything here is written independently of mmskin.preprocess (which packs the same parameters for the kernel): the matrix
inversion and the Gaussian taps are derived again from the angle and (k, sigma).  `augment(images, params)` takes the dict
of per-sample parameter arrays that `TrainAugment.sample` returns (or hand-written ones; torch tensors or numpy arrays).
"""
import math

import numpy as np


def _np(v):
    return v.numpy() if hasattr(v, "numpy") else np.asarray(v)


# ---- borders (cv2 borderInterpolate, the loop form)
def border_reflect(p, n):
    """BORDER_REFLECT fedcba|abcdefgh|hgfedcb, repeated until the index is inside."""
    p = np.array(p, dtype=np.int64)
    if n == 1:
        return np.zeros_like(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p - 1, np.where(p >= n, 2 * n - 1 - p, p))
    return p


def border_reflect101(p, n):
    """BORDER_REFLECT_101 gfedcb|abcdefgh|gfedcba."""
    p = np.array(p, dtype=np.int64)
    if n == 1:
        return np.zeros_like(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))
    return p


# ---- Rotate
def rotation_matrix_inv(angle_deg, h, w):
    """cv2.getRotationMatrix2D((w/2 - 0.5, h/2 - 0.5), angle, 1.0) followed by warpAffine's float64 inversion."""
    cx, cy = w / 2 - 0.5, h / 2 - 0.5
    a = angle_deg * math.pi / 180.0
    alpha, beta = math.cos(a), math.sin(a)
    m = [alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy]
    d = m[0] * m[4] - m[1] * m[3]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[4] * d, m[0] * d
    m[0] = a11; m[1] *= -d; m[3] *= -d; m[4] = a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return np.array(m, dtype=np.float64).reshape(2, 3)


def rotate_u8(img, minv):
    """warpAffine(8-bit, INTER_LINEAR, BORDER_REFLECT) with the already inverted 2x3 float64 matrix: 10-bit fixed-point
    coordinates rounded to the 1/32 grid, 15-bit bilinear weights, (sum + 2^14) >> 15."""
    h, w = img.shape[:2]
    minv = np.asarray(minv, dtype=np.float64).reshape(2, 3)
    xs, ys = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    adelta = np.rint(minv[0, 0] * xs * 1024).astype(np.int64)
    bdelta = np.rint(minv[1, 0] * xs * 1024).astype(np.int64)
    x0 = np.rint((minv[0, 1] * ys + minv[0, 2]) * 1024).astype(np.int64) + 16
    y0 = np.rint((minv[1, 1] * ys + minv[1, 2]) * 1024).astype(np.int64) + 16
    X = (x0[:, None] + adelta[None, :]) >> 5
    Y = (y0[:, None] + bdelta[None, :]) >> 5
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx, fy = X & 31, Y & 31
    xa, xb = border_reflect(sx, w), border_reflect(sx + 1, w)
    ya, yb = border_reflect(sy, h), border_reflect(sy + 1, h)
    src = img.astype(np.int64)
    w00, w01 = 32 * (32 - fy) * (32 - fx), 32 * (32 - fy) * fx
    w10, w11 = 32 * fy * (32 - fx), 32 * fy * fx
    acc = (w00[..., None] * src[ya, xa] + w01[..., None] * src[ya, xb] + w10[..., None] * src[yb, xa]
           + w11[..., None] * src[yb, xb])
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


# ---- GaussianBlur
def gaussian_taps(k, sigma):
    """cv2's 8-bit fixed-point kernel: float64 Gaussian, normalised, quantised to 8 fractional bits by error diffusion from
    the edge inwards, the centre taking what is left of 256.  sigma <= 0 -> 0.3*((k-1)*0.5 - 1) + 0.8."""
    if sigma <= 0:
        sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    scale = -0.5 / (sigma * sigma)
    t = [math.exp(scale * (i - (k - 1) * 0.5) ** 2) for i in range(k)]
    inv = 1.0 / sum(t)
    taps, err, total = [0] * k, 0.0, 0
    for i in range(k // 2):
        adj = t[i] * inv * 256.0 + err
        v = int(np.rint(adj))
        err = adj - v
        taps[i] = taps[k - 1 - i] = v
        total += 2 * v
    taps[k // 2] = 256 - total
    return np.array(taps, dtype=np.int64)


def gaussian_blur_u8(img, k, sigma):
    """Separable, BORDER_REFLECT_101; the horizontal pass keeps all 16 bits, the vertical one rounds half up."""
    if k == 1:
        return img.copy()
    h, w = img.shape[:2]
    taps, r = gaussian_taps(k, sigma), k // 2
    xi = border_reflect101(np.arange(-r, w + r), w)
    yi = border_reflect101(np.arange(-r, h + r), h)
    src = img.astype(np.int64)[:, xi]
    hor = sum(taps[j] * src[:, j:j + w] for j in range(k))
    hor = hor[yi]
    ver = sum(taps[j] * hor[j:j + h] for j in range(k))
    return ((ver + (1 << 15)) >> 16).astype(np.uint8)


# ---- CoarseDropout
def coarse_dropout_u8(img, holes):
    out = img.copy()
    for x1, y1, x2, y2 in np.asarray(holes, dtype=np.int64).reshape(-1, 4):
        out[max(y1, 0):max(y2, 0), max(x1, 0):max(x2, 0)] = 0
    return out


# ---- HueSaturationValue
def _round_div(a, b):
    """a / b rounded half to even (cvRound of the exact quotient), integers."""
    q, r = divmod(a, b)
    return q + 1 if 2 * r > b or (2 * r == b and q % 2 == 1) else q


_SDIV = np.array([0] + [_round_div(255 << 12, i) for i in range(1, 256)], dtype=np.int64)
_HDIV = np.array([0] + [_round_div(180 << 12, 6 * i) for i in range(1, 256)], dtype=np.int64)


def rgb_to_hsv_u8(img):
    """cv2.cvtColor(RGB2HSV) on 8-bit: H in 0..179, 12-bit division tables."""
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    v = np.maximum(np.maximum(r, g), b)
    diff = v - np.minimum(np.minimum(r, g), b)
    s = (diff * _SDIV[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * _HDIV[diff] + (1 << 11)) >> 12
    h = np.where(h < 0, h + 180, h)
    return np.stack([np.clip(h, 0, 255), s, v], axis=-1).astype(np.uint8)


def hsv_to_rgb_u8(hsv):
    """cv2.cvtColor(HSV2RGB) on 8-bit: float32, every operation rounded on its own, round-half-even to uint8."""
    f32 = np.float32
    h = hsv[..., 0].astype(f32) * (f32(6.0) / f32(180.0))
    s = hsv[..., 1].astype(f32) * (f32(1.0) / f32(255.0))
    v = hsv[..., 2].astype(f32) * (f32(1.0) / f32(255.0))
    sector = np.floor(h).astype(np.int64)
    h = h - sector.astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    h = np.where(bad, f32(0), h).astype(f32)
    one = f32(1.0)
    tab = np.stack([v, v * (one - s), v * (one - s * h), v * (one - s * (one - h))], axis=-1)
    assert tab.dtype == np.float32
    order = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])[sector]     # (b, g, r) per sector
    bgr = np.take_along_axis(tab, order, axis=-1)
    bgr = np.where((hsv[..., 1] == 0)[..., None], v[..., None], bgr).astype(f32)
    out = np.clip(np.rint(bgr * f32(255.0)), 0, 255).astype(np.uint8)
    return out[..., ::-1]


def hue_saturation_value_u8(img, hue_shift, sat_shift, val_shift):
    """albumentations' _shift_hsv_uint8: LUTs on the int16 ramp, cast to uint8 by truncation."""
    hsv = rgb_to_hsv_u8(img)
    ramp = np.arange(256, dtype=np.int16)
    lut_h = np.mod(ramp + float(hue_shift), 180).astype(np.uint8)
    lut_s = np.clip(ramp + float(sat_shift), 0, 255).astype(np.uint8)
    lut_v = np.clip(ramp + float(val_shift), 0, 255).astype(np.uint8)
    hsv = np.stack([lut_h[hsv[..., 0]], lut_s[hsv[..., 1]], lut_v[hsv[..., 2]]], axis=-1)
    return hsv_to_rgb_u8(hsv)


# ---- RandomBrightnessContrast (brightness_by_max=True)
def brightness_contrast_lut(alpha, beta):
    lut = np.arange(256).astype(np.float32)
    lut = lut * np.float32(alpha)
    lut = lut + np.float32(float(beta) * 255)
    return np.clip(lut, 0, 255).astype(np.uint8)


def brightness_contrast_u8(img, alpha, beta):
    return brightness_contrast_lut(alpha, beta)[img]


# ---- the pipeline, in the reference's order
def augment_one(img, p, i):
    h, w = img.shape[:2]
    out = img
    if bool(p["rotate"][i]):
        out = rotate_u8(out, rotation_matrix_inv(float(p["angle"][i]), h, w))
    if bool(p["hflip"][i]):
        out = out[:, ::-1]
    if bool(p["vflip"][i]):
        out = out[::-1]
    if bool(p["blur"][i]):
        out = gaussian_blur_u8(out, int(p["ksize"][i]), float(p["sigma"][i]))
    if bool(p["dropout"][i]):
        out = coarse_dropout_u8(out, p["holes"][i][:int(p["n_holes"][i])])
    if bool(p["hsv"][i]):
        out = hue_saturation_value_u8(out, p["hue_shift"][i], p["sat_shift"][i], p["val_shift"][i])
    if bool(p["bc"][i]):
        out = brightness_contrast_u8(out, p["alpha"][i], p["beta"][i])
    return np.ascontiguousarray(out)


def augment(images, params):
    """uint8 [N, H, W, 3] + the parameter dict -> uint8 [N, H, W, 3]."""
    images = _np(images)
    p = {k: _np(v) for k, v in params.items()}
    return np.stack([augment_one(images[i], p, i) for i in range(images.shape[0])])


def identity_params(n):
    """Hand-written tables start here: every flag off, every parameter neutral (numpy arrays, the layout of
    `TrainAugment.sample`)."""
    z = lambda dt: np.zeros(n, dtype=dt)
    return dict(rotate=z(bool), angle=z(np.float64), hflip=z(bool), vflip=z(bool), blur=z(bool), ksize=np.full(n, 3, np.int32),
                sigma=z(np.float64), dropout=z(bool), n_holes=z(np.int32), holes=np.zeros((n, 8, 4), np.int32), hsv=z(bool),
                hue_shift=z(np.float32), sat_shift=z(np.float32), val_shift=z(np.float32), bc=z(bool),
                alpha=np.ones(n, np.float32), beta=z(np.float32))
