"""No GPU: the host half of the training-time augmentation -- `mmskin.preprocess.TrainAugment.sample` / `pack_augment_params`
-- and the numpy restatement tests/augment_oracle.py that the kernel is held to (tests/test_gpu_augment.py).  The
restatement is checked against properties that do not depend on its own formulas (numpy flips / rot90 / pad, float64
bilinear and Gaussian references), so it can be trusted before anything is compared with it."""
import math

import numpy as np
import pytest
import torch

import augment_oracle as O
from mmskin import _lib
from mmskin.preprocess import AUG_MAX_HOLES, TrainAugment, pack_augment_params


def _image(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _smooth(h, w, step):
    """uint8 image whose horizontal / vertical neighbours differ by at most `step` levels (asserted)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    amp = 0.45 * (step - 1)
    img = np.stack([128 + amp * (7 * np.sin(x / 7.0) + 6 * np.cos(y / 6.0)), 120 + amp * 9 * np.sin((x + y) / 13.0),
                    90 + amp * (5 * np.cos(x / 5.0) * np.sin(y / 9.0) + 4)], axis=-1)
    img = np.rint(img).astype(np.uint8)
    d = max(np.abs(np.diff(img.astype(int), axis=0)).max(), np.abs(np.diff(img.astype(int), axis=1)).max())
    assert 0 < d <= step, d
    return img


# ---- sampler
def test_sampler_is_reproducible():
    aug = TrainAugment()
    a = aug.sample(64, 37, 53, torch.Generator().manual_seed(7))
    b = aug.sample(64, 37, 53, torch.Generator().manual_seed(7))
    c = aug.sample(64, 37, 53, torch.Generator().manual_seed(8))
    assert a.keys() == b.keys()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], c[k]) for k in a)
    ta, tb = pack_augment_params(a, 37, 53), pack_augment_params(b, 37, 53)
    assert ta.tobytes() == tb.tobytes() and ta.itemsize == 160 and all(not v.is_cuda for v in a.values())


def test_sampler_rates_and_ranges():
    n, h, w = 20000, 224, 224
    p = TrainAugment().sample(n, h, w, torch.Generator().manual_seed(1))
    for name, prob in dict(rotate=0.5, hflip=0.5, vflip=0.2, blur=0.25, dropout=0.15, hsv=0.25, bc=0.25).items():
        rate = float(p[name].double().mean())
        assert abs(rate - prob) <= 5 * math.sqrt(prob * (1 - prob) / n), (name, rate)
    assert p["angle"].dtype == torch.float64 and float(p["angle"].abs().max()) <= 45 and float(p["angle"].abs().max()) > 40
    assert set(p["ksize"].tolist()) == {3, 5, 7}
    share = [float((p["ksize"] == k).double().mean()) for k in (3, 5, 7)]       # randrange(3, 8), even -> next odd
    assert all(abs(s - q) <= 5 * math.sqrt(q * (1 - q) / n) for s, q in zip(share, (0.2, 0.4, 0.4))), share
    assert float(p["sigma"].min()) >= 0 and float(p["sigma"].max()) <= 2
    f32 = lambda v: float(np.float32(v))
    for name, lim in (("hue_shift", 10), ("sat_shift", 15), ("val_shift", 10), ("beta", f32(0.2))):
        assert float(p[name].abs().max()) <= lim and float(p[name].min()) < -0.9 * lim and float(p[name].max()) > 0.9 * lim
    assert f32(0.8) <= float(p["alpha"].min()) < 0.82 and 1.18 < float(p["alpha"].max()) <= f32(1.2)
    assert set(p["n_holes"].tolist()) == {5}                  # min_holes=None -> max_holes (documented default)
    holes = p["holes"][:, :5]
    x1, y1, x2, y2 = holes.unbind(-1)
    assert int(x1.min()) >= 0 and int(y1.min()) >= 0 and int(x2.max()) <= w and int(y2.max()) <= h
    assert torch.equal(x2 - x1, torch.full_like(x1, 8)) and torch.equal(y2 - y1, torch.full_like(y1, 8))
    assert int(x1.max()) == w - 8 and int(y1.max()) == h - 8 and not p["holes"][:, 5:].any()


def test_sampler_hole_ranges_and_small_images():
    aug = TrainAugment(min_holes=0, max_holes=8, min_height=2, min_width=3)
    p = aug.sample(4000, 5, 9, torch.Generator().manual_seed(2))
    assert set(p["n_holes"].tolist()) == set(range(9))
    used = torch.arange(AUG_MAX_HOLES)[None] < p["n_holes"][:, None]
    x1, y1, x2, y2 = p["holes"].unbind(-1)
    assert int(x1.min()) >= 0 and int(y1.min()) >= 0 and int(x2.max()) <= 9 and int(y2.max()) <= 5
    assert set((y2 - y1)[used].tolist()) == {2, 3, 4, 5} and set((x2 - x1)[used].tolist()) == {3, 4, 5, 6, 7, 8}
    assert not p["holes"][~used].any()
    with pytest.raises(ValueError):
        TrainAugment(max_holes=AUG_MAX_HOLES + 1)
    with pytest.raises(ValueError):
        TrainAugment(blur_limit=(3, 9))


def test_packed_table_matches_the_restatement_helpers():
    """The packer's float64 matrix inversion and fixed-point taps against the restatement's own derivation."""
    p = O.identity_params(4)
    p["rotate"][:] = True
    p["angle"][:] = [45.0, -45.0, 0.0, 12.3456789]
    p["blur"][:] = True
    p["ksize"][:] = [3, 5, 7, 7]
    p["sigma"][:] = [0.0, 2.0, 0.0, 0.7]
    p["hsv"][:] = True
    p["hue_shift"][:] = [-0.5, 185.25, -180.0, 9.99]
    p["sat_shift"][:] = [-300.0, 300.0, -0.5, 14.5]
    t = pack_augment_params(p, 37, 53)
    for i in range(4):
        assert np.array_equal(t["minv"][i], O.rotation_matrix_inv(float(p["angle"][i]), 37, 53).ravel())
        k = int(p["ksize"][i])
        taps = O.gaussian_taps(k, float(p["sigma"][i]))
        assert taps.sum() == 256 and list(t["taps"][i][:k // 2 + 1]) == list(taps[k // 2:]) and not t["taps"][i][k // 2 + 1:].any()
    assert list(t["hue"]) == [179, 5, 0, 9] and list(t["sat"]) == [-255, 255, -1, 14] and list(t["flags"]) == [1 | 8 | 32] * 4


# ---- restatement: geometry
def test_all_flags_off_is_identity():
    img = np.stack([_image(37, 53, s) for s in range(3)])
    assert np.array_equal(O.augment(img, O.identity_params(3)), img)


def test_flip_only_equals_numpy_flip():
    img = np.stack([_image(37, 53, s) for s in range(3)])
    p = O.identity_params(3)
    p["hflip"][:] = [True, False, True]
    p["vflip"][:] = [False, True, True]
    out = O.augment(img, p)
    assert np.array_equal(out[0], np.flip(img[0], 1)) and np.array_equal(out[1], np.flip(img[1], 0))
    assert np.array_equal(out[2], np.flip(img[2], (0, 1)))


def test_rotate_by_90_equals_rot90_and_0_is_identity():
    img = _image(24, 24)
    assert np.array_equal(O.rotate_u8(img, O.rotation_matrix_inv(90.0, 24, 24)), np.rot90(img, 1))      # counter-clockwise
    assert np.array_equal(O.rotate_u8(img, O.rotation_matrix_inv(-90.0, 24, 24)), np.rot90(img, -1))
    odd = _image(37, 53, 3)
    assert np.array_equal(O.rotate_u8(odd, O.rotation_matrix_inv(0.0, 37, 53)), odd)


def test_reflect_border_equals_symmetric_padding():
    """5x9 turned by 45 degrees samples more than one image size outside: the repeated fedcba|abcdefgh reflection must equal
    reading an np.pad(mode="symmetric") copy padded wider than the image."""
    img, pad = _image(5, 9, 4), 40
    minv = O.rotation_matrix_inv(45.0, 5, 9)
    big = np.pad(img, ((pad, pad), (pad, pad), (0, 0)), mode="symmetric").astype(np.int64)
    want = np.empty_like(img)
    far = 0
    for y in range(5):
        for x in range(9):
            X = (int(np.rint((minv[0, 1] * y + minv[0, 2]) * 1024)) + 16 + int(np.rint(minv[0, 0] * x * 1024))) >> 5
            Y = (int(np.rint((minv[1, 1] * y + minv[1, 2]) * 1024)) + 16 + int(np.rint(minv[1, 0] * x * 1024))) >> 5
            sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
            far = max(far, -sx, sx - 8, -sy, sy - 4)
            q = big[sy + pad:sy + pad + 2, sx + pad:sx + pad + 2]
            acc = 32 * ((32 - fy) * ((32 - fx) * q[0, 0] + fx * q[0, 1]) + fy * ((32 - fx) * q[1, 0] + fx * q[1, 1]))
            want[y, x] = (acc + (1 << 14)) >> 15
    assert far >= 2                                            # really outside the image
    assert np.array_equal(O.rotate_u8(img, minv), want)
    idx = np.arange(-23, 24)
    assert np.array_equal(O.border_reflect(idx, 5), np.pad(np.arange(5), 25, mode="symmetric")[idx + 25])
    assert np.array_equal(O.border_reflect101(idx, 5), np.pad(np.arange(5), 25, mode="reflect")[idx + 25])
    assert list(O.border_reflect([-6, -1, 5, 10], 5)) == [4, 0, 4, 0] and list(O.border_reflect101([-5, -1, 5, 9], 5)) == [3, 1, 3, 1]


@pytest.mark.parametrize("angle", [45.0, -45.0, 33.7, -7.25])
def test_rotate_within_one_level_of_float64_bilinear(angle):
    """Coordinates are rounded to the 1/32 grid (error <= 1/64 pixel per axis); with neighbouring pixels at most 8 levels
    apart that is <= 2 * 8 / 64 = 0.25 level before the final rounding, so <= 1 level after it."""
    h, w = 40, 52
    img = _smooth(h, w, 8)
    minv = O.rotation_matrix_inv(angle, h, w)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    X = minv[0, 0] * x + minv[0, 1] * y + minv[0, 2]
    Y = minv[1, 0] * x + minv[1, 1] * y + minv[1, 2]
    grid = torch.from_numpy(np.stack([(2 * X + 1) / w - 1, (2 * Y + 1) / h - 1], axis=-1))[None]
    src = torch.from_numpy(img).double().permute(2, 0, 1)[None]
    ref = torch.nn.functional.grid_sample(src, grid, mode="bilinear", padding_mode="reflection", align_corners=False)
    ref = ref[0].permute(1, 2, 0).numpy()
    err = np.abs(O.rotate_u8(img, minv).astype(np.float64) - ref).max()
    print("max |restatement - float64 bilinear| =", err)
    assert err <= 1.0


# ---- restatement: blur
BLUR_CASES = [(3, 0.0), (3, 2.0), (5, 0.0), (5, 1.1), (7, 0.0), (7, 2.0), (7, 0.05), (3, -1.0), (5, 0.3), (7, 0.8)]


def _float_gaussian(k, sigma):
    """Normalised float64 Gaussian weights, written from the definition: sigma <= 0 means 0.3*((k-1)*0.5 - 1) + 0.8."""
    s = sigma if sigma > 0 else 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    wts = np.exp(-0.5 * (np.arange(-(k // 2), k // 2 + 1) / s) ** 2)
    return wts / wts.sum()


@pytest.mark.parametrize("k,sigma", BLUR_CASES)
def test_blur_taps_are_the_quantised_gaussian(k, sigma):
    """The fixed-point taps against the float64 weights.  Error diffusion rounds `256 w_i + carry` with |carry| <= 1/2, so an
    edge tap is within 1 of 256 w_i; the carry after the last edge tap bounds the summed edge error by 1/2, so the centre
    (what is left of 256) is within 1 too: every tap / 256 is within 1/256 of its weight."""
    taps, wts = O.gaussian_taps(k, sigma), _float_gaussian(k, sigma)
    assert len(taps) == k and taps.sum() == 256 and (taps >= 0).all() and np.array_equal(taps, taps[::-1])
    assert np.abs(taps / 256.0 - wts).max() <= 1 / 256 + 1e-12, (taps, wts)
    if sigma <= 0:                                             # the sigma-0 rule: same taps as the explicit sigma
        assert np.array_equal(taps, O.gaussian_taps(k, 0.3 * ((k - 1) * 0.5 - 1) + 0.8))


@pytest.mark.parametrize("k,sigma", BLUR_CASES)
def test_blur_of_an_impulse_is_the_outer_product_of_the_weights(k, sigma):
    """One pixel of 255 on black, away from the borders, blurs to 255 w_y w_x.  With every tap within e = 1/256 of its weight
    the product is within e (w_y + w_x) + e^2, plus 1/2 for the final rounding -- a bound from the float weights alone.  A
    blur that ignored or mis-scaled sigma, or did nothing, is tens of levels off here."""
    img = np.zeros((15, 17, 3), np.uint8)
    img[7, 8] = (255, 255, 100)
    wts, r, e = _float_gaussian(k, sigma), k // 2, 1 / 256
    got = O.gaussian_blur_u8(img, k, sigma).astype(np.float64)
    ref = np.zeros((15, 17), np.float64)
    bound = np.full((15, 17), 0.5)
    ref[7 - r:8 + r, 8 - r:9 + r] = np.outer(wts, wts)
    bound[7 - r:8 + r, 8 - r:9 + r] += 255 * (e * (wts[:, None] + wts[None, :]) + e * e)
    for c, amp in enumerate((255, 255, 100)):
        err = np.abs(got[..., c] - amp * ref)
        print(f"k={k} sigma={sigma} c={c}: max |restatement - float64| = {err.max():.3f}, bound at that pixel "
              f"{bound.flat[err.argmax()]:.3f}")
        assert (err <= bound).all()
    assert bound.max() <= 2.5
    if wts[r] < 0.9:                                           # the check can tell a blur from none, and one sigma from another
        assert (np.abs(img[..., 0] - 255 * ref) > bound).any()
        wide = _float_gaussian(k, (sigma if sigma > 0 else 0.3 * ((k - 1) * 0.5 - 1) + 0.8) * 1.5)
        other = np.zeros_like(ref)
        other[7 - r:8 + r, 8 - r:9 + r] = np.outer(wide, wide)
        assert (np.abs(got[..., 0] - 255 * other) > bound).any()


@pytest.mark.parametrize("k,sigma", BLUR_CASES)
def test_blur_constant_borders_and_float64_gaussian(k, sigma):
    """Taps sum to 256, so a constant stays.  Against the float64 Gaussian on a smooth image (neighbours at most 2 levels
    apart, <= 6 levels from the centre inside a 7-tap window): taps within 1/256 of the weights with errors summing to zero
    put a pass off by at most 6 * 6/256 = 0.15 level, two passes 0.3, plus 0.5 of rounding: < 1.  (The weights themselves are
    pinned by the two tests above; this one covers the reflect-101 border and the rounding on a full image.)"""
    for c in (0, 1, 200, 255):
        const = np.full((9, 11, 3), c, np.uint8)
        assert np.array_equal(O.gaussian_blur_u8(const, k, sigma), const)
    img = _smooth(21, 30, 2)
    r, wts = k // 2, _float_gaussian(k, sigma)
    pad = np.pad(img.astype(np.float64), ((r, r), (r, r), (0, 0)), mode="reflect")
    hor = sum(wts[j] * pad[:, j:j + 30] for j in range(k))
    ref = sum(wts[j] * hor[j:j + 21] for j in range(k))
    err = np.abs(O.gaussian_blur_u8(img, k, sigma).astype(np.float64) - ref).max()
    print("max |restatement - float64 gaussian| =", err)
    assert err <= 1.0
    tiny = _image(5, 9, 6)                                     # smaller than the kernel: the border reflects repeatedly
    taps = O.gaussian_taps(k, sigma)
    padt = np.pad(tiny.astype(np.int64), ((r, r), (r, r), (0, 0)), mode="reflect")
    full = sum(taps[a] * taps[b] * padt[a:a + 5, b:b + 9] for a in range(k) for b in range(k))
    assert np.array_equal(O.gaussian_blur_u8(tiny, k, sigma), (full + 32768) >> 16)


# ---- restatement: colour
def test_hsv_grey_hue_wrap_and_primaries():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)           # [256, 1, 3]
    for shift in (-300.0, -37.0, -0.5, 0.0, 0.5, 10.0, 41.9, 300.0):
        out = O.hue_saturation_value_u8(grey, 77.0, 0.0, shift)
        want = np.clip(np.arange(256) + math.floor(shift), 0, 255)
        assert np.array_equal(out, np.repeat(want[:, None, None], 3, axis=2).astype(np.uint8)), shift
    img = _image(16, 16, 9)
    assert np.array_equal(O.hue_saturation_value_u8(img, 180.0, 3.0, -4.0), O.hue_saturation_value_u8(img, 0.0, 3.0, -4.0))
    assert np.array_equal(O.hue_saturation_value_u8(img, -170.0, 0.0, 0.0), O.hue_saturation_value_u8(img, 10.0, 0.0, 0.0))
    prim = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8)
    assert np.array_equal(O.hue_saturation_value_u8(prim, 60.0, 0.0, 0.0), prim[:, [1, 2, 0]])    # red -> green -> blue -> red
    assert np.array_equal(O.rgb_to_hsv_u8(prim)[0], [[0, 255, 255], [60, 255, 255], [120, 255, 255]])
    back = O.hsv_to_rgb_u8(O.rgb_to_hsv_u8(img)).astype(int) - img
    assert np.abs(back).max() <= 6                             # H is quantised to 2-degree steps: a round trip is only close


@pytest.mark.parametrize("alpha,beta", [(0.8, -0.2), (1.2, 0.2), (0.8, 0.2), (1.2, -0.2), (1.0, 0.0), (1.0371, -0.0613)])
def test_brightness_lut_equals_float32_expression(alpha, beta):
    ramp = torch.arange(256, dtype=torch.float32)
    want = (ramp * torch.tensor(alpha, dtype=torch.float32) + torch.tensor(beta * 255, dtype=torch.float32)).clamp(0, 255)
    lut = O.brightness_contrast_lut(np.float32(alpha), beta)
    assert np.array_equal(lut, want.to(torch.uint8).numpy())
    img = _image(8, 8, 2)
    assert np.array_equal(O.brightness_contrast_u8(img, np.float32(alpha), beta), lut[img])


def test_dropout_zeroes_exactly_the_rectangles():
    img = np.maximum(_image(37, 53, 5), 1)
    holes = [(0, 0, 8, 8), (45, 29, 53, 37), (20, 0, 28, 3), (0, 30, 2, 37), (50, 10, 53, 18)]
    mask = np.zeros((37, 53), bool)
    for x1, y1, x2, y2 in holes:
        mask[y1:y2, x1:x2] = True
    out = O.coarse_dropout_u8(img, holes)
    assert not out[mask].any() and np.array_equal(out[~mask], img[~mask])
    p = O.identity_params(1)
    p["dropout"][:] = True
    p["n_holes"][:] = 2                                        # only the first two of the listed holes are in use
    p["holes"][0, :5] = holes
    out = O.augment(img[None], p)[0]
    mask2 = np.zeros((37, 53), bool)
    mask2[0:8, 0:8] = mask2[29:37, 45:53] = True
    assert not out[mask2].any() and np.array_equal(out[~mask2], img[~mask2])


def test_pipeline_composes_the_stages_in_order():
    img = _image(37, 53, 11)
    p = TrainAugment(rotate_p=1, hflip_p=1, vflip_p=1, blur_p=1, dropout_p=1, hsv_p=1, brightness_contrast_p=1).sample(
        1, 37, 53, torch.Generator().manual_seed(3))
    q = {k: v.numpy() for k, v in p.items()}
    want = O.rotate_u8(img, O.rotation_matrix_inv(float(q["angle"][0]), 37, 53))[::-1, ::-1]
    want = O.gaussian_blur_u8(want, int(q["ksize"][0]), float(q["sigma"][0]))
    want = O.coarse_dropout_u8(want, q["holes"][0][:5])
    want = O.hue_saturation_value_u8(want, q["hue_shift"][0], q["sat_shift"][0], q["val_shift"][0])
    want = O.brightness_contrast_u8(want, q["alpha"][0], q["beta"][0])
    assert np.array_equal(O.augment(img[None], p)[0], want)


# ---- boundary
def test_backbone_hook_is_off_by_default():
    from mmskin.backbone import _FlatBackbone
    assert _FlatBackbone.train_augment is None and _FlatBackbone.resize_to is None


def test_apply_has_no_cpu_fallback_and_validates_its_input():
    aug = TrainAugment()
    img = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    params = aug.sample(2, 8, 8, torch.Generator().manual_seed(0))
    with pytest.raises(_lib.MMSkinError, match="no CPU fallback"):
        aug.apply(img, params)
    with pytest.raises(_lib.MMSkinError, match="no CPU fallback"):
        aug(img)
    for bad in (img.float(), img[..., :2], img[0], img.permute(0, 3, 1, 2)):
        with pytest.raises(ValueError):
            aug.apply(bad, params)
