"""-m gpu: the training-time augmentation kernel (`mmskin_train_augment_u8` through `mmskin.preprocess.TrainAugment.apply`)
against the numpy restatement tests/augment_oracle.py -- bit for bit, no tolerance (cv2 / albumentations themselves are
absent -> parity with cv2 unpinned, like resize_u8).  Shapes are the smallest that still reach every path: 37x53 (odd, partial
tiles on both edges), 5x9 (smaller than the 7-tap blur and the 8x8 holes, borders reflect repeatedly), 64x96 (full tiles,
halo across seams), and one 224x224 case."""
import ctypes

import numpy as np
import pytest
import torch

import augment_oracle as O
from gpu_util import DEV
from mmskin import _lib
from mmskin.preprocess import AUG_MAX_HOLES, TrainAugment, pack_augment_params

pytestmark = pytest.mark.gpu

SHAPES = [(3, 37, 53), (2, 5, 9), (2, 64, 96)]
SPECIAL = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [128, 128, 128], [255, 255, 0], [1, 0, 0],
                    [0, 0, 1], [254, 255, 255], [17, 17, 16], [200, 100, 100]], dtype=np.uint8)


def _images(n, h, w, seed=0):
    img = np.random.default_rng(seed * 7919 + h * 131 + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    flat = img.reshape(n, h * w, 3)
    m = min(len(SPECIAL), h * w // 2)
    flat[:, :m] = SPECIAL[:m]            # greys, primaries, black / white: the corners of the HSV conversion
    return img


def _assert_equals_restatement(got, img, params):
    want = O.augment(img, params)
    assert got.shape == want.shape and got.dtype == np.uint8
    if not np.array_equal(got, want):
        diff = np.abs(got.astype(int) - want.astype(int))
        first = int(np.nonzero(diff.reshape(len(diff), -1).any(axis=1))[0][0])
        where = np.argwhere(diff[first])[0].tolist()
        pytest.fail(f"kernel != restatement: max |diff| = {int(diff.max())}, {int((diff > 0).sum())} values differ, first "
                    f"differing sample {first} at (y, x, c) = {where}")


def _check(img, params):
    got = TrainAugment().apply(torch.from_numpy(img).to(DEV), params).cpu().numpy()
    _assert_equals_restatement(got, img, params)
    return got


def _run_corners(shape, corners, seed=0):
    """Every entry of `corners` (a dict of per-sample overrides on top of all-flags-off) runs at least once, `n` per call."""
    n, h, w = shape
    for start in range(0, len(corners), n):
        p = O.identity_params(n)
        for i in range(n):
            for key, value in corners[(start + i) % len(corners)].items():
                p[key][i] = value
        _check(_images(n, h, w, seed + start), p)


def _holes(h, w):
    """8 rectangles: one touching each image edge and corner, two overhanging, one single pixel."""
    return np.array([(0, 0, 8, 8), (w - 8, h - 8, w, h), (w // 2, 0, w // 2 + 8, 3), (0, h - 2, 5, h), (w - 3, 1, w, 4),
                     (-2, -2, 3, 3), (w - 2, h - 2, w + 5, h + 5), (w // 3, h // 3, w // 3 + 1, h // 3 + 1)], dtype=np.int32)


ROTATE = [dict(rotate=True, angle=a) for a in (45.0, -45.0, 0.0, 17.3, -33.77)]
FLIP = [dict(hflip=True), dict(vflip=True), dict(hflip=True, vflip=True), dict(rotate=True, angle=45.0, hflip=True),
        dict(rotate=True, angle=-20.5, vflip=True), dict(rotate=True, angle=31.0, hflip=True, vflip=True)]
BLUR = [dict(blur=True, ksize=k, sigma=s) for k in (3, 5, 7) for s in (0.0, 2.0)] + [dict(blur=True, ksize=7, sigma=0.6)]
HSV = [dict(hsv=True, hue_shift=a, sat_shift=b, val_shift=c) for a, b, c in
       ((170.5, 0.0, 0.0), (-10.0, -300.0, 300.0), (9.99, 300.0, -300.0), (-0.5, 15.0, 10.5), (179.0, -15.0, -10.5),
        (0.0, 0.0, 0.0), (95.25, 255.0, 255.0), (-95.25, -255.0, -255.0))]
BC = [dict(bc=True, alpha=a, beta=b) for a, b in ((0.8, -0.2), (1.2, 0.2), (0.8, 0.2), (1.2, -0.2), (1.0371, -0.0613), (1.0, 0.0))]


@pytest.mark.parametrize("shape", SHAPES)
def test_rotate_alone(shape):
    _run_corners(shape, ROTATE)


@pytest.mark.parametrize("shape", SHAPES)
def test_flips_alone_and_after_rotate(shape):
    _run_corners(shape, FLIP)
    n, h, w = shape                      # a flip-only sample is an exact permutation of its input
    p = O.identity_params(n)
    p["hflip"][:] = True
    p["vflip"][0] = True
    img = _images(n, h, w, 3)
    got = _check(img, p)
    assert np.array_equal(got[0], img[0, ::-1, ::-1]) and np.array_equal(got[1], img[1, :, ::-1])


@pytest.mark.parametrize("shape", SHAPES)
def test_blur_alone(shape):
    _run_corners(shape, BLUR)


@pytest.mark.parametrize("shape", SHAPES)
def test_dropout_alone(shape):
    n, h, w = shape
    holes = _holes(h, w)
    _run_corners(shape, [dict(dropout=True, n_holes=0, holes=holes), dict(dropout=True, n_holes=AUG_MAX_HOLES, holes=holes),
                         dict(dropout=True, n_holes=5, holes=holes), dict(dropout=False, n_holes=AUG_MAX_HOLES, holes=holes)])


@pytest.mark.parametrize("shape", SHAPES)
def test_hue_saturation_value_alone(shape):
    _run_corners(shape, HSV)


@pytest.mark.parametrize("shape", SHAPES)
def test_brightness_contrast_alone(shape):
    _run_corners(shape, BC)


def _everything(h, w, i):
    c = dict(dropout=True, n_holes=(AUG_MAX_HOLES, 3, 5)[i % 3], holes=_holes(h, w))
    for group in (ROTATE, FLIP[:3], BLUR, HSV, BC):
        c.update(group[i % len(group)])
    return c


@pytest.mark.parametrize("shape", SHAPES + [(2, 224, 224)])
def test_all_stages_together(shape):
    n, h, w = shape
    _run_corners(shape, [_everything(h, w, i) for i in range(7 if h < 200 else 2)], seed=5)


def test_mixed_batch_and_untouched_sample():
    """Every sample another subset of the stages (sample 0: none -> bit-identical to its input): per-sample indexing."""
    n, h, w = 8, 37, 53
    groups = [ROTATE[3], FLIP[2], BLUR[5], dict(dropout=True, n_holes=AUG_MAX_HOLES, holes=_holes(h, w)), HSV[1], BC[4]]
    subsets = [(), (0,), (1, 2), (3,), (4, 5), (0, 2, 4), (1, 3, 5), (0, 1, 2, 3, 4, 5)]
    p = O.identity_params(n)
    for i, subset in enumerate(subsets):
        for g in subset:
            for key, value in groups[g].items():
                p[key][i] = value
    img = _images(n, h, w, 9)
    got = _check(img, p)
    assert np.array_equal(got[0], img[0])
    flags = pack_augment_params(p, h, w)["flags"]
    assert len(set(flags.tolist())) == n and flags[0] == 0


def test_same_table_same_output():
    n, h, w = 3, 37, 53
    aug = TrainAugment(rotate_p=1, blur_p=1, dropout_p=1, hsv_p=1, brightness_contrast_p=1)
    p = aug.sample(n, h, w, torch.Generator().manual_seed(4))
    img = torch.from_numpy(_images(n, h, w, 2)).to(DEV)
    keep = img.clone()
    a, b = aug.apply(img, p), aug.apply(img, p)
    assert torch.equal(a, b) and torch.equal(img, keep) and a.data_ptr() != img.data_ptr()


@pytest.mark.parametrize("seed,boost", [(0, False), (1, True)])
def test_sampled_table_matches_restatement(seed, boost):
    """The reference's probabilities, and a second table with every stage likely so that 8 samples reach all of them."""
    aug = TrainAugment(rotate_p=0.8, hflip_p=0.5, vflip_p=0.5, blur_p=0.8, dropout_p=0.8, hsv_p=0.8,
                       brightness_contrast_p=0.8) if boost else TrainAugment()
    p = aug.sample(8, 37, 53, torch.Generator().manual_seed(seed))
    _check(_images(8, 37, 53, seed), p)


def test_sampled_table_full_size_through_call():
    """224x224 through __call__ (sample + apply) with a seeded generator."""
    aug = TrainAugment(rotate_p=1, blur_p=1, dropout_p=1, hsv_p=1, brightness_contrast_p=1)
    img = _images(2, 224, 224, 1)
    got = aug(torch.from_numpy(img).to(DEV), torch.Generator().manual_seed(11)).cpu().numpy()
    _assert_equals_restatement(got, img, aug.sample(2, 224, 224, torch.Generator().manual_seed(11)))


def test_bad_arguments_raise():
    aug, img = TrainAugment(), torch.from_numpy(_images(2, 16, 16)).to(DEV)
    p = O.identity_params(2)
    p["blur"][:] = True
    for k in (4, 9, 0, -3):
        p["ksize"][1] = k
        with pytest.raises(_lib.MMSkinError, match="kernel size"):
            aug.apply(img, p)
    p = O.identity_params(2)
    p["dropout"][:] = True
    p["n_holes"][0] = AUG_MAX_HOLES + 1
    with pytest.raises(_lib.MMSkinError, match="holes"):
        aug.apply(img, p)
    with pytest.raises(ValueError):
        aug.apply(img, O.identity_params(3))
    table = pack_augment_params(O.identity_params(2), 16, 16)
    dev = torch.empty(table.nbytes, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(img)
    host = ctypes.c_void_p(table.ctypes.data)
    for n, h, w in ((2, 0, 16), (2, 16, 0), (2, -1, 16), (0, 16, 16)):
        with pytest.raises(_lib.MMSkinError, match="bad shape"):
            _lib.call("mmskin_train_augment_u8", _lib.ptr(img), n, h, w, host, _lib.ptr(dev), _lib.ptr(out), _lib.stream())
    with pytest.raises(_lib.MMSkinError, match="null"):
        _lib.call("mmskin_train_augment_u8", _lib.ptr(img), 2, 16, 16, None, _lib.ptr(dev), _lib.ptr(out), _lib.stream())
    with pytest.raises(ValueError):
        aug.apply(img.float(), O.identity_params(2))
    torch.cuda.synchronize()


def test_backbone_hook_trains_on_augmented_batch_and_leaves_eval_alone(monkeypatch):
    """`image_encoder.train_augment`: in train() mode a uint8 batch is augmented on the device before the stem, so the
    logits equal the same model without the hook fed the restatement's output for that table; in eval() mode the hook does
    nothing."""
    import os
    from helpers import SMALL, disable_dropout
    from models import multimodalIntraInterModal as M
    from oracle.detinit import det_init_, det_inputs
    os.environ["MMSKIN_BACKBONE_DTYPE"] = "fp32"
    model = det_init_(M.MultimodalModel(**dict(SMALL, cnn_model_name="resnet-18", attention_mecanism="concatenation", device=DEV))).to(DEV)
    disable_dropout(model)
    raw = torch.from_numpy(_images(3, 96, 96, 5))
    meta = det_inputs(3, 32, 20, 6)[1].to(DEV)
    aug = TrainAugment(rotate_p=1, blur_p=1, dropout_p=1, hsv_p=1, brightness_contrast_p=1)
    table = aug.sample(3, 96, 96, torch.Generator().manual_seed(6))
    monkeypatch.setattr(aug, "sample", lambda *a, **k: table)
    want_images = torch.from_numpy(O.augment(raw.numpy(), table))
    assert not torch.equal(want_images, raw)
    enc = model.image_encoder
    with torch.no_grad():
        model.train()
        enc.train_augment = aug
        a = model(raw.to(DEV), meta).cpu()
        enc.train_augment = None
        b = model(want_images.to(DEV), meta).cpu()
        plain = model(raw.to(DEV), meta).cpu()
        model.eval()
        c = model(raw.to(DEV), meta).cpu()
        enc.train_augment = aug
        d = model(raw.to(DEV), meta).cpu()
    assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), (a - b).abs().max()
    assert not torch.allclose(a, plain, rtol=1e-3, atol=1e-4)          # the hook really changed the batch
    assert torch.allclose(c, d, rtol=1e-5, atol=1e-6), (c - d).abs().max()
