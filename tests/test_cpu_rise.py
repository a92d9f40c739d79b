"""No GPU: tests/rise_oracle.py (the restatement the RISE kernels are held to) against torch's bilinear interpolate and the
statistics of its generator, the refusals of the mmskin_rise_* entry points (a status, nothing launched: they run here without
a device), and the Python-side refusals of mmskin.rise.RISE."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import rise_oracle as ro
from mmskin import _lib
from mmskin._lib import MMSkinError
from mmskin.rise import RISE

SHAPES = [(64, 64, 8), (30, 44, 4), (7, 9, 2), (17, 33, 16), (224, 224, 7)]


@pytest.mark.parametrize("H,W,g", SHAPES)
def test_oracle_mask_is_torch_bilinear_upsample_cropped_at_the_shift(H, W, g):
    ch, cw = ro.cell_size(H, W, g)
    shifts = {(0, 0), (ch - 1, cw - 1), (ch // 2, 0), (0, cw // 2)}
    for j in range(3):
        G = ro.cells(11, j, g, 0.5)
        up = torch.nn.functional.interpolate(torch.from_numpy(G)[None, None].double(), size=((g + 1) * ch, (g + 1) * cw), mode="bilinear",
                                             align_corners=False)[0, 0].numpy()
        for dy, dx in sorted(shifts | {ro.shift(11, j, H, W, g)}):
            got = ro.mask_unrounded(G, dy, dx, H, W)
            err = float(np.abs(got - up[dy:dy + H, dx:dx + W]).max())
            assert got.shape == (H, W) and err <= 1e-12, (j, dy, dx, err)
            num, den = ro.mask_exact(G, dy, dx, H, W)
            assert num.min() >= 0 and num.max() <= den < 2 ** 24            # both exact in fp32
    m = ro.mask(11, 0, g, 0.5, H, W)
    assert m.dtype == np.float32 and m.min() >= 0 and m.max() <= 1
    dy, dx = ro.shift(11, 0, H, W, g)
    assert np.abs(m - ro.mask_unrounded(ro.cells(11, 0, g, 0.5), dy, dx, H, W)).max() <= 2.0 ** -25


def test_mix64_is_the_splitmix64_finaliser():
    """the first outputs of splitmix64 seeded with 0 and with 1234567 (Vigna's reference implementation: state += golden
    gamma, then this finaliser; mix64 adds the gamma itself)"""
    assert ro.mix64(0) == 0xE220A8397B1DCDAF
    assert ro.mix64(1234567) == 6457827717110365317


@pytest.mark.parametrize("p1", [0.1, 0.5, 0.9])
def test_generator_on_fraction(p1):
    g, n = 16, 350                                                           # 350 * 289 = 101150 cells
    on = sum(int(ro.cells(5, j, g, p1).sum()) for j in range(n))
    total = n * (g + 1) ** 2
    assert total >= 10 ** 5
    sd = np.sqrt(total * p1 * (1 - p1))
    print(f"p1 {p1}: {on} of {total} on, {abs(on - total * p1) / sd:.2f} standard deviations")
    assert abs(on - total * p1) <= 5 * sd


def test_generator_shifts_and_seeds():
    H, W, g = 64, 44, 8                                                      # ch = 8, cw = 6
    ch, cw = ro.cell_size(H, W, g)
    shifts = np.asarray([ro.shift(3, j, H, W, g) for j in range(2000)])
    assert shifts.min() >= 0 and (shifts[:, 0] < ch).all() and (shifts[:, 1] < cw).all()
    assert set(shifts[:, 0]) == set(range(ch)) and set(shifts[:, 1]) == set(range(cw))
    a = np.stack([ro.cells(3, j, g, 0.5) for j in range(4)])
    assert np.array_equal(a, np.stack([ro.cells(3, j, g, 0.5) for j in range(4)]))
    assert not np.array_equal(a, np.stack([ro.cells(4, j, g, 0.5) for j in range(4)]))
    assert not np.array_equal(a[0], a[1])                                    # two masks of one seed differ too
    assert set(np.unique(a)) == {0, 1}


def test_accumulate_restatement_on_a_hand_case():
    """two masks, two classes: w by hand"""
    logits = np.log(np.array([[0.8, 0.2], [0.5, 0.5]], dtype=np.float64)).astype(np.float32)
    clean = np.log(np.array([[0.3, 0.7]], dtype=np.float64)).astype(np.float32)
    mask_set = np.asarray([[[1.0, 0.5]], [[0.0, 0.25]]], dtype=np.float32)
    out = ro.accumulate(logits, clean, mask_set)
    assert out["target"].tolist() == [1] and abs(out["clean_prob"][0] - 0.7) <= 1e-6
    assert np.allclose(out["saliency_sum"], [[[0.2, 0.1 + 0.125]]], atol=1e-6) and np.allclose(out["coverage"], [[1.0, 0.75]])
    out = ro.accumulate(logits, clean, mask_set, target=[0])
    assert np.allclose(out["saliency_sum"], [[[0.8, 0.4 + 0.125]]], atol=1e-6)


# ------------------------------------------------------------------------------------------------ refusals of the library
def test_bad_arguments_return_a_status_without_launching():
    """No device here: a call that got as far as a launch would fail with a HIP status (2), not an argument status."""
    lib = _lib.load()
    cap = lib.mmskin_faith_max_pixels()
    p = ctypes.c_void_p(4096)                     # never dereferenced: every check comes before the first use
    ARG, UNSUPPORTED = 1, 3

    def refused(rc, status, text):
        assert rc == status, (rc, lib.mmskin_last_error())
        assert text in lib.mmskin_last_error(), lib.mmskin_last_error()

    def masks(j0=0, n=2, grid=4, p1=0.5, H=8, W=8):
        return lib.mmskin_rise_masks(7, j0, n, grid, p1, H, W, p, None)

    def apply(N=2, H=8, W=8, grid=4, p1=0.5, n_masks=5, r0=0, n=4, n_pad=4):
        return lib.mmskin_rise_apply(p, p, N, H, W, 7, grid, p1, n_masks, r0, n, n_pad, p, None)

    def accumulate(N=2, K=6, H=8, W=8, grid=4, p1=0.5, n_masks=5):
        return lib.mmskin_rise_accumulate(p, None, p, N, K, H, W, 7, grid, p1, n_masks, p, p, p, p, p, None)

    for fn in (masks, apply, accumulate):
        refused(fn(grid=1), ARG, b"grid")
        refused(fn(grid=17), ARG, b"grid")
        refused(fn(p1=0.0), ARG, b"p1")
        refused(fn(p1=1.0), ARG, b"p1")
        refused(fn(p1=float("nan")), ARG, b"p1")
        refused(fn(H=0), ARG, b"H")
        refused(fn(W=-3), ARG, b"W")
        refused(fn(H=257, W=256), UNSUPPORTED, b"H * W")
        assert cap == 65536
    for fn in (apply, accumulate):
        refused(fn(N=0), ARG, b"N")
        refused(fn(n_masks=0), ARG, b"n_masks")
        refused(fn(n_masks=(1 << 20) + 1), UNSUPPORTED, b"n_masks")
    refused(apply(n=5, n_pad=4), ARG, b"n_pad")
    refused(apply(n=0), ARG, b"n =")
    refused(apply(n=1, n_pad=0), ARG, b"n_pad")
    refused(apply(r0=7, n=4), ARG, b"r0")                                     # 7 + 4 > 2 * 5
    refused(apply(r0=-1), ARG, b"r0")
    refused(accumulate(K=0), ARG, b"K")
    refused(masks(n=0), ARG, b"n =")
    refused(masks(j0=-1), ARG, b"j0")
    refused(masks(j0=(1 << 20) - 1, n=2), UNSUPPORTED, b"n_masks")
    refused(lib.mmskin_rise_masks(7, 0, 2, 4, 0.5, 8, 8, None, None), ARG, b"null")
    assert lib.mmskin_rise_workspace_bytes(2, 5) == 2 * 5 * 8 + 5 * 80
    assert lib.mmskin_rise_workspace_bytes(0, 5) == -1 and lib.mmskin_rise_workspace_bytes(2, (1 << 20) + 1) == -1


# ------------------------------------------------------------------------------------------------ refusals in Python
class _Plain(nn.Module):
    def forward(self, image, metadata):
        return image.mean(dim=(2, 3)) + metadata[:, :3]


def test_python_side_refusals():
    """every one of these raises before anything touches a device (there is none here)"""
    model = _Plain().eval()
    img, meta = torch.zeros(2, 3, 8, 8), torch.zeros(2, 5)
    with pytest.raises(ValueError, match="baseline"):
        RISE(model, "cpu", baseline="black")
    with pytest.raises(ValueError, match="normalize"):
        RISE(model, "cpu", normalize="max")
    with pytest.raises(ValueError, match="n_masks"):
        RISE(model, "cpu", n_masks=0)
    with pytest.raises(ValueError, match="n_masks"):
        RISE(model, "cpu", n_masks=(1 << 20) + 1)
    with pytest.raises(ValueError, match="grid"):
        RISE(model, "cpu", grid=1)
    with pytest.raises(ValueError, match="p1"):
        RISE(model, "cpu", p1=1.0)
    with pytest.raises(ValueError, match="ksize"):
        RISE(model, "cpu", baseline="blur", blur_ksize=10)
    with pytest.raises(ValueError, match="chunk"):
        RISE(model, "cpu", chunk=0)
    r = RISE(model, "cpu", n_masks=4, grid=2, chunk=4)
    with pytest.raises(ValueError, match="images"):
        r.generate_batch(img[:, :2], meta)
    with pytest.raises(ValueError, match="images"):
        r.generate_batch(img[0], meta)
    with pytest.raises(ValueError, match="image must have shape"):
        r.generate(img, meta)                                               # two images: generate takes one
    with pytest.raises(ValueError, match="metadata"):
        r.generate_batch(img, meta[:1])
    with pytest.raises(ValueError, match="metadata"):
        r.generate_batch(img, {"values": meta, "mask": meta[:1]})
    with pytest.raises(ValueError, match="target_class"):
        r.generate_batch(img, meta, target_class=torch.zeros(3, dtype=torch.long))
    with pytest.raises(MMSkinError, match="cap"):
        r.generate_batch(torch.zeros(1, 3, 257, 256), meta[:1])
    model.train()
    with pytest.raises(MMSkinError, match="eval mode"):
        r.generate_batch(img, meta)
