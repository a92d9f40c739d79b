"""No GPU: tests/faithfulness_oracle.py (the restatement the faithfulness kernels are held to) against independent forms of
the published definitions, the refusals of the mmskin_faith_* entry points (a status, nothing launched: they run here without
a device), and the Python-side refusals of mmskin.faithfulness.CamFaithfulness."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import faithfulness_oracle as fo
from mmskin import _lib
from mmskin._lib import MMSkinError
from mmskin.faithfulness import CamFaithfulness

EPS = 2.0 ** -24


def special_map(H, W, seed=0):
    """a random map with +-0.0, +-inf, repeated values and a few NaNs"""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(H * W).astype(np.float32)
    specials = [0.0, -0.0, np.inf, -np.inf, np.nan, 0.0, -0.0, np.nan, 1.5, 1.5, np.inf, -np.inf]
    for i, v in zip(rng.permutation(H * W), specials):
        s[i] = v
    return s.reshape(1, H, W)


def rank_by_definition(s):
    """rank[p] = #{q : s[q] > s[p]} + #{q < p : s[q] == s[p]} on the floats themselves; a NaN is below every number and equal to
    every NaN"""
    s = np.asarray(s, dtype=np.float32).ravel()
    nan = np.isnan(s)
    out = np.empty(len(s), dtype=np.int32)
    for p in range(len(s)):
        greater = (~nan) if nan[p] else (s > s[p])
        equal = nan if nan[p] else (s == s[p])
        out[p] = int(greater.sum()) + int(equal[:p].sum())
    return out


@pytest.mark.parametrize("H,W", [(1, 1), (5, 3), (9, 11)])
def test_rank_matches_the_definition(H, W):
    rng = np.random.default_rng(1)
    maps = [rng.standard_normal((1, H, W)).astype(np.float32), np.full((1, H, W), 0.25, np.float32),
            np.maximum(rng.standard_normal((1, H, W)) - 1.0, 0).astype(np.float32)]
    if H * W >= 12:
        maps.append(special_map(H, W))
    for s in maps:
        got = fo.rank(s)
        assert got.dtype == np.int32 and got.shape == s.shape
        assert np.array_equal(got.ravel(), rank_by_definition(s))
        assert np.array_equal(np.sort(got.ravel()), np.arange(H * W))          # a permutation: every pixel is touched once
    flat = fo.rank(np.zeros((1, H, W), np.float32))
    assert np.array_equal(flat.ravel(), np.arange(H * W))                      # all ties: row-major order


def test_rank_treats_signed_zeros_as_equal_and_nan_as_lowest():
    s = np.array([[[-0.0, 0.0, np.nan, -np.inf, np.nan, np.inf]]], dtype=np.float32)
    assert fo.rank(s).ravel().tolist() == [1, 2, 4, 3, 5, 0]


@pytest.mark.parametrize("ksize,H,W", [(3, 12, 12), (11, 12, 12), (3, 37, 29), (11, 37, 29), (31, 37, 29), (5, 3, 40)])
def test_blur_matches_conv2d_on_a_reflect_padded_fp64_input(ksize, H, W):
    """Bound (2 ksize + 4) * 2^-24 * max|x|: the fp32 rounding of two passes of ksize products and sums with weights summing to 1
    (the taps themselves are the same fp32 numbers on both sides)."""
    x =torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(ksize))
    taps = fo.gaussian_taps(ksize, 5.0)
    assert taps.dtype == np.float32 and abs(float(taps.astype(np.float64).sum()) - 1) <= ksize * EPS
    got = fo.blur(x.numpy(), taps)
    r = ksize // 2
    t64 = torch.from_numpy(taps.astype(np.float64))
    padded = nn.functional.pad(x.double().reshape(6, 1, H, W), (r, r, r, r), mode="reflect")
    want = nn.functional.conv2d(padded, torch.outer(t64, t64)[None, None]).reshape(2, 3, H, W).numpy()
    err, bound = float(np.abs(got - want).max()), (2 * ksize + 4) * EPS * float(x.abs().max())
    print(f"ksize {ksize} {H}x{W}: max abs diff {err:.3e}, bound {bound:.3e}")
    assert got.dtype == np.float32 and err <= bound


def test_mean_fill_is_the_plane_mean():
    x = np.random.default_rng(2).standard_normal((2, 3, 37, 29)).astype(np.float32)
    got = fo.mean_fill(x)
    want = x.astype(np.float64).mean(axis=(2, 3))
    assert got.shape == x.shape and np.array_equal(got, np.broadcast_to(got[:, :, :1, :1], x.shape))
    assert np.abs(got[:, :, 0, 0] - want).max() <= EPS * np.abs(want).max() + 37 * 29 * 2.0 ** -53 * np.abs(x).max()


@pytest.mark.parametrize("S", [1, 8, 32])
def test_trapezoid_matches_numpy(S):
    curve = np.random.default_rng(S).random(S + 1)
    trapz = getattr(np, "trapezoid", None) or np.trapz
    assert abs(fo.trapezoid(curve) - trapz(curve, np.arange(S + 1) / S)) <= 1e-14


def test_curve_end_points_are_the_image_and_the_baseline():
    """deletion k = 0 and insertion k = S are the unmodified image, deletion k = S and insertion k = 0 the baseline; every step
    is a pure select, and step k touches exactly (k * H * W) // S pixels"""
    rng = np.random.default_rng(3)
    N, H, W, S = 2, 7, 5, 4
    img = rng.standard_normal((N, 3, H, W)).astype(np.float32)
    sal = np.maximum(rng.standard_normal((N, H, W)), 0).astype(np.float32)
    for baseline in ("blur", "zero", "mean"):
        base = fo.baseline_images(img, baseline, ksize=3, sigma=1.0)
        rows = fo.perturbed_rows(img, sal, S, baseline, ksize=3, sigma=1.0).reshape(N, 2 * S + 3, 3, H, W)
        assert np.array_equal(rows[:, 0], img) and np.array_equal(rows[:, 2 * S + 1], img)
        assert np.array_equal(rows[:, S], base) and np.array_equal(rows[:, S + 1], base)
        for k in range(S + 1):
            dele, ins = rows[:, k], rows[:, S + 1 + k]
            assert ((dele == img) | (dele == base)).all() and ((ins == img) | (ins == base)).all()
            if baseline == "zero":
                touched = (dele[:, 0] != img[:, 0]).reshape(N, -1).sum(axis=1)
                assert (touched == (k * H * W) // S).all()
        h = np.clip(sal, 0, 1)[:, None]
        assert np.abs(rows[:, 2 * S + 2] - (base + h * (img - base))).max() <= 4 * EPS * np.abs(img).max()


def test_curves_restatement_on_a_hand_case():
    """two classes, S = 1: probabilities by hand"""
    logits = np.log(np.array([[0.8, 0.2], [0.1, 0.9], [0.3, 0.7], [0.8, 0.2], [0.9, 0.1]], dtype=np.float64)).astype(np.float32)
    out = fo.curves(logits, 1, 1)
    assert out["target"].tolist() == [0]
    assert np.allclose(out["deletion"], [[0.8, 0.1]], atol=1e-6) and np.allclose(out["insertion"], [[0.3, 0.8]], atol=1e-6)
    assert abs(out["deletion_auc"][0] - 0.45) <= 1e-6 and abs(out["insertion_auc"][0] - 0.55) <= 1e-6
    assert out["average_drop"][0] == 0 and out["increase"][0] == 1 and out["mean_increase"] == 1
    out = fo.curves(logits, 1, 1, target=[1])
    assert np.allclose(out["deletion"], [[0.2, 0.9]], atol=1e-6)
    assert abs(out["average_drop"][0] - 0.5) <= 1e-6 and out["increase"][0] == 0


# ------------------------------------------------------------------------------------------------ refusals of the library
def test_bad_arguments_return_a_status_without_launching():
    """No device here: a call that got as far as a launch would fail with a HIP status (2), not an argument status."""
    lib = _lib.load()
    cap = lib.mmskin_faith_max_pixels()
    assert cap >= 240 * 240
    p = ctypes.c_void_p(4096)                     # never dereferenced: every check comes before the first use
    taps = (ctypes.c_float * 31)(*([1.0 / 31] * 31))
    ARG, UNSUPPORTED = 1, 3

    def refused(rc, status, text):
        assert rc == status, (rc, lib.mmskin_last_error())
        assert text in lib.mmskin_last_error(), lib.mmskin_last_error()

    refused(lib.mmskin_faith_rank(p, 0, 16, p, None), ARG, b"extent")
    refused(lib.mmskin_faith_rank(p, 1, 0, p, None), ARG, b"extent")
    refused(lib.mmskin_faith_rank(p, 1, cap + 1, p, None), UNSUPPORTED, b"cap")
    refused(lib.mmskin_faith_blur(p, 0, 8, 8, taps, 3, p, None), ARG, b"extent")
    refused(lib.mmskin_faith_blur(p, 3, 8, 0, taps, 3, p, None), ARG, b"extent")
    refused(lib.mmskin_faith_blur(p, 3, 8, 8, taps, 4, p, None), ARG, b"odd")
    refused(lib.mmskin_faith_blur(p, 3, 64, 64, taps, 33, p, None), ARG, b"at most 31")
    refused(lib.mmskin_faith_blur(p, 3, 8, 5, taps, 11, p, None), ARG, b"reflect")
    refused(lib.mmskin_faith_mean(p, 0, 8, p, None), ARG, b"extent")
    refused(lib.mmskin_faith_mean(p, 3, 0, p, None), ARG, b"extent")
    perturb = lambda N, H, W, S, n, n_pad: lib.mmskin_faith_perturb(p, p, p, p, p, N, H, W, S, n, n_pad, p, None)   # noqa: E731
    refused(perturb(0, 8, 8, 4, 1, 1), ARG, b"extent")
    refused(perturb(1, 0, 8, 4, 1, 1), ARG, b"extent")
    refused(perturb(1, 8, 8, 0, 1, 1), ARG, b"steps")
    refused(perturb(1, 64, 64, 1025, 1, 1), ARG, b"steps")
    refused(perturb(1, 4, 4, 17, 1, 1), ARG, b"steps")                          # S > H * W
    refused(perturb(1, 257, 256, 4, 1, 1), UNSUPPORTED, b"cap")
    refused(perturb(1, 8, 8, 4, 0, 4), ARG, b"padded")
    refused(perturb(1, 8, 8, 4, 5, 4), ARG, b"padded")                          # n > chunk
    curves = lambda N, S, C: lib.mmskin_faith_curves(p, None, N, S, C, p, p, p, p, None)                           # noqa: E731
    refused(curves(0, 4, 2), ARG, b"extent")
    refused(curves(1, 4, 0), ARG, b"extent")
    refused(curves(1, 0, 2), ARG, b"steps")
    refused(curves(1, 1025, 2), ARG, b"steps")
    refused(lib.mmskin_faith_rank(None, 1, 16, p, None), ARG, b"null")


# ------------------------------------------------------------------------------------------------ refusals in Python
class _Plain(nn.Module):
    def forward(self, image, metadata):
        return image.mean(dim=(2, 3)) + metadata[:, :3]


def test_python_side_refusals():
    model = _Plain().eval()
    img, meta, sal = torch.zeros(2, 3, 8, 8), torch.zeros(2, 5), torch.zeros(2, 8, 8)
    with pytest.raises(ValueError, match="steps"):
        CamFaithfulness(model, "cpu", steps=0)
    with pytest.raises(ValueError, match="steps"):
        CamFaithfulness(model, "cpu", steps=1025)
    with pytest.raises(ValueError, match="baseline"):
        CamFaithfulness(model, "cpu", baseline="black")
    with pytest.raises(ValueError, match="ksize"):
        CamFaithfulness(model, "cpu", blur_ksize=10)
    with pytest.raises(ValueError, match="chunk"):
        CamFaithfulness(model, "cpu", chunk=0)
    f = CamFaithfulness(model, "cpu", steps=8, chunk=4)
    with pytest.raises(ValueError, match="images"):
        f.evaluate(img[:, :2], meta, sal)
    with pytest.raises(ValueError, match="saliency"):
        f.evaluate(img, meta, sal[:1])
    with pytest.raises(ValueError, match="saliency"):
        f.evaluate(img, meta, torch.zeros(2, 8, 7))
    with pytest.raises(ValueError, match="saliency"):
        f.evaluate(img, meta, np.zeros((2, 8, 8), dtype=np.int64))
    with pytest.raises(ValueError, match="metadata"):
        f.evaluate(img, meta[:1], sal)
    with pytest.raises(ValueError, match="metadata"):
        f.evaluate(img, {"values": meta, "mask": meta[:1]}, sal)
    with pytest.raises(ValueError, match="target_class"):
        f.evaluate(img, meta, sal, target_class=torch.zeros(3, dtype=torch.long))
    with pytest.raises(ValueError, match="steps"):
        CamFaithfulness(model, "cpu", steps=65).evaluate(img, meta, sal)           # S > H * W
    with pytest.raises(MMSkinError, match="cap"):
        f.evaluate(torch.zeros(1, 3, 257, 256), meta[:1], torch.zeros(1, 257, 256))
    model.train()
    with pytest.raises(MMSkinError, match="eval mode"):
        f.evaluate(img, meta, sal)


def test_row_table_matches_the_restatement():
    f = CamFaithfulness(_Plain().eval(), "cpu", steps=5, baseline="zero")
    assert np.array_equal(f.row_table(3), fo.row_table(3, 5))
