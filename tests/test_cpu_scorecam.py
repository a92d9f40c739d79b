"""No GPU: tests/scorecam_oracle.py (the numpy restatement the Score-CAM kernels are held to bit for bit) against
torch.nn.Upsample on the CPU and against a golden recorded from the reference's own ScoreCAM class
(tests/golden/gen_scorecam_golden.py)."""
import os

import numpy as np
import pytest
import torch

import scorecam_oracle as so
from helpers import GOLDEN

EPS = 2.0 ** -24
SHAPES = [(5, 7, 7, 224, 224), (5, 5, 3, 37, 29), (3, 1, 1, 9, 9), (4, 4, 4, 4, 4), (2, 2, 3, 64, 96)]


def nonneg_fmap(C, fh, fw, seed=0):
    """relu(randn) with a zero in the top-left corner of every channel: the edge clamp reproduces that sample exactly, so the
    upsampled minimum is 0"""
    g = torch.Generator().manual_seed(seed)
    f = torch.relu(torch.randn(C, fh, fw, generator=g))
    f[:, 0, 0] = 0
    return f


def torch_upsample(f, size):
    return torch.nn.Upsample(size=size, mode="bilinear")(f[None])[0]


@pytest.mark.parametrize("C,fh,fw,H,W", SHAPES)
def test_upsample_matches_torch(C, fh, fw, H, W):
    """Before normalisation, within 16 * 2^-24 * max|f|: the handful of fp32 products, differences and sums of a convex
    combination on either side, plus the fp32 source coordinate.  Equal sizes: the copy is exact."""
    f = nonneg_fmap(C, fh, fw) + (0.25 if fh * fw == 1 else 0)
    want = torch_upsample(f, (H, W)).numpy()
    got = so.upsample(f.numpy(), (H, W))
    err = float(np.abs(got - want).max())
    bound = 16 * EPS * float(f.abs().max())
    print(f"{fh}x{fw}->{H}x{W}: max abs diff {err:.3e}, bound {bound:.3e}")
    assert got.dtype == np.float32 and got.shape == (C, H, W)
    assert err <= bound
    if (fh, fw) == (H, W):
        assert err == 0 and np.array_equal(got, f.numpy())


@pytest.mark.parametrize("C,fh,fw,H,W", SHAPES)
def test_normalised_maps_match_torch(C, fh, fw, H, W):
    """After normalisation the bound is divided by max - min of the upsampled map (inputs are non-negative with a zero the
    upsample reproduces, so the minimum is 0).  A flat channel gives zeros, as ScoreCam.py:117-121."""
    f = nonneg_fmap(C, fh, fw, seed=1)
    if C >= 3:
        f[1] = 0.7                                     # a constant channel -> all zeros
    up = torch_upsample(f, (H, W))
    got = so.cams(f.numpy(), (H, W))
    for c in range(C):
        mn, mx = up[c].min(), up[c].max()
        if f[c].max() == f[c].min():
            # a constant channel is flat.  torch's own upsample keeps it exactly constant only where its kernel fuses
            # (1 - l) * a + l * a (observed: exact at 7x7 -> 224x224, one ulp of noise at 5x3 -> 37x29 and 1x1 -> 9x9,
            # which the reference's normalisation would stretch to [0, 1]); the restatement's difference form always does
            assert not got[c].any()
            continue
        want = ((up[c] - mn) / (mx - mn)).numpy()
        bound = 16 * EPS * float(f[c].abs().max()) / float(mx - mn)
        err = float(np.abs(got[c] - want).max())
        print(f"{fh}x{fw}->{H}x{W} channel {c}: max abs diff {err:.3e}, bound {bound:.3e}")
        assert err <= bound
        assert got[c].min() == 0 and got[c].max() == 1


def test_minmax_is_of_the_upsampled_map_not_of_the_source():
    f = torch.relu(torch.randn(8, 7, 7, generator=torch.Generator().manual_seed(2))).numpy()
    mm = so.minmax(f, (224, 224))
    up = torch_upsample(torch.from_numpy(f), (224, 224)).numpy()
    assert np.abs(mm[:, 1] - up.max(axis=(1, 2))).max() <= 16 * EPS * f.max()
    assert (mm[:, 1] < f.max(axis=(1, 2))).all()       # no output pixel lands on a source sample
    f[0, 0, 0] = 9.0                                   # ... except through the edge clamp: a corner maximum is reproduced exactly
    assert so.minmax(f, (224, 224))[0, 1] == np.float32(9.0)


def test_mask_pads_with_zero_rows_and_zeroes_flat_channels():
    g = torch.Generator().manual_seed(3)
    f = torch.randn(5, 5, 3, generator=g).numpy()
    f[2] = -1.5
    img = torch.randn(3, 37, 29, generator=g).numpy()
    out = so.mask(f, img, 1, 3, 4)
    cam = so.cams(f, (37, 29))
    assert out.shape == (4, 3, 37, 29) and out.dtype == np.float32
    assert np.array_equal(out[0], img * cam[1][None]) and np.array_equal(out[2], img * cam[3][None])
    assert not out[1].any() and not out[3].any()        # channel 2 is flat; row 3 is padding


def test_reproduces_the_reference_heat_map():
    """The restatement fed the golden's own features and scores gives the reference's heat map.  Cams lie in [0, 1] and scores
    are >= 0, so every partial sum is <= sum(scores) and each of the C steps of either side rounds by at most 2^-24 of that;
    the normalisation divides by max - min of the un-normalised sum."""
    gold = np.load(os.path.join(GOLDEN, "scorecam_resnet18.npz"))
    fmap, scores, heat = gold["fmap"], gold["scores"], gold["heat"]
    C = fmap.shape[0]
    assert fmap.shape == (512, 2, 2) and scores.shape == (512,) and heat.shape == (64, 64) and (scores >= 0).all()
    probs = torch.softmax(torch.from_numpy(gold["logits"]), dim=1)[:, int(gold["target_class"])].numpy()
    assert np.array_equal(probs, scores)
    raw = so.combine_raw(fmap, scores, (64, 64))
    bound = 4 * C * EPS * float(scores.sum()) / float(raw.max() - raw.min())
    err = float(np.abs(so.combine(fmap, scores, (64, 64)) - heat).max())
    print(f"heat map vs reference: max abs diff {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert heat.min() == 0 and heat.max() == 1
