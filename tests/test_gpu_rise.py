"""-m gpu: mmskin.rise end to end.  The setup of tests/test_gpu_faithfulness.py (resnet-18 + one-hot metadata + crossattention,
fp32 backbone, 64x64 images, N = 2) with n_masks = 40, grid = 4 and chunk = 16, which does not divide the 80 rows:
RISE.generate_batch against a loop that runs the restatement's masked rows (tests/rise_oracle.py) through the same model at the
same chunk size and then the restatement's sums.

Tolerance.  Both sides feed the model bit-identical inputs, so a weight w[n][j] moves by at most tol_j, that file's
probability_tolerance of row j's logits; the map is sum_j w_j m_j(p) / (n_masks p1) with m >= 0, so pixel p moves by at most
sum_j tol_j m_j(p) / (n_masks p1), plus 1e-6 for the fp32 rounding of a map of order 1."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import rise_oracle as ro
from gpu_util import DEV
from helpers import SMALL
from mmskin.faithfulness import CamFaithfulness
from mmskin.rise import RISE, RiseResult, rise_maps
from oracle.detinit import det_inputs, det_tensor
from test_gpu_faithfulness import hip_model, loop_logits, probability_tolerance

pytestmark = pytest.mark.gpu

N, SIZE, NM, GRID, CHUNK, P1, SEED = 2, 64, 40, 4, 16, 0.5, 0


@pytest.fixture(scope="module")
def setup():
    model = hip_model(**dict(SMALL, cnn_model_name="resnet-18", attention_mecanism="crossattention"))
    img, meta, _ = det_inputs(N, SIZE, 20, 6)
    with torch.no_grad():
        clean = model(img.to(DEV), meta.to(DEV)).float().cpu().numpy()
    return {"model": model, "img": img, "meta": meta, "clean": clean}


def loop_reference(model, img, meta, clean, n_masks, grid, chunk, baseline="zero", seed=SEED):
    """the restatement's rows through the same model -> (logits [N * n_masks, K], mask set, tol [N, H, W] of the "expected" map)"""
    n = img.shape[0]
    rows, mask_set = ro.masked_rows(img.numpy(), seed, grid, P1, n_masks, baseline)
    logits = loop_logits(model, rows, np.repeat(np.arange(n), n_masks), meta, chunk)
    tol_rows = probability_tolerance(logits).reshape(n, n_masks)
    tol = np.einsum("nj,jhw->nhw", tol_rows, mask_set.astype(np.float64)) / (n_masks * P1) + 1e-6
    return logits, mask_set, tol


@pytest.fixture(scope="module")
def reference(setup):
    """the loop's logits on the zero baseline, computed once"""
    logits, mask_set, tol = loop_reference(setup["model"], setup["img"], setup["meta"], setup["clean"], NM, GRID, CHUNK)
    return {"logits": logits, "masks": mask_set, "tol": tol}


def run(setup, target=None, **kw):
    kw = dict(dict(n_masks=NM, grid=GRID, p1=P1, seed=SEED, chunk=CHUNK), **kw)
    return RISE(setup["model"], DEV, **kw).generate_batch(setup["img"].to(DEV), setup["meta"].to(DEV), target)


def check_against(res, want, tol, n_masks=NM):
    got = res.saliency.numpy()
    err = np.abs(got - want["saliency_sum"] / (n_masks * P1))
    print(f"saliency: max error {err.max():.3e}, smallest tolerance {tol.min():.3e}, largest {tol.max():.3e}")
    assert got.dtype == np.float32 and got.shape == want["saliency_sum"].shape and np.isfinite(got).all()
    assert (err <= tol).all()
    assert np.abs(res.coverage.numpy() - want["coverage"]).max() <= 1e-10 * n_masks     # no model in it: the restatement's, to fp64


def test_generate_batch_matches_a_loop_through_the_same_model(setup, reference):
    res = run(setup)
    assert isinstance(res, RiseResult) and res.saliency.is_cuda and res.saliency.dtype == torch.float32
    assert res.saliency_sum.dtype == res.coverage.dtype == res.clean_prob.dtype == torch.float64 and res.target.dtype == torch.int32
    assert tuple(res.saliency.shape) == (N, SIZE, SIZE) and tuple(res.coverage.shape) == (SIZE, SIZE)
    again = run(setup)
    assert torch.equal(res.saliency_sum, again.saliency_sum) and torch.equal(res.coverage, again.coverage)     # bitwise repeatable
    res = res.cpu()
    want = ro.accumulate(reference["logits"], setup["clean"], reference["masks"])
    assert res.target.tolist() == want["target"].tolist() == setup["clean"].argmax(axis=1).tolist()             # the clean argmax
    assert (np.abs(res.clean_prob.numpy() - want["clean_prob"]) <= probability_tolerance(setup["clean"])).all()
    check_against(res, want, reference["tol"])
    assert np.abs(res.saliency.numpy() - (res.saliency_sum.numpy() / (NM * P1)).astype(np.float32)).max() <= 1e-7


@pytest.mark.parametrize("target", [3, "tensor"])
def test_given_targets_are_honoured(setup, reference, target):
    classes = [3, 3] if target == 3 else [4, 1]
    given = 3 if target == 3 else torch.tensor(classes, device=DEV)
    res = run(setup, target=given).cpu()
    assert res.target.tolist() == classes
    check_against(res, ro.accumulate(reference["logits"], setup["clean"], reference["masks"], classes), reference["tol"])
    with pytest.raises(ValueError, match="outside"):
        run(setup, target=6)


@pytest.mark.parametrize("baseline", ["blur", "mean"])
def test_other_baselines_against_the_loop(setup, baseline):
    logits, mask_set, tol = loop_reference(setup["model"], setup["img"], setup["meta"], setup["clean"], NM, GRID, CHUNK, baseline)
    res = run(setup, baseline=baseline).cpu()
    check_against(res, ro.accumulate(logits, setup["clean"], mask_set, res.target.tolist()), tol)


def test_coverage_normalisation(setup):
    res = run(setup, normalize="coverage").cpu()
    assert (res.coverage.numpy() > 0).all()
    want = (res.saliency_sum.numpy() / res.coverage.numpy()[None]).astype(np.float32)
    assert np.abs(res.saliency.numpy() - want).max() <= 1e-7
    assert (res.saliency.numpy() >= 0).all() and (res.saliency.numpy() <= 1).all()        # a weighted mean of probabilities


def test_generate_single_image(setup):
    rise = RISE(setup["model"], DEV, n_masks=NM, grid=GRID, chunk=CHUNK)
    heat = rise.generate(setup["img"][:1].to(DEV), setup["meta"][:1].to(DEV))
    assert isinstance(heat, np.ndarray) and heat.shape == (SIZE, SIZE) and heat.dtype == np.float32
    assert np.isfinite(heat).all() and heat.min() == 0 and 0.99 <= heat.max() <= 1


class _Rectangle(nn.Module):
    """class 1 = the mean of rows 12 .. 19, columns 8 .. 15 of the image; class 0 constant"""
    Y0, Y1, X0, X1 = 12, 20, 8, 16

    def forward(self, image, metadata):
        s = image[:, :, self.Y0:self.Y1, self.X0:self.X1].mean(dim=(1, 2, 3))
        return torch.stack([torch.zeros_like(s), s], dim=1)


def test_the_map_peaks_where_the_model_looks():
    """a mask paired with another mask's forward (or another image's) loses this.  normalize="coverage": with 256 masks the
    coverage itself varies by several per cent from pixel to pixel, as much as the signal; the restatement run on this model puts
    the maximum inside the rectangle for every one of seeds 0 .. 11 under "coverage" and for about half of them under "expected"."""
    model = _Rectangle().to(DEV).eval()
    img = torch.full((2, 3, 32, 32), 4.0)
    img[1] += det_tensor("rise.rect", (3, 32, 32)).abs()
    res = RISE(model, DEV, n_masks=256, grid=4, baseline="zero", normalize="coverage", seed=1, chunk=100).generate_batch(img.to(DEV), torch.zeros(2, 1), 1)
    sal = res.saliency.cpu().numpy()
    inside = np.zeros((32, 32), dtype=bool)
    inside[_Rectangle.Y0:_Rectangle.Y1, _Rectangle.X0:_Rectangle.X1] = True
    for n in range(2):
        y, x = np.unravel_index(int(sal[n].argmax()), sal[n].shape)
        print(f"image {n}: maximum at ({y}, {x}), mean inside {sal[n][inside].mean():.4f}, outside {sal[n][~inside].mean():.4f}")
        assert inside[y, x] and sal[n][inside].mean() > sal[n][~inside].mean()


class _EncoderWithHead(nn.Module):
    """an image encoder that returns features [B, F], a linear head and a metadata term: called as model(images, metadata)"""

    def __init__(self, encoder, features, classes=6):
        super().__init__()
        self.encoder = encoder
        self.head = nn.Linear(features, classes)

    def forward(self, image, metadata):
        return self.head(self.encoder(image)) + metadata[:, :self.head.out_features]


def test_a_transformer_encoder_without_a_target_layer():
    """swin_tiny at 128x128 with window 4, the smallest transformer tests/test_gpu_swin.py builds: no layer of it delivers a
    (C, fh, fw) convolutional map, so no CAM class explains it"""
    from models.hip_swin import HipSwinTransformer
    from oracle.detinit import det_init_
    from swin_oracle import OracleSwin
    name, kw = "swin_tiny_patch4_window7_224", {"img_size": 128, "window_size": 4}
    torch.manual_seed(0)                                                     # the head's own initialisation
    enc = HipSwinTransformer(name, drop_path_rate=0.0, **kw)
    enc.load_state_dict(det_init_(OracleSwin(name, **kw)).state_dict(), strict=True)
    model = _EncoderWithHead(enc, 768).to(DEV).eval()
    img, meta = det_tensor("rise.swin.x", (1, 3, 128, 128)), det_tensor("rise.swin.m", (1, 6))
    with torch.no_grad():
        clean = model(img.to(DEV), meta.to(DEV)).float().cpu().numpy()
    n_masks, chunk = 8, 8
    logits, mask_set, tol = loop_reference(model, img, meta, clean, n_masks, 8, chunk, seed=5)
    res = RISE(model, DEV, n_masks=n_masks, grid=8, seed=5, chunk=chunk).generate_batch(img.to(DEV), meta.to(DEV)).cpu()
    assert tuple(res.saliency.shape) == (1, 128, 128) and res.target.tolist() == clean.argmax(axis=1).tolist()
    check_against(res, ro.accumulate(logits, clean, mask_set), tol, n_masks)


def test_rise_maps_feed_the_scorer(setup):
    img, meta = setup["img"].to(DEV), setup["meta"].to(DEV)
    maps = rise_maps(setup["model"], img, meta, None, n_masks=NM, grid=GRID, chunk=CHUNK)
    assert maps.is_cuda and maps.dtype == torch.float32 and tuple(maps.shape) == (N, SIZE, SIZE)
    res = CamFaithfulness(setup["model"], DEV, steps=8, chunk=CHUNK).evaluate(img, meta, maps).cpu()
    assert res.target.tolist() == setup["clean"].argmax(axis=1).tolist()
    for field in ("deletion", "insertion", "deletion_auc", "insertion_auc", "average_drop", "increase"):
        v = getattr(res, field).numpy()
        assert np.isfinite(v).all() and (v >= 0).all() and (v <= 1).all(), field
