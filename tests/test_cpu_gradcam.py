"""CPU: the torch restatement of the Grad-CAM kernels (tests/gradcam_oracle.py) against the golden recorded from the reference's
own classes (tests/golden/gen_gradcam_golden.py), and the properties the kernels are then held to on the GPU
(tests/test_gpu_gradcam.py): a flat map gives zeros, normalisation comes before the upsample, every row is normalised on its
own, rows find their image through row_image."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import gradcam_oracle as go
from helpers import GOLDEN, SMALL
from oracle.detinit import det_init_
from oracle.model import OracleMultimodalModel

F64 = torch.float64


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "gradcam_resnet18.npz"))


@pytest.fixture(scope="module")
def traced(gold):
    """The golden's model and rows, run once at batch R with hooks on the last conv and on the encoder: activations A, the
    gradient of every row's target logit at A, J = d sum(features) / dA and dfeat = d logit / d features."""
    model = det_init_(OracleMultimodalModel(**dict(SMALL, cnn_model_name="resnet-18", attention_mecanism="concatenation"))).eval()
    n, v, size = int(gold["n_images"]), int(gold["variants"]), int(gold["size"])
    img, meta = go.det_rows(n, size, v)
    conv = [m for m in model.image_encoder.modules() if isinstance(m, nn.Conv2d)][-1]
    store = {}
    hooks = [conv.register_forward_hook(lambda mod, i, o: store.__setitem__("acts", o)),
             model.image_encoder.register_forward_hook(lambda mod, i, o: store.__setitem__("feats", o))]
    try:
        logits = model(img.repeat_interleave(v, dim=0).requires_grad_(True), meta)
    finally:
        for h in hooks:
            h.remove()
    acts, feats = store["acts"], store["feats"]
    selected = logits.gather(1, torch.from_numpy(gold["targets"])[:, None]).sum()
    grads, dfeat = torch.autograd.grad(selected, (acts, feats), retain_graph=True)
    jac, = torch.autograd.grad(feats.sum(), acts)
    return dict(logits=logits.detach(), acts=acts.detach(), grads=grads, jac=jac, dfeat=dfeat.reshape(n * v, -1), n=n, v=v, size=size)


@pytest.mark.parametrize("mode,key", [(1, "plusplus_maps"), (0, "gradcam_maps")])
def test_fp64_restatement_reproduces_the_reference_golden(gold, traced, mode, key):
    """The reference computes in fp32; the restatement gets the same fp32 activations and gradients and computes in fp64.
    What separates them is the reference's own float arithmetic on a [0, 1] map: the fp32 restatement differs from the fp64 one
    by about 1e-6 here, and 2e-5 leaves room for the min-max division to stretch that.  Both forms of the gradient: the
    tensor autograd returns, and jac * dfeat through row_image (rows of one image share its activations)."""
    if key not in gold.files:
        pytest.skip("the reference's plain GradCAM did not load when the fixture was recorded: pinned on the restatement alone")
    t = traced
    R = t["n"] * t["v"]
    assert np.array_equal(t["logits"].argmax(dim=1).numpy(), gold["targets"])
    assert torch.allclose(t["logits"], torch.from_numpy(gold["logits"]), rtol=1e-5, atol=1e-6)
    want = torch.from_numpy(gold[key]).double()
    size = (t["size"], t["size"])
    generic = go.explain(t["acts"], t["grads"], None, torch.arange(R), mode, size, F64)[2]
    print(f"mode {mode}: max |fp64 restatement - reference| {float((generic - want).abs().max()):.3e}")
    assert float((generic - want).abs().max()) < 2e-5
    row_image = torch.arange(t["n"]).repeat_interleave(t["v"])
    one_per_image = t["acts"][::t["v"]].contiguous()
    assert torch.equal(one_per_image[row_image], t["acts"])             # the activations do not depend on the metadata
    factored = go.explain(one_per_image, t["jac"][::t["v"]].contiguous(), t["dfeat"], row_image, mode, size, F64)[2]
    print(f"mode {mode}: max |jac * dfeat form - reference| {float((factored - want).abs().max()):.3e}")
    assert float((factored - want).abs().max()) < 2e-5


def test_a_flat_map_gives_zeros_not_nan():
    for raw in (torch.full((2, 3, 3), 0.37), torch.full((1, 1, 1), 5.0), torch.full((1, 2, 2), -1.0), torch.zeros(1, 2, 2)):
        for dtype in (torch.float32, F64):
            cam = go.cam(raw, (8, 9), dtype)
            assert cam.shape == (raw.shape[0], 8, 9) and not cam.any()


def test_normalisation_comes_before_the_upsample():
    """A map with negative values: ReLU before the interpolation keeps them from pulling their neighbours down, ReLU after it
    does not.  (Without negative values the two orders agree: the edge clamp of align_corners=False reproduces the source's
    minimum and maximum in the corners.)"""
    raw = torch.tensor([[[-4.0, 1.0], [0.5, 2.0]]])
    first = go.cam(raw, (8, 8), F64)
    other = go.cam_upsample_first(raw, (8, 8), F64)
    assert float((first - other).abs().max()) > 0.1
    # by hand: relu -> [0, 1; 0.5, 2], min 0, max 2 -> [0, 0.5; 0.25, 1]; the corners of the upsampled map are the source corners
    assert torch.allclose(first[0, [0, 0, -1, -1], [0, -1, 0, -1]], torch.tensor([0.0, 0.5, 0.25, 1.0], dtype=F64), atol=1e-7)
    assert float(first[0, 0, 3]) == pytest.approx(0.375 * 0.5, abs=1e-7)      # src x = 3.5 * (2 / 8) - 0.5 = 0.375 between 0 and 0.5
    positive = torch.tensor([[[0.25, 1.0], [0.5, 2.0]]])
    assert torch.allclose(go.cam(positive, (8, 8), F64), go.cam_upsample_first(positive, (8, 8), F64), atol=1e-7)


def test_every_row_is_normalised_on_its_own():
    g = torch.Generator().manual_seed(0)
    raw = torch.rand(3, 4, 5, generator=g) * torch.tensor([1.0, 1e3, 1e-3])[:, None, None]
    cam, norm = go.cam(raw, (9, 11), F64), go.normalise(raw.double())
    for r in range(3):
        # 1e-8 in the denominator: the row scaled by 1e-3 tops out at 1 - 1e-5, not at 1
        assert float(norm[r].max()) == pytest.approx(1.0, abs=2e-5) and float(norm[r].min()) == 0.0
        assert float(cam[r].max()) > 0.8                  # with the batch's range the 1e-3 row would stay below 1e-5
        assert torch.equal(cam[r], go.cam(raw[r:r + 1], (9, 11), F64)[0])


@pytest.mark.parametrize("mode", [0, 1])
def test_rows_find_their_image_through_row_image(mode):
    """rows that share an image, in non-monotone order, and out-of-range entries clamped to the nearest image"""
    g = torch.Generator().manual_seed(1)
    N, C, fh, fw = 3, 6, 3, 2
    acts, jac = torch.rand(N, C, fh, fw, generator=g), torch.rand(N, C, fh, fw, generator=g)
    row_image = torch.tensor([2, 0, 2, 1, 0], dtype=torch.int32)
    dfeat = torch.rand(5, C, generator=g)
    w, raw, cam = go.explain(acts, jac, dfeat, row_image, mode, (6, 4), F64)
    for r, n in enumerate(row_image.tolist()):
        grads = (jac[n].double() * dfeat[r].double()[:, None, None])[None]
        w1, raw1, cam1 = go.explain(acts[n:n + 1], grads, None, torch.zeros(1, dtype=torch.int32), mode, (6, 4), F64)
        assert torch.allclose(w[r], w1[0], rtol=1e-12, atol=0) and torch.allclose(raw[r], raw1[0], rtol=1e-12, atol=0)
        assert torch.allclose(cam[r], cam1[0], rtol=1e-12, atol=1e-15)
    wild = torch.tensor([7, -3, 2, 1, 0], dtype=torch.int32)
    for a, b in zip(go.explain(acts, jac, dfeat, wild, mode, (6, 4), F64), go.explain(acts, jac, dfeat, row_image, mode, (6, 4), F64)):
        assert torch.equal(a, b)
