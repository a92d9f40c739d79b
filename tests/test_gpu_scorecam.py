"""-m gpu: the Score-CAM kernels (csrc/scorecam.hip) bit for bit against their numpy restatement (tests/scorecam_oracle.py, held
to torch and to the reference by tests/test_cpu_scorecam.py), and mmskin.cam.ScoreCAM end to end on the HIP model against
the golden recorded from the reference's own class."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import scorecam_oracle as so
from gpu_util import DEV
from helpers import GOLDEN, SMALL
from mmskin import _lib, ops
from mmskin._lib import MMSkinError, ptr, stream
from mmskin.cam import ScoreCAM
from models import multimodalIntraInterModal as M
from oracle.detinit import det_init_, det_inputs
from oracle.model import OracleMultimodalModel

pytestmark = pytest.mark.gpu

# (C, fh, fw, H, W): production scale 32; odd sizes, non-integer scale, partial tiles; one source pixel (every channel flat);
# scale 1; a 2x3 map; C = 1; and 21 channels so that a chunk spans several of the mask kernel's 8-row groups
SHAPES = [(5, 7, 7, 224, 224), (5, 5, 3, 37, 29), (3, 1, 1, 9, 9), (4, 4, 4, 4, 4), (2, 2, 3, 64, 96), (1, 7, 7, 224, 224),
          (21, 3, 3, 20, 24)]
SENTINEL = -77.0


def make_fmap(C, fh, fw, seed=0):
    """relu(randn); channel 0 has its maximum in the top-left corner (the edge clamp reproduces it exactly), channel 1 is
    constant, channel 2 has negative values"""
    g = torch.Generator().manual_seed(seed)
    f = torch.relu(torch.randn(C, fh, fw, generator=g))
    f[0, 0, 0] = 7.5
    if C > 1:
        f[1] = 0.7
    if C > 2:
        f[2] = torch.randn(fh, fw, generator=g) - 1.0
    return f


def chunks(C):
    """(c0, n, n_pad): the whole map, and a ragged chunk that starts past channel 0"""
    out = [(0, C, C), (min(1, C - 1), min(3, max(C - 1, 1)), 4)]
    if C > 16:
        out.append((2, C - 2, 32))       # three live 8-row groups (the last one partly padding) and one that is all padding
    return out


def equal_bits(got, want):
    """same values element for element (a -0.0 of the kernel equals the restatement's 0.0: no bit pattern is compared for zero)"""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("C,fh,fw,H,W", SHAPES)
def test_minmax_and_mask_match_the_restatement(C, fh, fw, H, W):
    f = make_fmap(C, fh, fw)
    img = torch.randn(3, H, W, generator=torch.Generator().manual_seed(1))
    fd, imgd = f.to(DEV), img.to(DEV)
    mm = ops.scorecam_minmax(fd, (H, W))
    want_mm = so.minmax(f.numpy(), (H, W))
    assert equal_bits(mm.cpu().numpy(), want_mm)
    assert want_mm[0, 1] == np.float32(7.5)                     # the corner maximum survives the upsample exactly
    for c0, n, n_pad in chunks(C):
        buf = torch.full((n_pad + 2, 3, H, W), SENTINEL, device=DEV)        # one guard row on either side of the output
        got = ops.scorecam_mask(fd, mm, imgd, c0, n, n_pad, out=buf[1:1 + n_pad])
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all(), "bytes outside the n_pad rows were written"
        want = so.mask(f.numpy(), img.numpy(), c0, n, n_pad)
        assert equal_bits(got.cpu().numpy(), want), (c0, n, n_pad)
        assert not host[1 + n:1 + n_pad].any()                                # padded rows are exactly zero
        for j in range(n):
            if f[c0 + j].max() == f[c0 + j].min():
                assert not host[1 + j].any()                                  # a flat channel masks everything
    if C == 5 and H == 224:                                                   # a fresh output buffer takes the same path
        assert equal_bits(ops.scorecam_mask(fd, mm, imgd, 1, 3, 4).cpu().numpy(), so.mask(f.numpy(), img.numpy(), 1, 3, 4))


@pytest.mark.parametrize("C,fh,fw,H,W,block", [s + (0,) for s in SHAPES if s[1] * s[2] > 1] + [(70, 3, 3, 20, 24, 16)])
def test_combine_matches_the_restatement(C, fh, fw, H, W, block):
    """fp32, ascending channels, product and sum rounded separately on both sides: bit for bit.  C = 70 in channel blocks of 16:
    the LDS streaming crosses four block boundaries and ends on a remainder of 6."""
    f = make_fmap(C, fh, fw, seed=2)
    scores = torch.softmax(torch.randn(C, generator=torch.Generator().manual_seed(3)), dim=0)
    fd = f.to(DEV)
    mm = ops.scorecam_minmax(fd, (H, W))
    got = ops.scorecam_combine(fd, mm, scores.to(DEV), (H, W), channel_block=block).cpu().numpy()
    want = so.combine(f.numpy(), scores.numpy(), (H, W))
    assert np.isfinite(want).all() and want.min() == 0 and want.max() == 1
    assert equal_bits(got, want)
    if block:
        assert equal_bits(ops.scorecam_combine(fd, mm, scores.to(DEV), (H, W)).cpu().numpy(), want)


def test_bad_arguments_return_a_status_without_launching():
    lib = _lib.load()
    f = torch.zeros(2, 7, 7, device=DEV)
    mm = torch.zeros(2, 2, device=DEV)
    img = torch.zeros(3, 8, 8, device=DEV)
    out = torch.full((4, 3, 8, 8), SENTINEL, device=DEV)
    rc = lib.mmskin_scorecam_mask(ptr(f), ptr(mm), ptr(img), 2, 7, 7, 6, 8, 0, 2, 4, ptr(out), stream())     # H < fh
    assert rc != 0 and b"feature map" in lib.mmskin_last_error()
    rc = lib.mmskin_scorecam_minmax(ptr(f), 2, 7, 7, 8, 6, ptr(mm), stream())                                 # W < fw
    assert rc != 0 and b"feature map" in lib.mmskin_last_error()
    rc = lib.mmskin_scorecam_mask(ptr(f), ptr(mm), ptr(img), 2, 7, 7, 8, 8, 0, 2, 1, ptr(out), stream())     # n > n_pad
    assert rc != 0 and b"padded" in lib.mmskin_last_error()
    rc = lib.mmskin_scorecam_mask(ptr(f), ptr(mm), ptr(img), 2, 7, 7, 8, 8, 1, 2, 4, ptr(out), stream())     # c0 + n > C
    assert rc != 0 and b"outside" in lib.mmskin_last_error()
    rc = lib.mmskin_scorecam_combine(ptr(f), ptr(mm), ptr(mm), 0, 7, 7, 8, 8, 0, ptr(out), stream())         # C < 1
    assert rc != 0 and b"extent" in lib.mmskin_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(MMSkinError):
        ops.scorecam_mask(f, mm, img, 0, 3, 2)


# ---------------------------------------------------------------------------------------------------------- end to end
def hip_model(**kw):
    os.environ["MMSKIN_BACKBONE_DTYPE"] = "fp32"
    cpu = det_init_(OracleMultimodalModel(**dict(kw, device="cpu")))
    hip = M.MultimodalModel(**dict(kw, device=DEV))
    hip.load_state_dict(cpu.state_dict(), strict=True)
    return hip.to(DEV).eval()


def last_conv(module):
    last = None
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            last = m
    return last


def check_heat_against_restatement(cam, heat, size):
    """the returned map is the restatement's combine of the features and scores the run itself produced"""
    fmap = cam.features[0].float().cpu().numpy()
    want = so.combine(fmap, cam.scores.cpu().numpy(), size)
    assert heat.dtype == np.float32 and heat.shape == size
    assert equal_bits(heat, want)


@pytest.fixture(scope="module")
def resnet18():
    return hip_model(**dict(SMALL, cnn_model_name="resnet-18", attention_mecanism="crossattention"))


@pytest.mark.parametrize("chunk", [128, 200])
def test_scorecam_resnet18_against_the_reference_golden(resnet18, chunk):
    """chunk 128: four full chunks; chunk 200: a ragged last chunk.  Scores: the fp32 eval logits tolerance test_gpu_model.py
    applies to this encoder (rtol 1e-3, atol 1e-4 on the logits the golden recorded), halved: a soft-max output moves at most
    half as much as its largest logit error."""
    gold = np.load(os.path.join(GOLDEN, "scorecam_resnet18.npz"))
    target = int(gold["target_class"])
    img, meta, _ = det_inputs(1, 64, 20, 6)
    layer = last_conv(resnet18.image_encoder)
    cam = ScoreCAM(resnet18, layer, DEV, chunk=chunk)
    try:
        heat = cam.generate_heatmap(img.to(DEV), meta.to(DEV), target)
        assert list(layer._forward_hooks.values()) == [cam.hook_fn]          # the hook is back on the target layer
        assert tuple(cam.features.shape) == (1, 512, 2, 2)
        fmap_err = float(np.abs(cam.features[0].cpu().numpy() - gold["fmap"]).max())
        assert fmap_err <= 1e-4 * float(np.sqrt((gold["fmap"] ** 2).mean())), fmap_err
        scores = cam.scores.cpu().numpy()
        tol = 0.5 * (1e-4 + 1e-3 * np.abs(gold["logits"])).max(axis=1)
        err = np.abs(scores - gold["scores"])
        print(f"chunk {chunk}: max score error {err.max():.3e}, smallest tolerance {tol.min():.3e}")
        assert scores.shape == (512,) and (err <= tol).all()
        check_heat_against_restatement(cam, heat, (64, 64))
        assert np.isfinite(heat).all() and heat.min() == 0 and heat.max() == 1
        print(f"chunk {chunk}: max |heat - reference heat| {np.abs(heat - gold['heat']).max():.3e}")
    finally:
        cam.remove_hook()
    assert len(layer._forward_hooks) == 0


def test_hook_is_restored_after_an_exception_in_a_masked_forward(resnet18):
    """Metadata of a wrong width reaches the SECOND forward (the first masked one) through a forward pre-hook on the model:
    ops.linear rejects the width on the host, before any kernel is launched; the hook must be back on the layer."""
    img, meta, _ = det_inputs(1, 64, 20, 6)
    layer = last_conv(resnet18.image_encoder)
    cam = ScoreCAM(resnet18, layer, DEV, chunk=128)
    calls = []

    def narrow_metadata(module, args):
        calls.append(tuple(args[1].shape))
        if len(calls) > 1:
            return args[0], args[1][:, :10].contiguous()

    pre = resnet18.register_forward_pre_hook(narrow_metadata)
    try:
        with pytest.raises(MMSkinError, match="width"):
            cam.generate_heatmap(img.to(DEV), meta.to(DEV), 2)
        assert calls == [(1, 20), (128, 20)]
        assert list(layer._forward_hooks.values()) == [cam.hook_fn]
    finally:
        pre.remove()
        cam.remove_hook()
    for make, exc, match in [(lambda: (ScoreCAM(resnet18, layer, DEV), torch.zeros(2, 3, 64, 64, device=DEV)), ValueError, "batch|shape"),
                             (lambda: (ScoreCAM(resnet18, nn.Identity(), DEV), img.to(DEV)), MMSkinError, "did not fire"),
                             (lambda: (ScoreCAM(resnet18, resnet18.image_projector, DEV), img.to(DEV)), MMSkinError, "feature map")]:
        other, image = make()        # two images; a layer the forward never reaches; a layer that delivers a 2-D output
        try:
            with pytest.raises(exc, match=match):
                other.generate_heatmap(image, meta.to(DEV), 2)
        finally:
            other.remove_hook()
    assert len(layer._forward_hooks) == 0


class _PlainModel(nn.Module):
    """ordinary torch modules only; metadata arrives as a mapping of tensors, like a tokenizer's BatchEncoding"""

    def __init__(self):
        super().__init__()
        self.pool = nn.AvgPool2d(8)
        g = torch.Generator().manual_seed(5)
        self.w = nn.Parameter(torch.randn(3, 4, generator=g))
        self.v = nn.Parameter(torch.randn(5, 4, generator=g))

    def forward(self, image, metadata):
        return self.pool(image).mean(dim=(2, 3)) @ self.w + metadata["values"].float() @ self.v


def test_scorecam_on_an_ordinary_module_layer_with_mapping_metadata():
    """C = 3 in chunks of 2 (ragged), 40x24 image, 5x3 map; the scores are those of the reference's per-channel loop run on the
    restatement's masks"""
    model = _PlainModel().to(DEV).eval()
    g = torch.Generator().manual_seed(6)
    img, meta = torch.randn(1, 3, 40, 24, generator=g), {"values": torch.randn(1, 5, generator=g).to(DEV)}
    cam = ScoreCAM(model, model.pool, DEV, chunk=2)
    try:
        heat = cam.generate_heatmap(img.to(DEV), meta, 3)
        fmap = cam.features[0].cpu().numpy()
        assert fmap.shape == (3, 5, 3)
        check_heat_against_restatement(cam, heat, (40, 24))        # before the hook (back on the layer) sees another forward
        masks = torch.from_numpy(so.mask(fmap, img[0].numpy(), 0, 3, 3)).to(DEV)
        with torch.no_grad():
            want = torch.stack([torch.softmax(model(masks[c:c + 1], meta), dim=1)[0, 3] for c in range(3)])
        assert torch.allclose(cam.scores, want, rtol=1e-5, atol=1e-6)
        assert list(model.pool._forward_hooks.values()) == [cam.hook_fn]
    finally:
        cam.remove_hook()


def test_scorecam_densenet169_features_tail():
    """image_encoder.features[-1] of DenseNet-169, the target of every Score-CAM script of the reference: C = 1664, a 2x2 map at
    64x64, chunk 256 (six full chunks and a ragged one of 128)."""
    model = hip_model(**dict(SMALL, cnn_model_name="densenet169", attention_mecanism="crossattention"))
    img, meta, _ = det_inputs(1, 64, 20, 6)
    layer = model.image_encoder.features[-1]
    cam = ScoreCAM(model, layer, DEV, chunk=256)
    try:
        heat = cam.generate_heatmap(img.to(DEV), meta.to(DEV), 1)
        assert tuple(cam.features.shape) == (1, 1664, 2, 2) and tuple(cam.scores.shape) == (1664,)
        assert np.isfinite(heat).all() and heat.min() >= 0 and heat.max() <= 1
        check_heat_against_restatement(cam, heat, (64, 64))
        assert list(layer._forward_hooks.values()) == [cam.hook_fn]
    finally:
        cam.remove_hook()
