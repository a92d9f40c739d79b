"""-m gpu: the Grad-CAM kernels (csrc/gradcam.hip) against their fp64 torch restatement (tests/gradcam_oracle.py, held to the
reference's own classes by tests/test_cpu_gradcam.py), and mmskin.cam.GradCAM / GradCAMPlusPlus end to end: against the
reference-formula loop run row by row through the hooked route on the same HIP model, against the CPU oracle model, and
against the golden recorded from the reference.

Tolerance of the op-level tests.  err(x, want) = max |x - want| / max |want|.  For every case the fp32 restatement is run on
the CPU on the same fp32 inputs; the kernel may be 4 times as far from the fp64 restatement as that (its sums run in another
order than torch's).  Measured err of the fp32 restatement (CPU, torch 2.x), largest over the cases of a shape
(weights mode 0, weights mode 1, raw, cam):
    (33, 7, 7, 37, 53, 2, 5)        1.4e-07  1.7e-07  2.4e-07  5.5e-07
    (512, 2, 2, 64, 64, 3, 3)       8.8e-08  1.1e-07  1.2e-07  3.7e-06
    (1664, 2, 2, 64, 64, 1, 17)     1.0e-07  1.3e-07  1.6e-07  4.7e-06
    (2048, 7, 7, 224, 224, 1, 15)   1.8e-07  1.9e-07  1.5e-07  3.4e-06
    (16, 1, 1, 8, 8, 1, 1)          3.3e-08  8.4e-08  5.1e-08  0 (the flat map: exact zeros)
    (8, 3, 5, 3, 5, 2, 4)           1.1e-07  1.3e-07  7.9e-08  1.6e-07
Conditioning: the Grad-CAM++ denominator 2 g^2 + sum(A g^3) + 1e-8 can cancel when g has mixed sign.  The main cases have
A, jac, dfeat >= 0 (denominator >= 1e-8, nothing excluded).  The mixed-sign case of every shape leaves out the (row, channel)
pairs with a pixel whose fp64 denominator is below 1e-3 * (2 g^2 + |sum(A g^3)| + 1e-8); the data (gradients 1 + 0.45 randn:
1.3 % of the pixels negative) and seed were chosen on the CPU so that this is under 1 % of the pairs (at most 0.23 %, on the
2048-channel shape), and the test asserts it.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import gradcam_oracle as go
from gpu_util import DEV, rel_err
from helpers import GOLDEN, SMALL
from mmskin import _lib, backbone, ops
from mmskin._lib import MMSkinError, ptr, stream
from mmskin.cam import GradCAM, GradCAMPlusPlus
from test_gpu_model import build_pair

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
# (C, fh, fw, H, W, N, R): odd sizes and a 64-lane sub-wave; a 2x2 map (4-lane sub-waves) with one row per image; DenseNet's
# 1664 channels with 17 rows of one image; production scale; one pixel (the flat map); H = fh (no upsample) with a 16-lane sub-wave
SHAPES = [(33, 7, 7, 37, 53, 2, 5), (512, 2, 2, 64, 64, 3, 3), (1664, 2, 2, 64, 64, 1, 17), (2048, 7, 7, 224, 224, 1, 15),
          (16, 1, 1, 8, 8, 1, 1), (8, 3, 5, 3, 5, 2, 4)]
MIXED_SEED = 11
SENTINEL = -77.0


def err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


def rows_to_images(N, R):
    """rows share images (R > N) and come in non-monotone image order (N > 1)"""
    return (((R - 1 - torch.arange(R)) * 3 + 1) % N).to(torch.int32)


def make_case(shape, with_dfeat, mixed, seed=0):
    C, fh, fw, H, W, N, R = shape
    g = torch.Generator().manual_seed(MIXED_SEED if mixed else seed)
    acts = torch.rand(N, C, fh, fw, generator=g)
    jshape = (N if with_dfeat else R, C, fh, fw)
    if mixed:
        jac = 1 + 0.45 * torch.randn(jshape, generator=g)
        dfeat = 1 + 0.35 * torch.randn(R, C, generator=g) if with_dfeat else None
        w = torch.randn(R, C, generator=g)
        acts_map = acts - 0.3
    else:
        jac = torch.rand(jshape, generator=g)
        dfeat = torch.rand(R, C, generator=g) if with_dfeat else None
        w = torch.rand(R, C, generator=g)
        acts_map = acts
    return dict(acts=acts, jac=jac, dfeat=dfeat, row_image=rows_to_images(N, R), w=w, acts_map=acts_map, size=(H, W))


def kept_pairs(case):
    """[R, C] bool: pairs whose Grad-CAM++ denominator does not cancel (see the module docstring)"""
    den, bound = go.plusplus_denominator(case["acts"], case["jac"], case["dfeat"], case["row_image"], F64)
    return ~(den < 1e-3 * bound).any(dim=(2, 3))


def dev(t):
    return None if t is None else t.to(DEV)


def gpu_weights(case, mode, row_image=None):
    ri = case["row_image"] if row_image is None else row_image
    return ops.gradcam_weights(dev(case["acts"]), dev(case["jac"]), dev(case["dfeat"]), dev(ri), mode).cpu()


@pytest.mark.parametrize("mixed", [False, True], ids=["positive", "mixed"])
@pytest.mark.parametrize("with_dfeat", [True, False], ids=["jac_x_dfeat", "full_gradient"])
@pytest.mark.parametrize("mode", [0, 1], ids=["gradcam", "plusplus"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weights_match_the_fp64_restatement(shape, mode, with_dfeat, mixed):
    case = make_case(shape, with_dfeat, mixed)
    args = (case["acts"], case["jac"], case["dfeat"], case["row_image"], mode)
    want, w32 = go.weights(*args, F64), go.weights(*args, F32)
    keep = torch.ones_like(want, dtype=torch.bool)
    if mixed and mode == 1:
        keep = kept_pairs(case)
        excluded = 1.0 - float(keep.double().mean())
        print(f"{shape} mixed: {excluded:.4%} of the pairs excluded")
        assert excluded <= 0.01
    elif mode == 1:
        assert bool(kept_pairs(case).all())
    got = gpu_weights(case, mode)
    assert got.shape == want.shape and bool(torch.isfinite(got[keep]).all())
    noise, e = err(w32[keep], want[keep]), err(got[keep], want[keep])
    print(f"{shape} mode {mode} dfeat {with_dfeat} mixed {mixed}: fp32 restatement {noise:.3e}, kernel {e:.3e}")
    assert e <= 4 * noise
    assert torch.equal(gpu_weights(case, mode), got)                                   # two runs, bit for bit


@pytest.mark.parametrize("mixed", [False, True], ids=["positive", "mixed"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_map_matches_the_fp64_restatement(shape, mixed):
    case = make_case(shape, True, mixed)
    acts, w, ri, size = case["acts_map"].contiguous(), case["w"], case["row_image"], case["size"]
    want_raw, raw32 = go.raw_map(acts, w, ri, F64), go.raw_map(acts, w, ri, F32)
    want_cam, cam32 = go.cam(want_raw, size, F64), go.cam(raw32, size, F32)
    raw, cam = ops.gradcam_map(dev(acts), dev(w), dev(ri), size)
    raw2, cam2 = ops.gradcam_map(dev(acts), dev(w), dev(ri), size)
    assert torch.equal(raw, raw2) and torch.equal(cam, cam2)                           # two runs, bit for bit
    assert raw.shape == want_raw.shape and cam.shape == want_cam.shape
    for name, got, w32, want in (("raw", raw, raw32, want_raw), ("cam", cam, cam32, want_cam)):
        noise, e = err(w32, want), err(got, want)
        print(f"{shape} mixed {mixed} {name}: fp32 restatement {noise:.3e}, kernel {e:.3e}")
        assert bool(torch.isfinite(got).all()) and e <= 4 * noise, name
    assert float(cam.min()) >= 0 and float(cam.max()) <= 1
    if shape[1] * shape[2] == 1:
        assert not bool(cam.any())                                                     # the flat map: zeros, not NaN


def test_normalisation_before_upsample_and_per_row_on_the_device():
    """the two cases of test_cpu_gradcam.py through the kernel: one channel of weight 1 makes raw the activations themselves"""
    acts = torch.tensor([[[[-4.0, 1.0], [0.5, 2.0]]], [[[250.0, 1000.0], [500.0, 2000.0]]]])
    ri = torch.tensor([0, 1, 0], dtype=torch.int32)
    raw, cam = ops.gradcam_map(dev(acts), torch.ones(3, 1, device=DEV), dev(ri), (8, 8))
    assert torch.equal(raw.cpu(), acts[ri.long(), 0])
    want = go.cam(acts[ri.long(), 0], (8, 8), F64)
    assert float((cam.cpu().double() - want).abs().max()) < 1e-6
    assert float((cam.cpu().double() - go.cam_upsample_first(acts[ri.long(), 0], (8, 8), F64))[0].abs().max()) > 0.1
    assert float(cam[1].max()) == pytest.approx(1.0, abs=1e-6) and torch.equal(cam[0], cam[2])


def test_an_out_of_range_row_image_entry_is_clamped():
    shape = (33, 7, 7, 37, 53, 2, 5)
    case = make_case(shape, True, False)
    wild = torch.tensor([7, -3, 1, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32)
    tame = wild.clamp(0, 1)
    for mode in (0, 1):
        assert torch.equal(gpu_weights(case, mode, wild), gpu_weights(case, mode, tame))
        want = go.weights(case["acts"], case["jac"], case["dfeat"], wild, mode, F64)             # the restatement clamps too
        noise = err(go.weights(case["acts"], case["jac"], case["dfeat"], wild, mode, F32), want)
        assert err(gpu_weights(case, mode, wild), want) <= 4 * noise
    a, b = ops.gradcam_map(dev(case["acts"]), dev(case["w"]), dev(wild), case["size"])
    c, d = ops.gradcam_map(dev(case["acts"]), dev(case["w"]), dev(tame), case["size"])
    assert torch.equal(a, c) and torch.equal(b, d)
    want = go.raw_map(case["acts"], case["w"], wild, F64)
    assert err(a, want) <= 4 * err(go.raw_map(case["acts"], case["w"], wild, F32), want)


def test_bad_arguments_return_a_status_without_launching():
    lib = _lib.load()
    N, R, C, fh, fw, H, W = 2, 3, 4, 7, 7, 8, 8
    acts, jac = torch.zeros(N, C, fh, fw, device=DEV), torch.zeros(N, C, fh, fw, device=DEV)
    dfeat, ri = torch.zeros(R, C, device=DEV), torch.zeros(R, dtype=torch.int32, device=DEV)
    w = torch.full((R, C), SENTINEL, device=DEV)
    raw, cam = torch.full((R, fh, fw), SENTINEL, device=DEV), torch.full((R, H, W), SENTINEL, device=DEV)

    def weights(N=N, R=R, C=C, fh=fh, fw=fw, mode=0):
        return lib.mmskin_gradcam_weights(ptr(acts), ptr(jac), ptr(dfeat), ptr(ri), N, R, C, fh, fw, mode, ptr(w), stream())

    def cmap(N=N, R=R, C=C, fh=fh, fw=fw, H=H, W=W):
        return lib.mmskin_gradcam_map(ptr(acts), ptr(dfeat), ptr(ri), N, R, C, fh, fw, H, W, ptr(raw), ptr(cam), stream())

    for kw in (dict(N=0), dict(C=0), dict(fh=0), dict(fw=-1)):
        assert weights(**kw) != 0 and b"extent" in lib.mmskin_last_error()
        assert cmap(**kw) != 0 and b"extent" in lib.mmskin_last_error()
    assert cmap(H=0) != 0 and b"extent" in lib.mmskin_last_error()
    assert cmap(W=0) != 0 and b"extent" in lib.mmskin_last_error()
    assert weights(R=0) != 0 and b"rows" in lib.mmskin_last_error()
    assert cmap(R=0) != 0 and b"rows" in lib.mmskin_last_error()
    assert cmap(H=6) != 0 and b"feature map" in lib.mmskin_last_error()                # H < fh
    assert cmap(W=6) != 0 and b"feature map" in lib.mmskin_last_error()                # W < fw
    for mode in (-1, 2):
        assert weights(mode=mode) != 0 and b"mode" in lib.mmskin_last_error()
    unsupported = weights(fh=65, fw=64)                                                # 4160 samples > the 4096 of the LDS tile
    assert unsupported != 0 and b"LDS" in lib.mmskin_last_error()
    assert unsupported != weights(mode=2)                                              # MMSKIN_ERR_UNSUPPORTED, not MMSKIN_ERR_ARG
    assert cmap(fh=65, fw=64, H=128, W=128) == unsupported
    torch.cuda.synchronize()
    assert bool((w == SENTINEL).all()) and bool((raw == SENTINEL).all()) and bool((cam == SENTINEL).all())
    with pytest.raises(ValueError, match="mode"):
        ops.gradcam_weights(acts, jac, dfeat, ri, 2)
    with pytest.raises(ValueError, match="jac"):
        ops.gradcam_weights(acts, jac, None, ri, 0)                                    # without dfeat jac must have R rows
    with pytest.raises(ValueError, match="row_image"):
        ops.gradcam_map(acts, dfeat, ri.long(), (H, W))
    with pytest.raises(MMSkinError):
        ops.gradcam_map(acts.cpu(), dfeat, ri, (H, W))                                 # no CPU fallback


# ---------------------------------------------------------------------------------------------------------- end to end
def last_conv(module):
    return [m for m in module.modules() if isinstance(m, nn.Conv2d)][-1]


def target_of(model, arch):
    return model.image_encoder.features[-1] if arch == "densenet169" else last_conv(model.image_encoder)


def reference_loop(model, layer, img, meta, variants, mode, targets=None):
    """The reference's generate (gradcam_atualizado.py:230-306), one row at a time through the hooked route, every row for its
    predicted class (or targets[r]): what a user of the parent commit runs.  Returns per-row tensors on the CPU."""
    store, out = {}, dict(acts=[], grads=[], pred=[], raw=[], cam=[])
    handle = layer.register_forward_hook(lambda mod, i, o: store.__setitem__("a", o))
    try:
        for r in range(meta.shape[0]):
            image = img[r // variants:r // variants + 1].clone().requires_grad_(True)
            logits = model(image, meta[r:r + 1])
            pred = int(logits.argmax(dim=1)) if targets is None else int(targets[r])
            acts = store["a"]
            grads = torch.autograd.grad(logits[:, pred].sum(), acts)[0]
            if mode == 0:
                weights = grads.mean(dim=(2, 3), keepdim=True)
            else:
                g2, g3 = grads ** 2, grads ** 3
                alpha = g2 / (2 * g2 + (acts * g3).sum(dim=(2, 3), keepdim=True) + 1e-8)
                weights = (alpha * torch.relu(grads)).sum(dim=(2, 3), keepdim=True)
            raw = (weights * acts).sum(dim=1, keepdim=True)
            cam = torch.relu(raw)
            cam = (cam - cam.min()) / (cam.max() - cam.min() + 1e-8)
            cam = F.interpolate(cam, size=image.shape[-2:], mode="bilinear", align_corners=False)
            for k, v in (("acts", acts[0]), ("grads", grads[0]), ("raw", raw[0, 0]), ("cam", cam[0, 0])):
                out[k].append(v.detach().float().cpu())
            out["pred"].append(pred)
    finally:
        handle.remove()
    return {k: torch.tensor(v) if k == "pred" else torch.stack(v) for k, v in out.items()}


PAIRS = {"resnet-18": 3, "densenet169": 2, "custom-cnn": 2}


_BUILT = {}


def pair(arch):
    """(arch, cpu model, hip model, images, metadata rows): built once per encoder; no test modifies it"""
    if arch not in _BUILT:
        cpu, hip = build_pair("fp32", **dict(SMALL, cnn_model_name=arch, attention_mecanism="concatenation"))
        _BUILT[arch] = (arch, cpu.eval(), hip.eval()) + go.det_rows(PAIRS[arch], 64)
    return _BUILT[arch]


@pytest.fixture(scope="module", params=list(PAIRS))
def setup(request):
    return pair(request.param)


@pytest.mark.parametrize("cls", [GradCAMPlusPlus, GradCAM], ids=["plusplus", "gradcam"])
def test_generate_batch_against_the_loop_the_oracle_model_and_the_golden(setup, cls, monkeypatch):
    arch, cpu, hip, img, meta = setup
    V, mode = go.VARIANTS, cls.mode
    N, R = img.shape[0], meta.shape[0]
    layer = target_of(hip, arch)
    forwards = []
    apply = backbone._BackboneFn.apply
    monkeypatch.setattr(backbone._BackboneFn, "apply", staticmethod(lambda *a: (forwards.append(a[0].shape[0]), apply(*a))[1]))
    cam = cls(hip, layer)
    try:
        maps = cam.generate_batch(img.to(DEV), meta.to(DEV), None, variants_per_image=V)
        # the point of the feature: ONE encoder forward, at batch N (custom-cnn is no plan encoder: its generic route runs at batch R)
        assert forwards == ([] if arch == "custom-cnn" else [N])
        assert list(layer._forward_hooks.values()) == [cam._forward_hook]
        assert maps.is_cuda and maps.dtype == F32 and tuple(maps.shape) == (R, 64, 64)
        assert float(maps.min()) >= 0 and float(maps.max()) <= 1
        C, fh, fw = cam.activations.shape[1:]
        assert tuple(cam.weights.shape) == (R, C) and tuple(cam.raw.shape) == (R, fh, fw)
        assert tuple(cam.pred.shape) == (R,) and tuple(cam.probs.shape) == (R, 6)
        assert torch.equal(cam.probs.argmax(dim=1), cam.pred)
        if arch != "custom-cnn":
            first = cam.generate(img[:1].to(DEV), meta[:1].to(DEV), int(cam.pred[0]))       # R = 1: row 0 of the batch
            assert isinstance(first, np.ndarray) and first.dtype == np.float32 and first.shape == (64, 64)
    finally:
        cam.remove_hook()
    assert len(layer._forward_hooks) == 0
    maps = maps.cpu()

    # (a) the loop of the parent commit on the same HIP model; tolerance: 4 x the float noise of the loop's own formula, measured
    # as the fp32 restatement against the fp64 restatement on the loop's activations and gradients
    loop = reference_loop(hip, layer, img.to(DEV), meta.to(DEV), V, mode)
    every = torch.arange(R, dtype=torch.int32)
    w64, raw64, cam64 = go.explain(loop["acts"], loop["grads"], None, every, mode, (64, 64), F64)
    w32, raw32, cam32 = go.explain(loop["acts"], loop["grads"], None, every, mode, (64, 64), F32)
    got = cls(hip, layer)
    try:
        got_maps = got.generate_batch(img.to(DEV), meta.to(DEV), None, variants_per_image=V).cpu()
        assert torch.equal(got_maps, maps)                                                  # and the call repeats bit for bit
        assert torch.equal(got.pred.cpu(), loop["pred"])
        for name, mine, theirs, f32, f64 in (("raw", got.raw, loop["raw"], raw32, raw64), ("cam", got_maps, loop["cam"], cam32, cam64)):
            noise = err(f32, f64)
            print(f"{arch} mode {mode} {name}: fp32 restatement {noise:.3e}, the loop itself {err(theirs, f64):.3e}, generate_batch "
                  f"{err(mine, f64):.3e} (all against the loop's formula in fp64)")
            assert err(mine, f64) <= 4 * noise, name
        if arch != "custom-cnn":
            assert float(np.abs(first - got_maps[0].numpy()).max()) <= 4 * err(cam32, cam64)

        # (b) the CPU oracle model, the bound test_gpu_model.py puts on this quantity
        ref = reference_loop(cpu, target_of(cpu, arch), img, meta, V, mode, targets=loop["pred"])
        print(f"{arch} mode {mode}: rel_err(raw) against the oracle model {rel_err(got.raw, ref['raw']):.3e}")
        assert rel_err(got.raw, ref["raw"]) < 1e-3

        # (c) the reference's own maps
        if arch == "resnet-18":
            gold = np.load(os.path.join(GOLDEN, "gradcam_resnet18.npz"))
            assert np.array_equal(got.pred.cpu().numpy(), gold["targets"])
            want = torch.from_numpy(gold["plusplus_maps" if mode == 1 else "gradcam_maps"])
            print(f"{arch} mode {mode}: rel_err(maps) against the golden {rel_err(got_maps, want):.3e}")
            assert rel_err(got_maps, want) < 1e-3
    finally:
        got.remove_hook()


def test_explicit_targets_batch_checks_and_modes():
    arch, cpu, hip, img, meta = pair("resnet-18")
    layer = target_of(hip, arch)
    cam = GradCAMPlusPlus(hip, layer)
    try:
        R = meta.shape[0]
        a = cam.generate_batch(img.to(DEV), meta.to(DEV), 2, variants_per_image=go.VARIANTS)
        b = cam.generate_batch(img.to(DEV), meta.to(DEV), torch.full((R,), 2), variants_per_image=go.VARIANTS)
        assert torch.equal(a, b)
        with pytest.raises(ValueError, match=r"\(1, 3, H, W\)"):
            cam.generate(img[:2].to(DEV), meta[:1].to(DEV), 2)                               # a batch-2 image
        with pytest.raises(ValueError, match="rows"):
            cam.generate_batch(img.to(DEV), meta[:4].to(DEV), 2, variants_per_image=go.VARIANTS)
        with pytest.raises(ValueError, match="outside"):
            cam.generate_batch(img.to(DEV), meta.to(DEV), 6, variants_per_image=go.VARIANTS)
        hip.train()
        try:
            with pytest.raises(MMSkinError, match="eval mode"):
                cam.generate_batch(img.to(DEV), meta.to(DEV), 2, variants_per_image=go.VARIANTS)
        finally:
            hip.eval()
        assert list(layer._forward_hooks.values()) == [cam._forward_hook]
    finally:
        cam.remove_hook()
    assert len(layer._forward_hooks) == 0


def test_hook_stays_and_state_is_cleared_after_an_exception_inside_fuse():
    """Metadata of the right row count but a wrong width passes generate_batch's own checks and reaches model.fuse, where
    ops.linear rejects the width on the host before any kernel is launched.  As documented: the hook stays on the layer until
    remove_hook(), nothing half-built stays on the object, and the next call works."""
    arch, cpu, hip, img, meta = pair("resnet-18")
    layer = target_of(hip, arch)
    cam = GradCAM(hip, layer)
    fused = []
    fuse = hip.fuse
    hip.fuse = lambda feats, metadata: (fused.append(tuple(feats.shape)), fuse(feats, metadata))[1]
    try:
        with pytest.raises(MMSkinError, match="width"):
            cam.generate_batch(img.to(DEV), meta[:, :10].contiguous().to(DEV), None, variants_per_image=go.VARIANTS)
        assert fused == [(meta.shape[0], 512)]
        assert list(layer._forward_hooks.values()) == [cam._forward_hook]
        assert cam.activations is None and cam.weights is None and cam.raw is None and cam.pred is None and cam.probs is None
        maps = cam.generate_batch(img.to(DEV), meta.to(DEV), None, variants_per_image=go.VARIANTS)
        assert bool(torch.isfinite(maps).all()) and cam.weights is not None
        cam.clear()
        assert cam.activations is None and cam.weights is None
    finally:
        del hip.fuse
        cam.remove_hook()
    assert len(layer._forward_hooks) == 0
    other = GradCAM(hip, nn.Identity())
    try:
        with pytest.raises(MMSkinError, match="did not fire"):
            other.generate_batch(img.to(DEV), meta.to(DEV), None, variants_per_image=go.VARIANTS)
    finally:
        other.remove_hook()


@pytest.mark.parametrize("arch,n_images", [("resnet-18", 3), ("densenet169", 2)])
def test_bf16_model_runs_and_gives_finite_maps_in_range(arch, n_images):
    """no numeric bound is claimed for the bf16 encoder: the maps exist, are finite and lie in [0, 1]"""
    _, hip = build_pair("bf16", **dict(SMALL, cnn_model_name=arch, attention_mecanism="concatenation"))
    hip.eval()
    img, meta = go.det_rows(n_images, 64)
    for cls in (GradCAM, GradCAMPlusPlus):
        cam = cls(hip, target_of(hip, arch))
        try:
            maps = cam.generate_batch(img.to(DEV), meta.to(DEV), None, variants_per_image=go.VARIANTS)
            assert tuple(maps.shape) == (n_images * go.VARIANTS, 64, 64)
            assert bool(torch.isfinite(maps).all()) and float(maps.min()) >= 0 and float(maps.max()) <= 1
        finally:
            cam.remove_hook()
