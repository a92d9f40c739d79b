"""RISE saliency (Petsiuk et al., 2018, "RISE: Randomized Input Sampling for Explanation of Black-box Models"): the image is
masked with many random smooth masks, the model runs on every masked image, and the masks are averaged with the probability of
the target class as their weight.  It needs nothing of the model but `model(images, metadata)`, so it explains the encoders
the CAM classes of mmskin.cam cannot hook (the transformer encoders, the NAS DynamicCNN), and its maps go straight into
mmskin.faithfulness.CamFaithfulness.evaluate.

A mask is a pure function of (seed, mask index, pixel), stated in include/mmskin.h: a (grid + 1)^2 binary cell grid, each cell
on with probability p1, upsampled bilinearly by the cell size and cropped at a random shift.  The masks are shared by all
images of a call, as in RISE.  `RISE.generate_batch` writes one chunk of masked images with one kernel (mmskin.ops.rise_apply),
runs each chunk as one forward, keeps the logits on the device and reduces them with one call (rise_accumulate); both kernels
compute the mask in registers, no mask tensor exists, and nothing is read back between chunks.  The sums are fp64 in a fixed
order: a call is bitwise repeatable.

Unlike the published code, which upsamples a grid x grid array of cells with skimage.resize, the upsample here is the one
stated above (half-pixel centres, edge clamp), exact in integers.

Eval mode, forward only: nothing here is differentiable.
"""
from dataclasses import dataclass, fields

import numpy as np
import torch

from . import ops
from ._lib import MMSkinError
from ._image_explainer import (Baseline, check_images, check_rows, check_target_range, chunk_or_default, chunked_logits,
                               model_device, require_eval, target_tensor)

NORMALIZE = ("expected", "coverage")


@dataclass
class RiseResult:
    """Device tensors; `.cpu()` copies all of them to the host at once."""
    saliency: torch.Tensor                # [N, H, W] fp32: saliency_sum / (n_masks * p1) ("expected") or / coverage ("coverage")
    saliency_sum: torch.Tensor            # [N, H, W] fp64: sum over the masks of probability * mask
    coverage: torch.Tensor                # [H, W] fp64: sum over the masks of the mask
    clean_prob: torch.Tensor              # [N] fp64: the probability of the target class on the unmasked image
    target: torch.Tensor                  # [N] int32: the class every image was explained on

    def cpu(self):
        return RiseResult(**{f.name: getattr(self, f.name).cpu() for f in fields(self)})


class RISE:
    def __init__(self, model, device, n_masks=4000, grid=8, p1=0.5, baseline="zero", seed=0, chunk=None, normalize="expected",
                 blur_ksize=11, blur_sigma=5.0):
        """
        model: the loaded multimodal model (eval mode); any module called as model(images, metadata) that returns logits.
        device: the model's device.
        n_masks, grid, p1, seed: the masks (4000 / 8 / 0.5 are the paper's for ResNet-50); grid in 2 .. 16, p1 inside (0, 1).
        baseline: what a masked pixel fades to, CamFaithfulness's: "zero" = the dataset mean in normalised space (the paper's),
            "blur" = Gaussian blur of the image itself (blur_ksize, blur_sigma), "mean" = the image's own per-channel mean.
        chunk: rows per forward (the batch size of those forwards); the ragged last chunk is padded to it with zero rows.
        normalize: "expected" divides the weighted sum by n_masks * p1 (the paper's), "coverage" by the sum of the masks at the
            pixel (0 where no mask reaches it).
        """
        self.model = model
        self.device = device
        self.n_masks = int(n_masks)
        if not 1 <= self.n_masks <= ops.RISE_MAX_MASKS:
            raise ValueError(f"RISE: n_masks must be in 1 .. {ops.RISE_MAX_MASKS}, got {n_masks}")
        self.seed, self.grid, self.p1 = ops._rise_args(seed, grid, p1, "RISE")
        if normalize not in NORMALIZE:
            raise ValueError(f"RISE: normalize must be one of {NORMALIZE}, got {normalize!r}")
        self.normalize = normalize
        self._baseline = Baseline("RISE", baseline, blur_ksize, blur_sigma)
        self.baseline, self.taps = baseline, self._baseline.taps
        self.chunk = chunk_or_default(chunk, "RISE")

    def baseline_images(self, images):
        """images [N, 3, H, W] fp32 on the device -> the baseline of every image, same shape"""
        return self._baseline.images(images)

    def generate_batch(self, images, metadata, target_class=None):
        """images (N, 3, H, W) as the model takes them; metadata (N, V) or a mapping of such tensors; target_class an int, an
        int tensor (N,), or None = the argmax of the clean forward, taken on the device -> RiseResult."""
        who = "RISE.generate_batch"
        check_images(images, who)
        N, _, H, W = images.shape
        check_rows(metadata, N, who)
        dev = self.device
        target = target_tensor(target_class, N, dev, who)
        require_eval(self.model, "RISE")
        if H * W > ops.faith_max_pixels():
            raise MMSkinError(f"{who}: {H}x{W} images are above the kernels' cap of {ops.faith_max_pixels()} pixels")

        images = images.detach().to(dev).float().contiguous()
        base = self.baseline_images(images)
        n_masks, chunk = self.n_masks, self.chunk
        R = N * n_masks
        row_image = torch.arange(-(-R // chunk) * chunk, device=dev).div_(n_masks, rounding_mode="floor").clamp_(max=N - 1)
        with torch.no_grad():
            clean = self.model(images, metadata)
        if clean.dim() != 2 or clean.shape[0] != N:
            raise MMSkinError(f"{who}: the model must return logits of shape ({N}, K), got {tuple(clean.shape)}")
        clean = clean.float().contiguous()
        K = clean.shape[1]

        def write_chunk(r0, n, out):
            return ops.rise_apply(images, base, self.seed, self.grid, self.p1, n_masks, r0, n, chunk, out=out)

        logits = chunked_logits(self.model, metadata, row_image, R, chunk, write_chunk, who, K)
        check_target_range(target, K, who)
        total, coverage, clean_prob, used = ops.rise_accumulate(logits, clean, (H, W), self.seed, self.grid, self.p1, n_masks, target)
        if self.normalize == "expected":
            saliency = total / (n_masks * self.p1)
        else:
            saliency = torch.where(coverage > 0, total / coverage, torch.zeros_like(total))
        return RiseResult(saliency=saliency.float(), saliency_sum=total, coverage=coverage, clean_prob=clean_prob, target=used)

    def generate(self, image, metadata, target_class=None):
        """image (1, 3, H, W), metadata of one row -> np.ndarray [H, W] float32, min-max normalised to [0, 1] (+1e-8 in the
        denominator: a flat map gives zeros): the convention of the CAM classes."""
        check_images(image, "RISE.generate", one=True)
        sal = self.generate_batch(image, metadata, target_class).saliency[0]
        lo, hi = sal.min(), sal.max()
        return ((sal - lo) / (hi - lo + 1e-8)).cpu().numpy()


def rise_maps(model, images, metadata, target=None, **kw):
    """The RISE maps [N, H, W] (device, fp32) of RISE(model, device, **kw) on `target` (an int, an int tensor [N], or None = the
    model's own prediction; device=... for a model without parameters): what CamFaithfulness.evaluate takes as `saliency`, unchanged."""
    device = kw.pop("device", None) or model_device(model)
    return RISE(model, device, **kw).generate_batch(images, metadata, target).saliency
