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
from .cam import ScoreCAM, _check_rows
from .faithfulness import BASELINES, _take_rows

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
        if baseline not in BASELINES:
            raise ValueError(f"RISE: baseline must be one of {BASELINES}, got {baseline!r}")
        self.baseline = baseline
        if normalize not in NORMALIZE:
            raise ValueError(f"RISE: normalize must be one of {NORMALIZE}, got {normalize!r}")
        self.normalize = normalize
        self.taps = ops.gaussian_taps(blur_ksize, blur_sigma) if baseline == "blur" else None
        self.chunk = int(chunk) if chunk is not None else ScoreCAM.default_chunk
        if self.chunk < 1:
            raise ValueError(f"RISE: chunk must be >= 1, got {chunk}")

    def baseline_images(self, images):
        """images [N, 3, H, W] fp32 on the device -> the baseline of every image, same shape"""
        if self.baseline == "blur":
            return ops.faith_blur(images, self.taps)
        if self.baseline == "mean":
            return ops.faith_mean(images)
        return torch.zeros_like(images)

    def generate_batch(self, images, metadata, target_class=None):
        """images (N, 3, H, W) as the model takes them; metadata (N, V) or a mapping of such tensors; target_class an int, an
        int tensor (N,), or None = the argmax of the clean forward, taken on the device -> RiseResult."""
        who = "RISE.generate_batch"
        if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
            raise ValueError(f"{who}: images must have shape (N, 3, H, W), got "
                             f"{tuple(images.shape) if torch.is_tensor(images) else type(images).__name__}")
        N, _, H, W = images.shape
        _check_rows(metadata, N, who)
        if torch.is_tensor(target_class) and (target_class.dim() != 1 or target_class.shape[0] != N or target_class.is_floating_point()):
            raise ValueError(f"{who}: target_class must be an int, None or an int tensor [{N}], got "
                             f"{target_class.dtype} {tuple(target_class.shape)}")
        if self.model.training:
            raise MMSkinError("RISE runs in eval mode: call model.eval() first")
        if H * W > ops.faith_max_pixels():
            raise MMSkinError(f"{who}: {H}x{W} images are above the kernels' cap of {ops.faith_max_pixels()} pixels")
        dev = self.device
        target = None
        if target_class is not None:
            if torch.is_tensor(target_class):
                target = target_class.to(dev).to(torch.int32).contiguous()
            else:
                target = torch.full((N,), int(target_class), device=dev, dtype=torch.int32)

        images = images.detach().to(dev).float().contiguous()
        base = self.baseline_images(images)
        n_masks, chunk = self.n_masks, self.chunk
        R = N * n_masks
        n_chunks = -(-R // chunk)
        row_image = torch.arange(n_chunks * chunk, device=dev).div_(n_masks, rounding_mode="floor").clamp_(max=N - 1)
        masked = torch.empty((chunk, 3, H, W), device=dev, dtype=torch.float32)
        with torch.no_grad():
            clean = self.model(images, metadata)
            if clean.dim() != 2 or clean.shape[0] != N:
                raise MMSkinError(f"{who}: the model must return logits of shape ({N}, K), got {tuple(clean.shape)}")
            clean = clean.float().contiguous()
            K = clean.shape[1]
            logits = torch.empty((n_chunks * chunk, K), device=dev, dtype=torch.float32)
            for c in range(n_chunks):
                r0 = c * chunk
                ops.rise_apply(images, base, self.seed, self.grid, self.p1, n_masks, r0, min(chunk, R - r0), chunk, out=masked)
                out = self.model(masked, _take_rows(metadata, row_image[r0:r0 + chunk]))
                if out.dim() != 2 or tuple(out.shape) != (chunk, K):
                    raise MMSkinError(f"{who}: the model must return logits of shape ({chunk}, {K}), got {tuple(out.shape)}")
                logits[r0:r0 + chunk] = out                              # the padded rows' logits are never read
        if target is not None and bool(((target < 0) | (target >= K)).any()):       # checked where the tensor lives
            raise ValueError(f"{who}: target_class has entries outside 0 .. {K - 1}")
        total, coverage, clean_prob, used = ops.rise_accumulate(logits, clean, (H, W), self.seed, self.grid, self.p1, n_masks, target)
        if self.normalize == "expected":
            saliency = total / (n_masks * self.p1)
        else:
            saliency = torch.where(coverage > 0, total / coverage, torch.zeros_like(total))
        return RiseResult(saliency=saliency.float(), saliency_sum=total, coverage=coverage, clean_prob=clean_prob, target=used)

    def generate(self, image, metadata, target_class=None):
        """image (1, 3, H, W), metadata of one row -> np.ndarray [H, W] float32, min-max normalised to [0, 1] (+1e-8 in the
        denominator: a flat map gives zeros): the convention of the CAM classes."""
        if not torch.is_tensor(image) or image.dim() != 4 or image.shape[0] != 1 or image.shape[1] != 3:
            raise ValueError(f"RISE.generate: image must have shape (1, 3, H, W), got "
                             f"{tuple(image.shape) if torch.is_tensor(image) else type(image).__name__}")
        sal = self.generate_batch(image, metadata, target_class).saliency[0]
        lo, hi = sal.min(), sal.max()
        return ((sal - lo) / (hi - lo + 1e-8)).cpu().numpy()


def rise_maps(model, images, metadata, target=None, **kw):
    """The RISE maps [N, H, W] (device, fp32) of RISE(model, device, **kw) on `target` (an int, an int tensor [N], or None = the
    model's own prediction; device=... for a model without parameters): what CamFaithfulness.evaluate takes as `saliency`, unchanged."""
    device = kw.pop("device", None) or getattr(model, "device", None) or next(model.parameters()).device
    return RISE(model, device, **kw).generate_batch(images, metadata, target).saliency
