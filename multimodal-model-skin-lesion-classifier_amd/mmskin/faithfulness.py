"""Faithfulness scores of class-activation maps: which of Score-CAM, Grad-CAM and Grad-CAM++ (mmskin.cam) explains the model
better.  The reference compares the three by eye (interpretability/cam_methods_comparison.py draws them side by side); this
is the standard quantitative comparison, batched on the GPU:

  deletion / insertion curves (Petsiuk et al., RISE): the probability of the target class while the most salient pixels are
      replaced by a baseline (deletion: lower area is better) or restored onto it (insertion: higher area is better)
  average drop / increase in confidence (Chattopadhay et al., Grad-CAM++): the probability on the explanation image
      baseline + saliency * (image - baseline) against the clean probability

A curve of S steps is 2 (S + 1) + 1 forwards per image, each on a differently perturbed image.  `CamFaithfulness.evaluate`
ranks the pixels of all maps with one kernel (mmskin.ops.faith_rank), builds the perturbed images chunk by chunk with one
kernel (faith_perturb), runs each chunk as one forward of the model on its eval plan, keeps the logits on the device and
reduces them with one kernel (faith_curves).  Nothing is read back between chunks, or at all: the result holds device tensors.

Definitions (include/mmskin.h states them with the kernels): rank = descending saliency, ties by ascending row-major pixel
index; step k = 0 .. S touches the (k * H * W) // S top-ranked pixels; the curve value is the soft-max probability of the
target class; areas by the trapezoid rule over x = k / S; average_drop = max(0, p - p_expl) / p; increase = 1[p_expl > p].

Eval mode, forward only: nothing here is differentiable.
"""
from dataclasses import dataclass, fields

import numpy as np
import torch

from . import ops
from ._lib import MMSkinError
from ._image_explainer import (BASELINES, Baseline, check_images, check_rows, check_target_range, chunk_or_default,  # noqa: F401
                               chunked_logits, model_device, require_eval, take_rows, target_tensor)
from .cam import GradCAM, GradCAMPlusPlus, ScoreCAM


@dataclass
class FaithfulnessResult:
    """Device tensors (fp64 unless noted); `.cpu()` copies all of them to the host at once."""
    deletion: torch.Tensor                # [N, S + 1] probability of the target class after deleting the top k / S of the pixels
    insertion: torch.Tensor               # [N, S + 1] ... after inserting them onto the baseline
    deletion_auc: torch.Tensor            # [N]
    insertion_auc: torch.Tensor           # [N]
    average_drop: torch.Tensor            # [N] max(0, p - p_expl) / p
    increase: torch.Tensor                # [N] 1.0 where p_expl > p
    target: torch.Tensor                  # [N] int32: the class every image was scored on
    mean_deletion_auc: torch.Tensor       # 0-dim: the means over the N images
    mean_insertion_auc: torch.Tensor
    mean_average_drop: torch.Tensor
    mean_increase: torch.Tensor

    def cpu(self):
        return FaithfulnessResult(**{f.name: getattr(self, f.name).cpu() for f in fields(self)})


class CamFaithfulness:
    def __init__(self, model, device, steps=32, baseline="blur", blur_ksize=11, blur_sigma=5.0, chunk=None):
        """
        model: the loaded multimodal model (eval mode).
        device: the model's device.
        steps: S, the number of curve steps (1 .. 1024, at most H * W).
        baseline: what a deleted pixel becomes: "blur" = Gaussian blur of the image itself with reflect padding (blur_ksize odd
            and <= 31, blur_sigma; RISE uses 11 / 5), "zero" = the dataset mean in normalised space, "mean" = the image's own
            per-channel mean.
        chunk: rows per forward (the batch size of those forwards); the ragged last chunk is padded to it with zero rows.
        """
        self.model = model
        self.device = device
        self.steps = int(steps)
        if not 1 <= self.steps <= ops.FAITH_MAX_STEPS:
            raise ValueError(f"CamFaithfulness: steps must be in 1 .. {ops.FAITH_MAX_STEPS}, got {steps}")
        self._baseline = Baseline("CamFaithfulness", baseline, blur_ksize, blur_sigma)
        self.baseline, self.taps = baseline, self._baseline.taps
        self.chunk = chunk_or_default(chunk, "CamFaithfulness")

    def baseline_images(self, images):
        """images [N, 3, H, W] fp32 on the device -> the baseline of every image, same shape"""
        return self._baseline.images(images)

    def row_table(self, n_images):
        """int32 [N * (2 S + 3), 3] of (image, k, mode), image-major: deletion k = 0 .. S, insertion k = 0 .. S, explanation"""
        S = self.steps
        ks = np.concatenate([np.arange(S + 1), np.arange(S + 1), [0]])
        modes = np.concatenate([np.full(S + 1, ops.FAITH_DELETION), np.full(S + 1, ops.FAITH_INSERTION), [ops.FAITH_EXPLANATION]])
        per_image = np.stack([np.zeros_like(ks), ks, modes], axis=1)
        table = np.tile(per_image, (n_images, 1))
        table[:, 0] = np.repeat(np.arange(n_images), 2 * S + 3)
        return table.astype(np.int32)

    def evaluate(self, images, metadata, saliency, target_class=None):
        """images (N, 3, H, W) as the model takes them; metadata (N, V) or a mapping of such tensors; saliency (N, H, W), a float
        tensor or numpy array (any CAM class's output); target_class an int, an int tensor (N,), or None = the argmax of the
        clean forward, taken on the device -> FaithfulnessResult."""
        who = "CamFaithfulness.evaluate"
        check_images(images, who)
        N, _, H, W = images.shape
        if isinstance(saliency, np.ndarray):
            saliency = torch.from_numpy(saliency)
        if not torch.is_tensor(saliency) or not saliency.is_floating_point() or tuple(saliency.shape) != (N, H, W):
            raise ValueError(f"{who}: saliency must be a float tensor or array of shape {(N, H, W)}, got "
                             f"{(saliency.dtype, tuple(saliency.shape)) if torch.is_tensor(saliency) else type(saliency).__name__}")
        check_rows(metadata, N, who)
        S = self.steps
        if S > H * W:
            raise ValueError(f"{who}: {S} steps on an image of {H * W} pixels; steps must be <= H * W")
        if H * W > ops.faith_max_pixels():
            raise MMSkinError(f"{who}: {H}x{W} images are above the rank kernel's cap of {ops.faith_max_pixels()} pixels")
        require_eval(self.model, "CamFaithfulness")
        dev = self.device
        target = target_tensor(target_class, N, dev, who)

        images = images.detach().to(dev).float().contiguous()
        saliency = saliency.detach().to(dev).float().contiguous()
        rank = ops.faith_rank(saliency)
        base = self.baseline_images(images)

        P, chunk = 2 * S + 3, self.chunk
        R = N * P
        table = np.zeros((-(-R // chunk) * chunk, 3), dtype=np.int32)    # the padding rows point at image 0 and are never built
        table[:R] = self.row_table(N)
        rows = torch.from_numpy(table).to(dev)

        def write_chunk(r0, n, out):
            return ops.faith_perturb(images, base, rank, saliency, rows[r0:r0 + chunk], S, n, chunk, out=out)

        logits = chunked_logits(self.model, metadata, rows[:, 0].long(), R, chunk, write_chunk, who)
        check_target_range(target, logits.shape[1], who)
        curves, scalars, means, used = ops.faith_curves(logits, S, N, target)
        return FaithfulnessResult(deletion=curves[0], insertion=curves[1], deletion_auc=scalars[0], insertion_auc=scalars[1],
                                  average_drop=scalars[2], increase=scalars[3], target=used, mean_deletion_auc=means[0],
                                  mean_insertion_auc=means[1], mean_average_drop=means[2], mean_increase=means[3])


CAM_METHODS = ("gradcam", "gradcam++", "scorecam")


def cam_maps(model, target_layer, images, metadata, method, target, chunk=None):
    """The maps [N, H, W] (device, fp32) of one method on the existing classes of mmskin.cam; target: int tensor [N] on the
    device.  Score-CAM explains one image per call, so it loops over the images."""
    device = model_device(model)
    if method in ("gradcam", "gradcam++"):
        cam = (GradCAM if method == "gradcam" else GradCAMPlusPlus)(model, target_layer)
        try:
            return cam.generate_batch(images, metadata, target).detach()
        finally:
            cam.remove_hook()
    if method == "scorecam":
        cam = ScoreCAM(model, target_layer, device, chunk=chunk)
        try:
            classes = target.tolist()
            one = torch.arange(1, device=target.device)
            heats = [cam.generate_heatmap(images[i:i + 1], take_rows(metadata, one + i), classes[i]) for i in range(images.shape[0])]
        finally:
            cam.remove_hook()
        return torch.from_numpy(np.stack(heats)).to(device)
    raise ValueError(f"compare_cam_methods: method must be one of {CAM_METHODS}, got {method!r}")


def compare_cam_methods(model, target_layer, images, metadata, methods=CAM_METHODS, target_class=None, **kw):
    """The numerical form of the reference's cam_methods_comparison.py: the maps of every method in `methods` on the same images
    and target classes, each scored by one CamFaithfulness(model, device, **kw).

    target_class: an int, an int tensor [N], or None = the model's own prediction on the clean images (one forward, shared by
    all methods).  -> {method: {"maps": device tensor [N, H, W], "result": FaithfulnessResult}}"""
    require_eval(model, "compare_cam_methods")
    device = model_device(model)
    images = images.detach().to(device).float().contiguous()
    N = images.shape[0]
    check_rows(metadata, N, "compare_cam_methods")
    target = target_tensor(target_class, N, device, "compare_cam_methods", torch.long)
    if target is None:
        with torch.no_grad():
            target = model(images, metadata).argmax(dim=1)
    scorer = CamFaithfulness(model, device, **kw)
    out = {}
    for method in methods:
        maps = cam_maps(model, target_layer, images, metadata, method, target, chunk=kw.get("chunk"))
        out[method] = {"maps": maps, "result": scorer.evaluate(images, metadata, maps, target)}
    return out
