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
from collections.abc import Mapping
from dataclasses import dataclass, fields

import numpy as np
import torch

from . import ops
from ._lib import MMSkinError
from .cam import GradCAM, GradCAMPlusPlus, ScoreCAM, _check_rows

BASELINES = ("blur", "zero", "mean")


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


def _take_rows(metadata, index):
    """rows `index` (a long device tensor) of a metadata tensor, or of every tensor of a mapping"""
    if isinstance(metadata, Mapping):
        return {k: _take_rows(v, index) for k, v in metadata.items()}
    if torch.is_tensor(metadata):
        return metadata.to(index.device).index_select(0, index)
    return metadata


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
        if baseline not in BASELINES:
            raise ValueError(f"CamFaithfulness: baseline must be one of {BASELINES}, got {baseline!r}")
        self.baseline = baseline
        self.taps = ops.gaussian_taps(blur_ksize, blur_sigma) if baseline == "blur" else None
        self.chunk = int(chunk) if chunk is not None else ScoreCAM.default_chunk
        if self.chunk < 1:
            raise ValueError(f"CamFaithfulness: chunk must be >= 1, got {chunk}")

    def baseline_images(self, images):
        """images [N, 3, H, W] fp32 on the device -> the baseline of every image, same shape"""
        if self.baseline == "blur":
            return ops.faith_blur(images, self.taps)
        if self.baseline == "mean":
            return ops.faith_mean(images)
        return torch.zeros_like(images)

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
        if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3 or images.shape[0] < 1:
            raise ValueError(f"{who}: images must have shape (N, 3, H, W), got "
                             f"{tuple(images.shape) if torch.is_tensor(images) else type(images).__name__}")
        N, _, H, W = images.shape
        if isinstance(saliency, np.ndarray):
            saliency = torch.from_numpy(saliency)
        if not torch.is_tensor(saliency) or not saliency.is_floating_point() or tuple(saliency.shape) != (N, H, W):
            raise ValueError(f"{who}: saliency must be a float tensor or array of shape {(N, H, W)}, got "
                             f"{(saliency.dtype, tuple(saliency.shape)) if torch.is_tensor(saliency) else type(saliency).__name__}")
        _check_rows(metadata, N, who)
        S = self.steps
        if S > H * W:
            raise ValueError(f"{who}: {S} steps on an image of {H * W} pixels; steps must be <= H * W")
        if H * W > ops.faith_max_pixels():
            raise MMSkinError(f"{who}: {H}x{W} images are above the rank kernel's cap of {ops.faith_max_pixels()} pixels")
        if self.model.training:
            raise MMSkinError("CamFaithfulness runs in eval mode: call model.eval() first")
        dev = self.device
        target = None
        if target_class is not None:
            if torch.is_tensor(target_class):
                if target_class.dim() != 1 or target_class.shape[0] != N or target_class.is_floating_point():
                    raise ValueError(f"{who}: target_class must be an int, None or an int tensor [{N}], got "
                                     f"{target_class.dtype} {tuple(target_class.shape)}")
                target = target_class.to(dev).to(torch.int32).contiguous()
            else:
                target = torch.full((N,), int(target_class), device=dev, dtype=torch.int32)

        images = images.detach().to(dev).float().contiguous()
        saliency = saliency.detach().to(dev).float().contiguous()
        rank = ops.faith_rank(saliency)
        base = self.baseline_images(images)

        P, chunk = 2 * S + 3, self.chunk
        R = N * P
        n_chunks = -(-R // chunk)
        table = np.zeros((n_chunks * chunk, 3), dtype=np.int32)          # the padding rows point at image 0 and are never built
        table[:R] = self.row_table(N)
        rows = torch.from_numpy(table).to(dev)
        row_image = rows[:, 0].long()
        masked = torch.empty((chunk, 3, H, W), device=dev, dtype=torch.float32)
        logits = None
        with torch.no_grad():
            for c in range(n_chunks):
                r0 = c * chunk
                ops.faith_perturb(images, base, rank, saliency, rows[r0:r0 + chunk], S, min(chunk, R - r0), chunk, out=masked)
                out = self.model(masked, _take_rows(metadata, row_image[r0:r0 + chunk]))
                if logits is None:
                    if out.dim() != 2 or out.shape[0] != chunk:
                        raise MMSkinError(f"{who}: the model must return logits of shape ({chunk}, K), got {tuple(out.shape)}")
                    logits = torch.empty((n_chunks * chunk, out.shape[1]), device=dev, dtype=torch.float32)
                logits[r0:r0 + chunk] = out                              # the padded rows' logits are never read
        K = logits.shape[1]
        if target is not None and bool(((target < 0) | (target >= K)).any()):       # checked where the tensor lives
            raise ValueError(f"{who}: target_class has entries outside 0 .. {K - 1}")
        curves, scalars, means, used = ops.faith_curves(logits, S, N, target)
        return FaithfulnessResult(deletion=curves[0], insertion=curves[1], deletion_auc=scalars[0], insertion_auc=scalars[1],
                                  average_drop=scalars[2], increase=scalars[3], target=used, mean_deletion_auc=means[0],
                                  mean_insertion_auc=means[1], mean_average_drop=means[2], mean_increase=means[3])


CAM_METHODS = ("gradcam", "gradcam++", "scorecam")


def cam_maps(model, target_layer, images, metadata, method, target, chunk=None):
    """The maps [N, H, W] (device, fp32) of one method on the existing classes of mmskin.cam; target: int tensor [N] on the
    device.  Score-CAM explains one image per call, so it loops over the images."""
    device = getattr(model, "device", None) or next(model.parameters()).device
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
            heats = [cam.generate_heatmap(images[i:i + 1], _take_rows(metadata, one + i), classes[i]) for i in range(images.shape[0])]
        finally:
            cam.remove_hook()
        return torch.from_numpy(np.stack(heats)).to(device)
    raise ValueError(f"compare_cam_methods: method must be one of {CAM_METHODS}, got {method!r}")


def compare_cam_methods(model, target_layer, images, metadata, methods=CAM_METHODS, target_class=None, **kw):
    """The numerical form of the reference's cam_methods_comparison.py: the maps of every method in `methods` on the same images
    and target classes, each scored by one CamFaithfulness(model, device, **kw).

    target_class: an int, an int tensor [N], or None = the model's own prediction on the clean images (one forward, shared by
    all methods).  -> {method: {"maps": device tensor [N, H, W], "result": FaithfulnessResult}}"""
    if model.training:
        raise MMSkinError("compare_cam_methods runs in eval mode: call model.eval() first")
    device = getattr(model, "device", None) or next(model.parameters()).device
    images = images.detach().to(device).float().contiguous()
    N = images.shape[0]
    _check_rows(metadata, N, "compare_cam_methods")
    if target_class is None:
        with torch.no_grad():
            target = model(images, metadata).argmax(dim=1)
    elif torch.is_tensor(target_class):
        target = target_class.to(device).long()
    else:
        target = torch.full((N,), int(target_class), device=device, dtype=torch.long)
    scorer = CamFaithfulness(model, device, **kw)
    out = {}
    for method in methods:
        maps = cam_maps(model, target_layer, images, metadata, method, target, chunk=kw.get("chunk"))
        out[method] = {"maps": maps, "result": scorer.evaluate(images, metadata, maps, target)}
    return out
