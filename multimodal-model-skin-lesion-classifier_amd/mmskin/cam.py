"""Score-CAM with the reference's class and call (interpretability/ScoreCam.py:62-155), batched on the GPU.

The reference explains one image with C batch-1 forwards, a device-to-host `.item()` and a full-size `.cpu().numpy()` copy per
channel, and sums the weighted maps in numpy.  Here the C masked images are built in chunks by one HIP kernel
(mmskin.ops.scorecam_mask), each chunk is one batched forward of the model on its un-hooked eval plan, the soft-max scores
stay on the device, and one kernel pair sums, rectifies and normalises the heat map (mmskin.ops.scorecam_combine): one host
copy per explained image.  The normalised upsampled maps are never stored; the kernels recompute them from the feature map.

Eval mode, forward only: nothing here is differentiable.
"""
from collections.abc import Mapping

import torch

from . import ops
from ._lib import MMSkinError


def _expand_batch(metadata, n):
    """metadata of batch 1 -> batch n: a tensor (1, V), or a mapping of such tensors (the tokenizer's BatchEncoding)."""
    if isinstance(metadata, Mapping):
        return {k: _expand_batch(v, n) for k, v in metadata.items()}
    if torch.is_tensor(metadata):
        if metadata.dim() == 0 or metadata.shape[0] != 1:
            raise ValueError(f"ScoreCAM: metadata must have batch 1, got shape {tuple(metadata.shape)}")
        return metadata.expand(n, *metadata.shape[1:]).contiguous()
    return metadata


class ScoreCAM:
    # Channels per masked forward: the fastest of 64 / 128 / 256 on densenet169 + crossattention at 224x224
    default_chunk = 256

    def __init__(self, model, target_layer, device, chunk=None):
        """
        model: the loaded multimodal model (eval mode).
        target_layer: the layer to hook for feature maps: the last conv of a ResNet encoder, `image_encoder.features[-1]` of
            DenseNet, or any ordinary nn.Module layer that returns a 4-D map.
        device: the model's device.
        chunk: channels per masked forward (the batch size of those forwards); the ragged last chunk is padded to it.
        """
        self.model = model
        self.target_layer = target_layer
        self.device = device
        self.chunk = int(chunk) if chunk is not None else self.default_chunk
        if self.chunk < 1:
            raise ValueError(f"ScoreCAM: chunk must be >= 1, got {chunk}")
        self.features = None
        self.scores = None           # soft-max score of the target class per channel, device tensor [C], after generate_heatmap
        self.hook_handle = self.target_layer.register_forward_hook(self.hook_fn)

    def hook_fn(self, module, input, output):
        self.features = output.detach()

    def remove_hook(self):
        self.hook_handle.remove()

    def forward(self, image, metadata):
        self.features = None
        return self.model(image, metadata)

    def generate_heatmap(self, image, metadata, target_class):
        """image (1, 3, H, W), metadata (1, V) or a mapping of batch-1 tensors -> np.ndarray [H, W] float32 in [0, 1].
        A combined map that is flat comes back as NaN, as in the reference (no zero guard on the last division)."""
        if image.dim() != 4 or image.shape[0] != 1 or image.shape[1] != 3:
            raise ValueError(f"ScoreCAM.generate_heatmap: image must have shape (1, 3, H, W), got {tuple(image.shape)}: the "
                             "per-channel min-max of the reference is only meaningful for one image")
        if self.model.training:
            raise MMSkinError("ScoreCAM runs in eval mode: call model.eval() first")
        image = image.to(self.device).float().contiguous()
        H, W = image.shape[2:]

        _ = self.forward(image, metadata)
        fmap = self.features
        if fmap is None:
            raise MMSkinError("ScoreCAM: the forward hook on target_layer did not fire")
        if not torch.is_tensor(fmap) or fmap.dim() != 4 or fmap.shape[0] != 1:
            raise MMSkinError("ScoreCAM: target_layer must deliver a (1, C, fh, fw) feature map, got "
                              f"{tuple(fmap.shape) if torch.is_tensor(fmap) else type(fmap).__name__}")
        fmap = fmap[0].float().contiguous()
        C = fmap.shape[0]
        minmax = ops.scorecam_minmax(fmap, (H, W))
        scores = torch.empty(C, device=fmap.device, dtype=torch.float32)
        chunk = self.chunk
        meta = _expand_batch(metadata, chunk)
        masked = torch.empty((chunk, 3, H, W), device=fmap.device, dtype=torch.float32)

        # the masked forwards run without the hook: the encoder then takes its BatchNorm-folded eval plan, not the hooked route
        self.hook_handle.remove()
        try:
            with torch.no_grad():
                for c0 in range(0, C, chunk):
                    n = min(chunk, C - c0)
                    ops.scorecam_mask(fmap, minmax, image[0], c0, n, chunk, out=masked)
                    probs = torch.softmax(self.model(masked, meta).float(), dim=1)
                    scores[c0:c0 + n] = probs[:n, target_class]          # the padded rows' scores are dropped
        finally:
            self.hook_handle = self.target_layer.register_forward_hook(self.hook_fn)
        self.scores = scores
        return ops.scorecam_combine(fmap, minmax, scores, (H, W)).cpu().numpy()
