"""Score-CAM with the reference's class and call (interpretability/ScoreCam.py:62-155), batched on the GPU.

The reference explains one image with C batch-1 forwards, a device-to-host `.item()` and a full-size `.cpu().numpy()` copy per
channel, and sums the weighted maps in numpy.  Here the C masked images are built in chunks by one HIP kernel
(mmskin.ops.scorecam_mask), each chunk is one batched forward of the model on its un-hooked eval plan, the soft-max scores
stay on the device, and one kernel pair sums, rectifies and normalises the heat map (mmskin.ops.scorecam_combine): one host
copy per explained image.  The normalised upsampled maps are never stored; the kernels recompute them from the feature map.

Eval mode, forward only: nothing here is differentiable.

Grad-CAM and Grad-CAM++ with the reference's classes and call (interpretability/gradcam_atualizado.py:201-306), batched over
images and metadata variants (`GradCAM`, `GradCAMPlusPlus`).  The reference runs the whole model twice and one backward per
(image, variant) pair (multiple_sample_using_gradcam_plusplus_atualizado.py:341-399: 30 encoder passes for one image with 15
variants).  The activations at the target layer do not depend on the metadata, and on the two targets the encoders' plans
support -- the last conv of a ResNet, `image_encoder.features[-1]` of DenseNet-169 -- the tail from the activations to the
pooled features is diagonal in the channel.  So `generate_batch` encodes every image ONCE through the hooked eval route, takes
J = d sum(features) / d activations in one backward, runs the fusion head once on all R = images x variants rows
(`MultimodalModel.fuse`) and one head backward for d score / d features, and two HIP kernels (mmskin.ops.gradcam_weights,
gradcam_map) form the gradient J * dfeat in registers, the channel weights, the weighted sum, and the normalised upsampled
maps.  Any other layer that delivers a 4-D map takes the generic route: the whole model at batch R, autograd's gradient at the
layer, the same kernels.  Out of scope: second-order differentiation (the reference squares and cubes the first-order gradient
and never differentiates again), DenseNet's `find_last_conv` target, and the MBConv / VGG plans, whose encoders run no hooks.
"""
import torch
import torch.nn as nn

from . import ops
from ._image_explainer import (DEFAULT_CHUNK, check_images, check_rows, check_target_range, chunk_or_default, expand_batch,
                               model_device, require_eval, target_tensor)
from ._lib import MMSkinError
from .backbone import RESNET_DEPTHS, _FlatBackbone


class ScoreCAM:
    default_chunk = DEFAULT_CHUNK

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
        self.chunk = chunk_or_default(chunk, "ScoreCAM")
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
        check_images(image, "ScoreCAM.generate_heatmap", one=True,
                     why=": the per-channel min-max of the reference is only meaningful for one image")
        require_eval(self.model, "ScoreCAM")
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
        meta = expand_batch(metadata, chunk, "ScoreCAM")
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


class _GradCAMBase:
    """The reference's BaseCAM (gradcam_atualizado.py:201-224): a forward hook on target_layer keeps the activations."""
    mode = None

    def __init__(self, model, target_layer):
        """
        model: the loaded multimodal model (eval mode).
        target_layer: the last conv of a ResNet encoder or `image_encoder.features[-1]` of DenseNet-169 (one encoder pass per
            image), or any ordinary nn.Module layer that returns a 4-D map (the whole model runs on every row).
        """
        self.model = model
        self.target_layer = target_layer
        self.activations = None
        self.weights = None          # after generate_batch, device tensors: channel weights [R, C]
        self.raw = None              # the weighted sums before ReLU and normalisation [R, fh, fw]
        self.pred = None             # predicted class of every row [R] (argmax of the logits)
        self.probs = None            # soft-max of the logits [R, K]
        self._fh = self.target_layer.register_forward_hook(self._forward_hook)

    def _forward_hook(self, module, input, output):
        self.activations = output

    def clear(self):
        self.activations = None
        self.weights = self.raw = self.pred = self.probs = None

    def remove_hook(self):
        self._fh.remove()

    def _on_plan_route(self):
        """The one place the route is chosen: True when target_layer is a target the encoder's plan serves through its hooked
        eval route AND the tail behind it is diagonal in the channel (ResNet: BN(eval) + skip + ReLU + average pool; DenseNet
        features[-1]: ReLU + average pool), with the model split at encode_image / fuse."""
        enc = getattr(self.model, "image_encoder", None)
        if not isinstance(enc, _FlatBackbone) or not hasattr(self.model, "encode_image") or not hasattr(self.model, "fuse"):
            return False
        if enc.arch in RESNET_DEPTHS:
            convs = [m for m in enc.modules() if isinstance(m, nn.Conv2d)]
            return bool(convs) and self.target_layer is convs[-1]
        if enc.arch == "densenet169":
            feats = getattr(enc, "features", None)
            return isinstance(feats, nn.Sequential) and len(feats) > 0 and self.target_layer is feats[-1]
        return False

    def _taken_activations(self, rows):
        acts = self.activations
        who = type(self).__name__
        if acts is None:
            raise MMSkinError(f"{who}: the forward hook on target_layer did not fire")
        if not torch.is_tensor(acts) or acts.dim() != 4 or acts.shape[0] != rows:
            raise MMSkinError(f"{who}: target_layer must deliver a ({rows}, C, fh, fw) feature map, got "
                              f"{tuple(acts.shape) if torch.is_tensor(acts) else type(acts).__name__}")
        if not acts.requires_grad:
            raise MMSkinError(f"{who}: the activations of target_layer are not part of the autograd graph")
        return acts

    def _selected(self, logits, target_class, rows):
        """(the logit every row is explained by [rows], argmax [rows], soft-max [rows, K]), all on the device"""
        who = type(self).__name__
        if logits.dim() != 2 or logits.shape[0] != rows:
            raise MMSkinError(f"{who}: the model must return logits of shape ({rows}, K), got {tuple(logits.shape)}")
        K = logits.shape[1]
        pred = logits.detach().argmax(dim=1)
        index = target_tensor(target_class, rows, logits.device, who, torch.long)
        check_target_range(target_class, K, who)
        if index is None:
            index = pred
        return logits.gather(1, index[:, None])[:, 0], pred, torch.softmax(logits.detach().float(), dim=1)

    def generate_batch(self, images, metadata, target_class=None, variants_per_image=1):
        """images (N, 3, H, W); metadata of R = N * variants_per_image rows, image-major (rows n * V .. n * V + V - 1 belong to
        image n): a tensor or a mapping of tensors; target_class an int, an int tensor [R], or None = every row's own predicted
        class, taken on the device from the same head forward -> device tensor [R, H, W] float32 in [0, 1].

        Every row is normalised on its own, so row r equals the reference's `generate(images[n:n + 1], metadata[r:r + 1], t_r)`
        run row by row.  Leaves self.weights [R, C], self.raw [R, fh, fw], self.pred [R], self.probs [R, K] and the detached
        self.activations on the object; nothing is copied to the host."""
        who = type(self).__name__
        model = self.model
        check_images(images, f"{who}.generate_batch")
        V = int(variants_per_image)
        if V < 1:
            raise ValueError(f"{who}.generate_batch: variants_per_image must be >= 1, got {variants_per_image}")
        require_eval(model, who)
        N = images.shape[0]
        R = N * V
        check_rows(metadata, R, f"{who}.generate_batch")
        device = model_device(model)
        images = images.detach().to(device).float().contiguous()
        H, W = images.shape[2:]
        self.clear()
        try:
            with torch.enable_grad():
                if self._on_plan_route():
                    feats = model.encode_image(images)                              # the one encoder pass; the hook delivers A
                    acts = self._taken_activations(N)
                    jac, = torch.autograd.grad(feats.sum(), acts)
                    tiled = feats.detach().repeat_interleave(V, dim=0).requires_grad_(True)
                    selected, pred, probs = self._selected(model.fuse(tiled, metadata), target_class, R)
                    dfeat, = torch.autograd.grad(selected.sum(), tiled)
                    dfeat = dfeat.float().contiguous()
                    row_image = torch.arange(N, device=device, dtype=torch.int32).repeat_interleave(V)
                else:
                    logits = model(images.repeat_interleave(V, dim=0) if V > 1 else images, metadata)
                    acts = self._taken_activations(R)
                    selected, pred, probs = self._selected(logits, target_class, R)
                    jac, = torch.autograd.grad(selected.sum(), acts)
                    dfeat = None
                    row_image = torch.arange(R, device=device, dtype=torch.int32)
        except BaseException:
            self.clear()             # no half-built graph stays on the object; the hook stays on the layer
            raise
        acts = acts.detach().float().contiguous()
        weights = ops.gradcam_weights(acts, jac.detach().float().contiguous(), dfeat, row_image, self.mode)
        raw, cam = ops.gradcam_map(acts, weights, row_image, (H, W))
        self.activations, self.weights, self.raw, self.pred, self.probs = acts, weights, raw, pred, probs
        return cam

    def generate(self, image, metadata, target_class):
        """image (1, 3, H, W), metadata of one row, target_class an int -> np.ndarray [H, W] float32 in [0, 1]: the reference's
        call and result; the R = 1 case of generate_batch."""
        check_images(image, f"{type(self).__name__}.generate", one=True,
                     why=": the min-max of the reference runs over the whole batch and is only meaningful for one image "
                         "(generate_batch normalises every row on its own)")
        return self.generate_batch(image, metadata, target_class)[0].cpu().numpy()


class GradCAM(_GradCAMBase):
    """weights = mean of the gradient over the map (gradcam_atualizado.py:230-257)"""
    mode = ops.GRADCAM


class GradCAMPlusPlus(_GradCAMBase):
    """weights = sum of alpha * relu(gradient), alpha = g^2 / (2 g^2 + sum(A g^3) + 1e-8) (gradcam_atualizado.py:263-306)"""
    mode = ops.GRADCAM_PLUSPLUS
