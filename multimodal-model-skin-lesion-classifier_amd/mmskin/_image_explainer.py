"""What the explainers that perturb the image and run the model on every perturbed copy have in common (mmskin.cam, faithfulness,
rise): the argument checks, the target-class contract, the baseline a perturbed pixel fades to, the metadata rows of a chunk,
and the chunked forward loop.  `who` is the caller's name: every message keeps it in front."""
from collections.abc import Mapping

import torch

from . import ops
from ._lib import MMSkinError

BASELINES = ("blur", "zero", "mean")
# Rows per masked forward: the fastest of 64 / 128 / 256 on densenet169 + crossattention at 224x224
DEFAULT_CHUNK = 256


def check_images(images, who, one=False, why=""):
    """images (N, 3, H, W) with N >= 1, or with `one` exactly (1, 3, H, W); `why` is the caller's own reason, appended."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3 or (images.shape[0] != 1 if one else images.shape[0] < 1):
        want = "image must have shape (1, 3, H, W)" if one else "images must have shape (N, 3, H, W)"
        raise ValueError(f"{who}: {want}, got {tuple(images.shape) if torch.is_tensor(images) else type(images).__name__}{why}")


def check_rows(metadata, rows, who):
    """metadata of `rows` rows: a tensor (rows, V), or a mapping of such tensors"""
    if isinstance(metadata, Mapping):
        for v in metadata.values():
            check_rows(v, rows, who)
    elif torch.is_tensor(metadata) and (metadata.dim() == 0 or metadata.shape[0] != rows):
        raise ValueError(f"{who}: metadata must have {rows} rows (images x variants_per_image, image-major), got shape "
                         f"{tuple(metadata.shape)}")


def take_rows(metadata, index):
    """rows `index` (a long device tensor) of a metadata tensor, or of every tensor of a mapping"""
    if isinstance(metadata, Mapping):
        return {k: take_rows(v, index) for k, v in metadata.items()}
    if torch.is_tensor(metadata):
        return metadata.to(index.device).index_select(0, index)
    return metadata


def expand_batch(metadata, n, who):
    """metadata of batch 1 -> batch n: a tensor (1, V), or a mapping of such tensors (the tokenizer's BatchEncoding)."""
    if isinstance(metadata, Mapping):
        return {k: expand_batch(v, n, who) for k, v in metadata.items()}
    if torch.is_tensor(metadata):
        if metadata.dim() == 0 or metadata.shape[0] != 1:
            raise ValueError(f"{who}: metadata must have batch 1, got shape {tuple(metadata.shape)}")
        return metadata.expand(n, *metadata.shape[1:]).contiguous()
    return metadata


def target_tensor(target_class, N, device, who, dtype=torch.int32):
    """target_class an int, an int tensor [N], or None -> a `dtype` tensor [N] on the device, or None"""
    if target_class is None:
        return None
    if torch.is_tensor(target_class):
        if target_class.dim() != 1 or target_class.shape[0] != N or target_class.is_floating_point():
            raise ValueError(f"{who}: target_class must be an int, None or an int tensor [{N}], got "
                             f"{target_class.dtype} {tuple(target_class.shape)}")
        return target_class.to(device).to(dtype).contiguous()
    return torch.full((N,), int(target_class), device=device, dtype=dtype)


def check_target_range(target, K, who):
    """Every class of `target` (None, an int, or an int tensor, which is checked where it lives) must be one of the K."""
    if torch.is_tensor(target):
        if bool(((target < 0) | (target >= K)).any()):
            raise ValueError(f"{who}: target_class has entries outside 0 .. {K - 1}")
    elif target is not None and not 0 <= int(target) < K:
        raise ValueError(f"{who}: target_class {target} is outside 0 .. {K - 1}")


def require_eval(model, who):
    if model.training:
        raise MMSkinError(f"{who} runs in eval mode: call model.eval() first")


def model_device(model):
    return getattr(model, "device", None) or next(model.parameters()).device


class Baseline:
    """What a perturbed pixel fades to: "blur" = Gaussian blur of the image itself with reflect padding (blur_ksize odd and
    <= 31, blur_sigma), "zero" = the dataset mean in normalised space, "mean" = the image's own per-channel mean."""

    def __init__(self, who, name, blur_ksize, blur_sigma):
        if name not in BASELINES:
            raise ValueError(f"{who}: baseline must be one of {BASELINES}, got {name!r}")
        self.name = name
        self.taps = ops.gaussian_taps(blur_ksize, blur_sigma) if name == "blur" else None

    def images(self, images):
        """images [N, 3, H, W] fp32 on the device -> the baseline of every image, same shape"""
        if self.name == "blur":
            return ops.faith_blur(images, self.taps)
        if self.name == "mean":
            return ops.faith_mean(images)
        return torch.zeros_like(images)


def chunk_or_default(chunk, who):
    """The constructor argument `chunk` (rows per forward): an int >= 1, or DEFAULT_CHUNK for None."""
    rows = int(chunk) if chunk is not None else DEFAULT_CHUNK
    if rows < 1:
        raise ValueError(f"{who}: chunk must be >= 1, got {chunk}")
    return rows


def chunked_logits(model, metadata, row_image, n_rows, chunk, write_chunk, who, K=None):
    """The model's logits on n_rows perturbed images, `chunk` rows per forward -> fp32 [n_chunks * chunk, K] on the device; the
    ragged last chunk is padded and the padded rows' logits are never read.  `masked = write_chunk(r0, n, masked)` fills the
    one [chunk, 3, H, W] buffer with rows r0 .. r0 + n (None on the first call: the op allocates it); row_image [n_chunks *
    chunk] long names the image, and so the metadata row, of every row.  K: the width every chunk's logits must have, when the
    caller knows it; without it the first chunk's shape is checked and sets the width."""
    n_chunks = -(-n_rows // chunk)
    masked = logits = None
    with torch.no_grad():
        for r0 in range(0, n_chunks * chunk, chunk):
            masked = write_chunk(r0, min(chunk, n_rows - r0), masked)
            out = model(masked, take_rows(metadata, row_image[r0:r0 + chunk]))
            wrong = out.dim() != 2 or out.shape[0] != chunk or (K is not None and out.shape[1] != K)
            if wrong and (K is not None or logits is None):
                raise MMSkinError(f"{who}: the model must return logits of shape ({chunk}, {'K' if K is None else K}), got "
                                  f"{tuple(out.shape)}")
            if logits is None:
                logits = torch.empty((n_chunks * chunk, out.shape[1]), device=row_image.device, dtype=torch.float32)
            logits[r0:r0 + chunk] = out
    return logits
