"""What the analyses that run the fusion head on many metadata rows of an image encoded once have in common (mmskin.sweep,
shapley, lime, permutation, uncertainty): the refusals they open with, the argument checks, the head call, and the running
|value| sums.  `who` is the caller's class name: every message keeps the caller's name in front."""
import torch

from ._lib import MMSkinError


def check_metadata_model(who, model, verb):
    """The model must be in eval mode, take encoded one-hot rows, and have a fusion that reads them; `verb` is what the caller
    does with the metadata ("sweep", "explain")."""
    if model.training:
        raise MMSkinError(f"{who} runs in eval mode: call model.eval() first")
    if getattr(model, "text_model_name", None) != "one-hot-encoder":
        raise ValueError(f"{who} is defined on encoded one-hot rows: text_model_name is {getattr(model, 'text_model_name', None)!r}, "
                         "not 'one-hot-encoder'")
    if model.attention_mecanism in ("no-metadata", "no-metadata-without-mlp"):
        raise ValueError(f"{who}: the fusion {model.attention_mecanism!r} does not read the metadata, there is nothing to {verb}")


def rows_per_call(who, name, value, default):
    """The constructor argument `name` (most rows of one model call): an int >= 1, or `default` for None."""
    rows = int(value) if value is not None else default
    if rows < 1:
        raise ValueError(f"{who}: {name} must be >= 1, got {value}")
    return rows


def check_columns(who, encoder, categorical_columns, numeric_columns):
    """The two lists of names, which must name the encoder's columns in its order; `who` is the method the names were given to."""
    cats, nums = list(categorical_columns), list(numeric_columns)
    if len(cats) != len(encoder.categories_) or len(nums) != len(encoder.mean_):
        raise ValueError(f"{who}: the encoder has {len(encoder.categories_)} categorical + {len(encoder.mean_)} "
                         f"numeric columns, got {len(cats)} + {len(nums)} names")
    return cats, nums


def batch_codes(who, B, encoder, codes, numeric):
    """codes [B, n_cat] and numeric [B, n_num] of a batch of B images, as tensors; `who` is the method they were given to."""
    n_cat, n_num = len(encoder.categories_), len(encoder.mean_)
    codes, numeric = torch.as_tensor(codes), torch.as_tensor(numeric)
    if tuple(codes.shape) != (B, n_cat) or tuple(numeric.shape) != (B, n_num):
        raise ValueError(f"{who}: a batch of {B} images needs codes {(B, n_cat)} and numeric {(B, n_num)}, got "
                         f"{tuple(codes.shape)} and {tuple(numeric.shape)}")
    return codes, numeric


def head_logits(model, feats, metas, fp32=False):
    """model.fuse on the rows, contiguous, in a dtype the reduce kernels read: fp32 or bf16 as the head gives them, anything
    else (and everything, with `fp32`) converted to fp32."""
    logits = model.fuse(feats, metas)
    if fp32 or logits.dtype not in (torch.float32, torch.bfloat16):
        logits = logits.float()
    return logits.contiguous()


class AbsSum:
    """The running fp64 sums of |value| [features, classes] over the explained samples: `abs_sum` (None until the first batch)
    and `n_samples`."""

    def reset(self):
        """Forget the accumulated |values| (a new data set)."""
        self.abs_sum = None
        self.n_samples = 0

    @property
    def mean_abs(self):
        return self.abs_sum / max(self.n_samples, 1)

    def global_importance(self):
        """(importance = mean_abs averaged over the classes, the features in descending order of it, ties to the lower index)"""
        if self.abs_sum is None:
            raise ValueError("global_importance: nothing has been explained since the last reset()")
        importance = self.mean_abs.mean(-1)
        return importance, torch.argsort(importance, descending=True, stable=True)
