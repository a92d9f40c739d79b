"""LIME explanations of the metadata on the model itself, batched on the GPU.

The reference explains the metadata's contribution a second way (src/scripts/data_preprocessing/lime_padufes20.py): lime's
LimeTabularExplainer(training_data, mode="regression", discretize_continuous=False) and explain_instance(row, predict_fn,
num_features=15), again on the 300-tree random-forest SURROGATE of the recorded probabilities, because 5000 batch-1 forwards of
the real model per explained sample are out of reach.  Here predict_fn is the network: a batch's images are encoded ONCE
(`MultimodalModel.encode_image`), one HIP kernel writes a block of neighbourhood rows and their kernel weights
(mmskin.ops.lime_neighbourhood), the fusion head runs on the block (`MultimodalModel.fuse`), the block is added into the
weighted sums of the ridge problem on the device (mmskin.ops.lime_reduce), and one workgroup per (sample, class) selects the
features and fits them (mmskin.ops.lime_solve).

The algorithm is the published one, restated (include/mmskin.h has the formulas; parity with the `lime` package itself is
unpinned, it is not a dependency).  Features are the F = model.vocab_size ENCODED columns, one-hot cells and standardised
numerics alike, each a continuous feature -- what LIME does on the reference's script, and the deliberate difference from
mmskin.shapley, whose players are whole columns.  So a neighbourhood row is not a row a patient could have: LIME perturbs
every cell with Gaussian noise of the training set's mean and deviation.

    lime = MetadataLime(model, enc, device, training_rows)               # the encoded training rows [n, F]: mean / scale
    for images, rows in loader:                                          # rows = enc.transform(...), fp32 [B, F]
        res = lime.explain(images, rows)                                 # mean_abs accumulates over the batches
        res.as_list(0, 3, feature_names)                                 # the script's [(name, importance)] of sample 0, class 3
    importance, order = lime.global_importance()

Eval mode, forward only.
"""
import numpy as np
import torch

from . import _metadata_head as mh
from . import ops

OUTPUTS = {"prob": ops.LIME_PROB, "logit": ops.LIME_LOGIT}


class LimeResult(mh.AbsSum):
    """What `MetadataLime.explain` returns.  Per row of THIS batch, fp64 device tensors: `coef` [B, C, K] and `features` (int32)
    [B, C, K] in descending |coef| -- the explanation --, `intercept`, `score` (the weighted R^2 of the local fit), `local_pred`
    [B, C], `dense` [B, C, F] (coef scattered over all features, zeros where none was kept).  Accumulated since the last reset:
    `abs_sum` fp64 [F, C], `n_samples`, and `mean_abs` = abs_sum / n_samples."""

    def __init__(self, features, coef, intercept, score, local_pred, dense, abs_sum, n_samples):
        self.features, self.coef, self.intercept, self.score, self.local_pred = features, coef, intercept, score, local_pred
        self.dense, self.abs_sum, self.n_samples = dense, abs_sum, n_samples

    def as_list(self, b, c, feature_names=None):
        """lime's Explanation.as_list() of sample b for class c: [(name, importance)] in descending |importance|."""
        idx, val = self.features[b, c].tolist(), self.coef[b, c].tolist()
        if feature_names is not None and len(feature_names) != self.dense.shape[-1]:
            raise ValueError(f"as_list: {self.dense.shape[-1]} features, got {len(feature_names)} names")
        return [(feature_names[j] if feature_names is not None else str(j), v) for j, v in zip(idx, val)]


class MetadataLime(mh.AbsSum):
    # Rows per fusion-head call: the head is launch-bound on small blocks, and the [rows, F] image-feature
    # tile of a call is 64 MiB at F = 2048
    default_rows_per_head_call = 8192

    def __init__(self, model, encoder, device, training_rows, num_samples=5000, num_features=15, seed=0, output="prob",
                 sample_around_instance=False, rows_per_head_call=None):
        """
        model: the loaded MultimodalModel (eval mode, one-hot metadata, a fusion that reads the metadata).
        encoder: the fitted mmskin.preprocess.MetadataEncoder whose `transform` gives the rows (kept for the caller; rows narrower
            than the model's vocab_size are padded with zero columns by the caller, as the model's input is).
        device: the model's device.
        training_rows: the ENCODED training rows [n, F]; their mean and population deviation scale the neighbourhood.
        num_samples: N rows per explained sample, the explained row included (lime's default 5000).
        num_features: K features kept per (sample, class).  lime selects by forward selection for K <= 6, which is not built.
        seed: of the counter-based normal generator; explained sample i since the last reset() draws stream i.
        output: "prob" or "logit".  sample_around_instance: centre the rows on x instead of the training mean.
        rows_per_head_call: most rows one `model.fuse` call gets.
        """
        self.model, self.encoder, self.device = model, encoder, device
        rows = np.asarray(training_rows.cpu() if isinstance(training_rows, torch.Tensor) else training_rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 1:
            raise ValueError(f"MetadataLime: training_rows must be the encoded rows [n >= 1, F], got {rows.shape}")
        self.n_features = int(rows.shape[1])
        if self.n_features > ops.LIME_MAX_FEATURES:
            raise ValueError(f"MetadataLime: {self.n_features} features; the solver holds at most {ops.LIME_MAX_FEATURES}")
        self.mean, self.scale = self.fit_scaler(rows)
        self.kernel_width = 0.75 * np.sqrt(self.n_features)
        self.num_samples, self.num_features = int(num_samples), int(num_features)
        if self.num_samples < 2:
            raise ValueError(f"MetadataLime: num_samples must be >= 2, got {num_samples}")
        if self.num_features <= 6:
            raise ValueError(f"MetadataLime: num_features = {num_features}: for num_features <= 6 lime selects by forward_selection, which is "
                             "not built; highest_weights needs num_features >= 7")
        self.num_features = min(self.num_features, self.n_features)              # num_features >= F keeps every feature
        if output not in OUTPUTS:
            raise ValueError(f"MetadataLime: output must be 'prob' or 'logit', got {output!r}")
        self.output, self.seed, self.sample_around_instance = output, int(seed), bool(sample_around_instance)
        self.rows_per_head_call = mh.rows_per_call("MetadataLime", "rows_per_head_call", rows_per_head_call, self.default_rows_per_head_call)
        self.reset()

    @staticmethod
    def fit_scaler(rows):
        """(mean, scale) fp64 [F] of sklearn's StandardScaler: the population deviation, 0 replaced by 1."""
        rows = np.asarray(rows, dtype=np.float64)
        mean, scale = rows.mean(axis=0), rows.std(axis=0)
        scale[scale == 0.0] = 1.0
        return mean, scale

    # ---- per batch
    def explain(self, images, encoded_rows):
        """One batch: images [B, ...] as the model takes them, encoded_rows fp32 [B, F] (MetadataEncoder.transform).  Adds the batch's
        |coef| to the running sums and returns a LimeResult."""
        model = self.model
        mh.check_metadata_model("MetadataLime", model, "explain")
        F, N, K = self.n_features, self.num_samples, self.num_features
        if F != model.vocab_size:
            raise ValueError(f"MetadataLime: the training rows have {F} columns, the model's vocab_size is {model.vocab_size}")
        x = torch.as_tensor(encoded_rows)
        B = int(images.shape[0])
        if tuple(x.shape) != (B, F):
            raise ValueError(f"MetadataLime.explain: a batch of {B} images needs encoded rows {(B, F)}, got {tuple(x.shape)}")
        C = int(model.num_classes)
        if self.abs_sum is not None and tuple(self.abs_sum.shape) != (F, C):
            raise ValueError(f"MetadataLime.explain: the sums hold {tuple(self.abs_sum.shape)} features x classes; call reset() first")
        total = B * N
        with torch.no_grad():
            img_feat = model.encode_image(images)
            dev = img_feat.device
            x = x.to(device=dev, dtype=torch.float32).contiguous()
            mean, scale = torch.from_numpy(self.mean).to(dev), torch.from_numpy(self.scale).to(dev)
            acc = ops.lime_accumulator(B, N, F, C, dev)
            if self.abs_sum is None:
                self.abs_sum = torch.zeros((F, C), dtype=torch.float64, device=dev)
            for r0 in range(0, total, self.rows_per_head_call):
                r1 = min(r0 + self.rows_per_head_call, total)
                metas, weights = ops.lime_neighbourhood(x, mean, scale, N, self.seed, row0=r0, row1=r1, sample0=self.n_samples,
                                                        around_instance=self.sample_around_instance)
                # the image-feature tile of THIS call only: row -> its sample
                sample = torch.div(torch.arange(r0, r1, device=dev), N, rounding_mode="floor")
                logits = mh.head_logits(model, img_feat.index_select(0, sample), metas)
                ops.lime_reduce(metas, weights, logits, mean, scale, acc, B, N, r0, output=OUTPUTS[self.output])
            coef, feature, intercept, score, local_pred, dense = ops.lime_solve(acc, x, mean, scale, N, C, K, abs_sum=self.abs_sum)
        self.n_samples += B
        return LimeResult(feature, coef, intercept, score, local_pred, dense, self.abs_sum, self.n_samples)
