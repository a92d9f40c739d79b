"""Permutation importance of the metadata on a validation fold, on the model itself, batched on the GPU.

How much of a fold's accuracy, balanced accuracy and AUC does each metadata feature carry?  Breiman's answer, as
sklearn.inspection.permutation_importance states it: shuffle the feature among the fold's samples, score the fold again, and
take the drop; repeat R times.  The reference approaches the question with the missing-metadata degradation
(src/scripts/interpretability/inference_all_folds.py) and with a global ranking on a random-forest surrogate
(src/scripts/data_preprocessing/shap_values.py), because features x repeats validation passes of the network were out of reach.
Here the fold's images are encoded ONCE (`MultimodalModel.encode_image`); per block of rows one HIP kernel writes the shuffled
encoded metadata (mmskin.ops.permuted_rows), the fusion head runs on the block (`MultimodalModel.fuse`), and the block's cells are
scored on the device (mmskin.ops.permutation_scores): the logits of the whole (repeat, group, sample) cube never exist at once.

Features are GROUPS of the encoder's columns -- a categorical column (its whole one-hot block) is one group, a numeric column is
one group, the convention of mmskin.shapley -- so a shuffled row is the encoding of a row a patient could have.  The shuffles come
from a counter-based generator of (seed, repeat, group, position) on the device (include/mmskin.h), so a seed reproduces a run bit
for bit.  Metrics, per cell: accuracy, balanced accuracy (mean recall over the classes that occur), macro one-vs-rest AUC of the
soft-max (mean over the classes that have a positive and a negative row, ties at half weight).

    pi = MetadataPermutationImportance(model, enc, n_repeats=10, seed=0)
    res = pi.fit(images, enc.transform(codes, numeric), labels)           # the fold: S <= 4096 samples
    res.importances_mean["balanced_accuracy"]                             # [G], with res.group_names
    res.ranking("auc")                                                    # the groups in descending mean importance

Eval mode, forward only.
"""
import numpy as np
import torch

from . import _metadata_head as mh
from . import ops

METRICS = ops.PERMUTATION_METRICS


class PermutationImportanceResult:
    """What `MetadataPermutationImportance.fit` returns, all on the host.  Dicts keyed by "accuracy", "balanced_accuracy", "auc":
    `importances` float64 [G, R] (baseline - shuffled metric), `importances_mean` and `importances_std` [G] (ddof = 0, as sklearn),
    `metrics` [G, R] (the shuffled metrics themselves) and `baseline` (floats).  `group_names` [G]."""

    def __init__(self, metrics, importances, mean, std, baseline, group_names):
        self.metrics = {m: metrics[k] for k, m in enumerate(METRICS)}
        self.importances = {m: importances[k] for k, m in enumerate(METRICS)}
        self.importances_mean = {m: mean[k] for k, m in enumerate(METRICS)}
        self.importances_std = {m: std[k] for k, m in enumerate(METRICS)}
        self.baseline = {m: float(baseline[k]) for k, m in enumerate(METRICS)}
        self.group_names = list(group_names)

    def ranking(self, metric="balanced_accuracy"):
        """[(group name, mean importance)] in descending mean importance (ties to the lower index)"""
        mean = self.importances_mean[metric]
        return [(self.group_names[g], float(mean[g])) for g in np.argsort(-mean, kind="stable")]


class MetadataPermutationImportance:
    # Rows per fusion-head call (rounded down to a multiple of S, at least S): the head is launch-bound on small blocks (DESIGN.md
    # section 13), and the [rows, F] image-feature tile of a call is 64 MiB at F = 2048
    default_rows_per_call = 8192

    def __init__(self, model, encoder=None, groups=None, n_repeats=10, seed=0, rows_per_call=None, group_names=None, image_batch_size=None):
        """
        model: the loaded MultimodalModel (eval mode, one-hot metadata, a fusion that reads the metadata).
        encoder: the fitted mmskin.preprocess.MetadataEncoder behind the rows, or None.
        groups: the column -> group map, an int sequence over the model's vocab_size encoded columns (-1: never shuffled), or a
            dict {name: [columns]}.  None: with an encoder one group per categorical column (its one-hot block) and one per numeric
            column, columns beyond the encoder's width in no group; without one, one group per column.
        n_repeats: R shuffles per group (sklearn's default is 5, Breiman's figures use 10).  seed: of the device generator.
        rows_per_call: most rows one `model.fuse` call gets, rounded down to a multiple of the fold's size S (at least S).
        group_names: names for `groups` given as a map (default "cat0" .. / "num0" .. with an encoder, "col0" .. otherwise).
        image_batch_size: images per `model.encode_image` call (None: the whole fold at once); each image is encoded once.
        """
        self.model, self.encoder = model, encoder
        self.n_repeats, self.seed = int(n_repeats), int(seed)
        if self.n_repeats < 1:
            raise ValueError(f"MetadataPermutationImportance: n_repeats must be >= 1, got {n_repeats}")
        self.rows_per_call = mh.rows_per_call("MetadataPermutationImportance", "rows_per_call", rows_per_call, self.default_rows_per_call)
        if image_batch_size is not None and int(image_batch_size) < 1:
            raise ValueError(f"MetadataPermutationImportance: image_batch_size must be >= 1, got {image_batch_size}")
        self.image_batch_size = None if image_batch_size is None else int(image_batch_size)
        self.groups, self.group_names = self.resolve_groups(int(getattr(model, "vocab_size", 0) or 0), encoder, groups, group_names)

    @staticmethod
    def resolve_groups(width, encoder, groups, group_names=None):
        """(int32 [width] column -> group map, the G group names) for the constructor's `groups` argument"""
        if width < 1:
            raise ValueError(f"MetadataPermutationImportance: the model's vocab_size is {width}; there is no encoded column")
        names = None
        if groups is None:
            gmap = np.full(width, -1, dtype=np.int32)
            if encoder is not None:
                sizes = [len(c) for c in encoder.categories_] + [1] * len(encoder.mean_)
                names = [f"cat{i}" for i in range(len(encoder.categories_))] + [f"num{i}" for i in range(len(encoder.mean_))]
                if sum(sizes) > width:
                    raise ValueError(f"MetadataPermutationImportance: the encoder's rows have {sum(sizes)} columns, the model's vocab_size is {width}")
                at = 0
                for g, n in enumerate(sizes):
                    gmap[at:at + n] = g
                    at += n
            else:
                gmap[:] = np.arange(width)
                names = [f"col{j}" for j in range(width)]
        elif isinstance(groups, dict):
            gmap = np.full(width, -1, dtype=np.int32)
            names = [str(k) for k in groups]
            for g, cols in enumerate(groups.values()):
                cols = np.asarray(list(cols), dtype=np.int64)
                if cols.size == 0 or cols.min() < 0 or cols.max() >= width or (gmap[cols] >= 0).any():
                    raise ValueError(f"MetadataPermutationImportance: group {names[g]!r} must name columns in 0 .. {width - 1} that no other group holds")
                gmap[cols] = g
        else:
            gmap = np.asarray(groups)
            if gmap.shape != (width,) or not np.issubdtype(gmap.dtype, np.integer):
                raise ValueError(f"MetadataPermutationImportance: groups must map the {width} encoded columns to group indices, got shape {gmap.shape}")
            gmap = gmap.astype(np.int32)
        G = int(gmap.max()) + 1 if gmap.size else 0
        if G < 1 or gmap.min() < -1 or len(np.unique(gmap[gmap >= 0])) != G:
            raise ValueError("MetadataPermutationImportance: the groups must be numbered 0 .. G-1 without a gap (-1: in no group), with G >= 1")
        if group_names is not None:
            names = [str(n) for n in group_names]
        if names is None:
            names = [f"group{g}" for g in range(G)]
        if len(names) != G:
            raise ValueError(f"MetadataPermutationImportance: {G} groups, got {len(names)} names")
        return gmap, names

    def fit(self, images, metadata, labels):
        """The fold: images [S, ...] as the model takes them, metadata fp32 [S, vocab_size] (the ENCODED rows,
        MetadataEncoder.transform), labels integer [S].  Returns a PermutationImportanceResult."""
        model = self.model
        mh.check_metadata_model("MetadataPermutationImportance", model, "explain")
        W, K = int(model.vocab_size), int(model.num_classes)
        x, y = torch.as_tensor(metadata), torch.as_tensor(labels)
        S = int(images.shape[0])
        if tuple(x.shape) != (S, W) or tuple(y.shape) != (S,) or y.dtype.is_floating_point or y.dtype == torch.bool:
            raise ValueError(f"MetadataPermutationImportance.fit: a fold of {S} images needs encoded rows {(S, W)} and integer labels {(S,)}, got "
                             f"{tuple(x.shape)} and {y.dtype} {tuple(y.shape)}")
        if not 1 <= S <= ops.PERMUTATION_MAX_SAMPLES:
            raise ValueError(f"MetadataPermutationImportance.fit: a fold of {S} samples; the kernels hold 1 .. {ops.PERMUTATION_MAX_SAMPLES}")
        R, G = self.n_repeats, len(self.group_names)
        per_call = max(self.rows_per_call // S, 1) * S                            # whole cells: the scores take no split one
        total = R * G * S
        step = self.image_batch_size or S
        with torch.no_grad():
            img_feat = torch.cat([model.encode_image(images[i:i + step]) for i in range(0, S, step)])
            dev = img_feat.device
            x = x.to(device=dev, dtype=torch.float32).contiguous()
            y = y.to(device=dev, dtype=torch.int64).contiguous()
            group = torch.from_numpy(self.groups).to(dev)
            perm = ops.permutation_indices(self.seed, R, G, S, dev)
            # the unshuffled fold is a study of one cell
            base_conf, base_counts = ops.permutation_accumulators(1, 1, K, dev)
            ops.permutation_scores(mh.head_logits(model, img_feat, x, fp32=True), y, base_conf, base_counts, 0)
            baseline = ops.permutation_finalize(base_conf, base_counts, torch.zeros(3, dtype=torch.float64, device=dev))[0][:, 0, 0].contiguous()
            confusion, counts = ops.permutation_accumulators(R, G, K, dev)
            sample = torch.arange(S, device=dev)
            for r0 in range(0, total, per_call):
                r1 = min(r0 + per_call, total)
                metas = ops.permuted_rows(x, group, perm, row0=r0, row1=r1)
                # the image-feature tile of THIS call only: both ends are multiples of S, so the samples simply repeat
                logits = mh.head_logits(model, img_feat.index_select(0, sample.repeat((r1 - r0) // S)), metas, fp32=True)   # the scores take fp32 only
                ops.permutation_scores(logits, y, confusion, counts, r0)
            metrics, importances, mean, std = ops.permutation_finalize(confusion, counts, baseline)
        host = [t.cpu().numpy() for t in (metrics, importances, mean, std, baseline)]
        return PermutationImportanceResult(*host, self.group_names)
