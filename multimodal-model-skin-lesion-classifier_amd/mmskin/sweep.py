"""Metadata-sensitivity sweeps, batched on the GPU: the reference's flip-rate analysis (interpretability/flip_rate.py:164-256),
its missing-metadata degradation (inference_all_folds.py:116-140, 216-246) and its prediction-uncertainty table
(analyze_prediction_uncertainty.py:166-272).

The reference runs `model(img, meta)` at batch 1 once per image and metadata variant: the image encoder -- more than 99.8 % of
the model's MACs -- is re-run for every variant of an image that has not changed, every row is re-encoded through pandas and
sklearn, and every probability vector is copied to the host.  Here a batch's images are encoded ONCE
(`MultimodalModel.encode_image`), one HIP kernel writes all V mutated, encoded metadata batches from the integer codes
(mmskin.ops.metadata_variants), the fusion head runs on the V x B rows in a few large calls (`MultimodalModel.fuse`), and one
kernel turns the logits into predictions, flip / transition / confusion counts and the uncertainty measures on the device
(mmskin.ops.sweep_reduce).  Nothing is copied to the host until the caller reads a result.

    enc = MetadataEncoder.from_sklearn(ohe, scaler)
    sw = MetadataSweep(model, enc, device)
    variants = sw.flip_variants({"itch": ("toggle", "True", "False"), "age": ("set", 80.0), "diameter_1": ("add", 5.0)},
                                categorical_columns=[...], numeric_columns=[...])
    for images, cat_rows, numeric, labels in loader:                    # counters accumulate over the batches
        res = sw.run(images, enc.codes(cat_rows), numeric, variants, labels=labels)
    res.flip_rate, res.transitions, res.confusion                       # device tensors; variant 0 is the baseline

Variant 0 of every table is the unmutated baseline (`flip_variants` and `missing_variants` put it there): the other variants
are compared with it.  Eval mode, forward only.
"""
import numpy as np
import torch

from . import _metadata_head as mh
from . import ops


class SweepResult:
    """What `MetadataSweep.run` returns.  Per (variant, row) of the LAST batch: `logits`, `probs` [V, B, C], `pred` int32 and
    `margin` [V, B], `stats` [V, B, 4] = entropy (nats), KL(variant || baseline), JS, p_v[base_pred] - p_base[base_pred].
    Accumulated over every batch since the sweep's last reset: `flips` int32 [V], `transitions` int32 [V, C, C] indexed
    [baseline prediction][prediction], `confusion` int32 [V, C, C] indexed [label][prediction] (None without labels),
    `n_samples`, and `flip_rate` = flips / n_samples.  Everything but `n_samples` is a device tensor."""

    def __init__(self, logits, probs, pred, margin, stats, flips, transitions, confusion, n_samples):
        self.logits, self.probs, self.pred, self.margin, self.stats = logits, probs, pred, margin, stats
        self.flips, self.transitions, self.confusion, self.n_samples = flips, transitions, confusion, n_samples

    @property
    def flip_rate(self):
        return self.flips.double() / max(self.n_samples, 1)


class MetadataSweep:
    # Rows per fusion-head call: the fastest of 256 / 1088 / 4096 on densenet169 + gfcam at batch 64 (scripts/sweep_bench.py,
    # DESIGN.md section 13): the head is launch-bound at these sizes, so fewer, larger calls win, and the whole block of the
    # reference's flip-rate sweep (17 x 64 = 1088 rows) fits one call
    default_rows_per_head_call = 4096

    def __init__(self, model, encoder, device, rows_per_head_call=None, out_width=None):
        """
        model: the loaded MultimodalModel (eval mode, one-hot metadata, a fusion that reads the metadata).
        encoder: the fitted mmskin.preprocess.MetadataEncoder.
        device: the model's device.
        rows_per_head_call: most rows (variants x batch) one `model.fuse` call gets.
        out_width: width of the encoded metadata rows, padded with zeros or cut; must equal model.vocab_size (the default).
        """
        self.model, self.encoder, self.device = model, encoder, device
        self.rows_per_head_call = mh.rows_per_call("MetadataSweep", "rows_per_head_call", rows_per_head_call, self.default_rows_per_head_call)
        self.out_width = int(out_width) if out_width is not None else int(getattr(model, "vocab_size", encoder.width))
        self.reset()

    def reset(self):
        """Forget the accumulated counters (a new sweep)."""
        self.flips = self.transitions = self.confusion = None
        self.n_samples = 0

    # ---- host: names / strings -> records
    def _code(self, column, value):
        cats = [str(c) for c in self.encoder.categories_[column]]
        return cats.index(str(value)) if str(value) in cats else -1          # unseen at fit time: an all-zero block

    def flip_variants(self, spec, categorical_columns, numeric_columns):
        """The variant table of a flip-rate sweep: the baseline first, then one record per entry of `spec`, a mapping (or a
        list of pairs, to mutate a column more than once) column name -> ("toggle", a, b) | ("set", value) | ("add", value).
        `categorical_columns` / `numeric_columns` name the encoder's columns in its order; categorical values are given as
        the strings the encoder was fitted on (a string it has not seen encodes as an all-zero block)."""
        cats, nums = mh.check_columns("flip_variants", self.encoder, categorical_columns, numeric_columns)
        items = list(spec.items()) if hasattr(spec, "items") else list(spec)
        table = np.zeros(1 + len(items), dtype=ops.META_VARIANT_DTYPE)
        for i, (name, rule) in enumerate(items, start=1):
            kind, args = rule[0], tuple(rule[1:])
            if name in cats:
                col = cats.index(name)
                if kind == "toggle" and len(args) == 2:
                    table[i] = (ops.META_CAT_TOGGLE, col, self._code(col, args[0]), self._code(col, args[1]), 0.0, (0, 0, 0))
                elif kind == "set" and len(args) == 1:
                    table[i] = (ops.META_CAT_SET, col, self._code(col, args[0]), 0, 0.0, (0, 0, 0))
                else:
                    raise ValueError(f"flip_variants: {name!r} is categorical: ('toggle', a, b) or ('set', value), got {rule!r}")
            elif name in nums:
                if kind not in ("add", "set") or len(args) != 1:
                    raise ValueError(f"flip_variants: {name!r} is numeric: ('add', value) or ('set', value), got {rule!r}")
                table[i] = (ops.META_NUM_ADD if kind == "add" else ops.META_NUM_SET, len(cats) + nums.index(name), 0, 0, float(args[0]),
                            (0, 0, 0))
            else:
                raise ValueError(f"flip_variants: {name!r} is not a column of the encoder")
        return table

    def missing_variants(self, rates, n_rows, numeric_columns, categorical_columns, seeds):
        """The table and mask of a missing-metadata sweep: the baseline (nothing blanked) first, then one variant per rate.
        The cells to blank are drawn exactly as simulate_missing_metadata draws them (inference_all_folds.py:118-129):
        keep = np.random.default_rng(seed).random((n_rows, n_features)) < (1 - rate) with the features ordered numeric first,
        then categorical; `seeds` holds one seed per rate (the reference's rule, fold + int(rate * 1000), stays with the
        caller).  Returns (table, mask uint8 [1 + len(rates), n_rows, n_cat + n_num]) in the kernel's [categorical | numeric]
        column order; hand `run` the rows mask[:, r0:r1] of its batch."""
        rates, seeds = list(rates), list(seeds) if np.ndim(seeds) else [seeds] * len(list(rates))
        if len(seeds) != len(rates):
            raise ValueError(f"missing_variants: {len(rates)} rates but {len(seeds)} seeds")
        n_cat, n_num = map(len, mh.check_columns("missing_variants", self.encoder, categorical_columns, numeric_columns))
        mask = np.zeros((1 + len(rates), int(n_rows), n_cat + n_num), dtype=np.uint8)
        for i, (rate, seed) in enumerate(zip(rates, seeds), start=1):
            keep = np.random.default_rng(seed).random((int(n_rows), n_num + n_cat)) < (1 - rate)
            mask[i, :, :n_cat] = ~keep[:, n_num:]
            mask[i, :, n_cat:] = ~keep[:, :n_num]
        return np.zeros(1 + len(rates), dtype=ops.META_VARIANT_DTYPE), mask

    def _missing_codes(self):
        return np.array([self._code(j, "EMPTY") for j in range(len(self.encoder.categories_))], dtype=np.int32)

    # ---- per batch
    def run(self, images, codes, numeric, variants, mask=None, labels=None):
        """One batch: images [B, ...] as the model takes them, codes int32 [B, n_cat] (MetadataEncoder.codes), numeric
        [B, n_num] (NaN = missing), variants from flip_variants / missing_variants (variant 0 = baseline), mask uint8
        [V, B, n_cat + n_num] or None, labels [B] or None.  Adds this batch to the sweep's counters and returns a SweepResult."""
        model, enc = self.model, self.encoder
        mh.check_metadata_model("MetadataSweep", model, "sweep")
        if self.out_width != model.vocab_size:
            raise ValueError(f"MetadataSweep: out_width {self.out_width} is not the model's vocab_size {model.vocab_size}")
        table = np.ascontiguousarray(variants)
        if table.dtype != ops.META_VARIANT_DTYPE or table.ndim != 1 or len(table) < 1:
            raise ValueError("MetadataSweep.run: variants must be a table from flip_variants or missing_variants")
        if int(table["op"][0]) != ops.META_NONE:
            raise ValueError("MetadataSweep.run: variant 0 must be the baseline (op NONE)")
        V, n_cat, n_num = len(table), len(enc.categories_), len(enc.mean_)
        B = int(images.shape[0])
        codes, numeric = mh.batch_codes("MetadataSweep.run", B, enc, codes, numeric)
        if mask is not None:
            mask = torch.as_tensor(mask)
            if tuple(mask.shape) != (V, B, n_cat + n_num):
                raise ValueError(f"MetadataSweep.run: mask must have shape {(V, B, n_cat + n_num)}, got {tuple(mask.shape)}")
        if labels is not None:
            labels = torch.as_tensor(labels)
            if tuple(labels.shape) != (B,):
                raise ValueError(f"MetadataSweep.run: labels must have shape {(B,)}, got {tuple(labels.shape)}")
        C = int(model.num_classes)
        if self.flips is not None and (tuple(self.transitions.shape) != (V, C, C) or (labels is not None) != (self.confusion is not None)):
            raise ValueError(f"MetadataSweep.run: the sweep has accumulated {self.flips.shape[0]} variants "
                             f"{'with' if self.confusion is not None else 'without'} labels; call reset() before a different sweep")

        with torch.no_grad():
            img_feat = model.encode_image(images)
            dev = img_feat.device
            _, mean, scale = enc._tables(dev)
            codes = codes.to(device=dev, dtype=torch.int32).contiguous()
            numeric = numeric.to(device=dev, dtype=torch.float32).contiguous()
            if mask is not None:
                mask = mask.to(device=dev, dtype=torch.uint8).contiguous()
            missing = torch.from_numpy(self._missing_codes()).to(dev) if mask is not None and n_cat else None
            metas = ops.metadata_variants(codes, numeric, enc.col_offsets(), mean, scale, enc.nan_fill, table, self.out_width, mask=mask,
                                          missing_code=missing)
            feats = img_feat.unsqueeze(0).expand(V, *img_feat.shape).contiguous().reshape(V * B, -1)
            metas = metas.reshape(V * B, self.out_width)
            step = self.rows_per_head_call
            parts = [mh.head_logits(model, feats[r0:r0 + step], metas[r0:r0 + step]) for r0 in range(0, V * B, step)]
            logits = (parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)).reshape(V, B, C)
            if self.flips is None:
                self.flips = torch.zeros(V, dtype=torch.int32, device=dev)
                self.transitions = torch.zeros((V, C, C), dtype=torch.int32, device=dev)
                self.confusion = torch.zeros((V, C, C), dtype=torch.int32, device=dev) if labels is not None else None
            if labels is not None:
                labels = labels.to(device=dev, dtype=torch.int32).contiguous()
            probs, pred, margin, stats = ops.sweep_reduce(logits, logits[0].float().contiguous(), self.flips, self.transitions,
                                                          confusion=self.confusion, labels=labels)
        self.n_samples += B
        return SweepResult(logits, probs, pred, margin, stats, self.flips, self.transitions, self.confusion, self.n_samples)
