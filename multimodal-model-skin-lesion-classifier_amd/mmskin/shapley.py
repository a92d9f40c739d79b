"""Shapley values of the metadata on the model itself, batched on the GPU.

The reference explains the metadata contribution to prob_NEV ... prob_MEL on a SURROGATE
(src/scripts/data_preprocessing/shap_values.py; lime_padufes20.py does the same with LIME, see mmskin.lime for that half): a
300-tree RandomForestRegressor fitted on (encoded
metadata -> recorded probabilities), explained with shap's permutation explainer, because ~10^5 batch-1 forwards of the real
model per explained sample are out of reach.  The surrogate explains the forest, not the network, sees no image, and treats
each one-hot CELL as a feature, so most of its coalitions are rows no patient could have.  Here the network itself is explained:
a batch's images are encoded ONCE (`MultimodalModel.encode_image`), one HIP kernel writes the coalition rows of a block
(mmskin.ops.shapley_coalitions), the fusion head runs on the block (`MultimodalModel.fuse`), and the logits are reduced to
Shapley values on the device (mmskin.ops.shapley_reduce).

The estimator.  Players are the encoder's M = n_cat + n_num COLUMNS, categorical first: a categorical column (its whole one-hot
block) is one player, a numeric column is one player -- the deliberate difference from the reference's script.  For an explained
row x with image features f, G background metadata rows b_g and a coalition S

    v(S) = (1/G) sum_g out(fuse(f, mix(x, b_g, S)))         mix takes column j from x if j is in S, else from b_g

with out = the soft-max probabilities (output="prob", what the reference explains) or the raw logits ("logit").  P permutations
pi_p are each walked from both ends (antithetic sampling, shap's permutation explainer): S_k = the first k entries of pi_p,
T_k = its last k, and for the player j at position q of pi_p

    phi_j = (1/2P) sum_p [ v(S_{q+1}) - v(S_q) + v(T_{M-q}) - v(T_{M-q-1}) ]

v(all) = out(fuse(f, x)) is one row and v(empty) G rows; both are shared by all permutations, so a sample's walk has
1 + G + P 2 (M - 1) G rows.  sum_j phi_j = v(all) - v(empty) for every P (efficiency), and the estimator is exact at P = 1 for
a value function with at most pairwise interactions.  The permutations are drawn on the host from `seed`
(rng = np.random.default_rng(seed); rng.permutation(M) per p), so a seed reproduces a run bit for bit.

    sh = MetadataShapley(model, enc, device, background_codes, background_numeric)          # G = 100 rows of the training set
    for images, cat_rows, numeric in loader:                         # mean_abs accumulates over the batches
        res = sh.explain(images, enc.codes(cat_rows), numeric)
    res.values                                                       # [B, M, C] of the last batch
    importance, order = sh.global_importance()                       # the script's "Top 10": order[:10]

Eval mode, forward only.
"""
import numpy as np
import torch

from . import _metadata_head as mh
from . import ops

OUTPUTS = {"prob": ops.SHAPLEY_PROB, "logit": ops.SHAPLEY_LOGIT}


class ShapleyResult(mh.AbsSum):
    """What `MetadataShapley.explain` returns.  Per row of THIS batch: `values` fp32 [B, M, C], `base` [B, C] = v(empty) (it
    depends on the image) and `full` [B, C] = v(all).  Accumulated since the last reset: `abs_sum` fp64 [M, C], `n_samples`, and
    `mean_abs` = abs_sum / n_samples (the script's features x classes heat map).  Everything but `n_samples` is a device tensor."""

    def __init__(self, values, base, full, abs_sum, n_samples):
        self.values, self.base, self.full, self.abs_sum, self.n_samples = values, base, full, abs_sum, n_samples


class MetadataShapley(mh.AbsSum):
    # Rows per fusion-head call (rounded down to a multiple of G): the head is launch-bound on small blocks (DESIGN.md section
    # 13), and the [rows, F] image-feature tile of a call is 64 MiB at F = 2048
    default_rows_per_head_call = 8192

    def __init__(self, model, encoder, device, background_codes, background_numeric, n_permutations=10, seed=0, output="prob",
                 rows_per_head_call=None, out_width=None):
        """
        model: the loaded MultimodalModel (eval mode, one-hot metadata, a fusion that reads the metadata).
        encoder: the fitted mmskin.preprocess.MetadataEncoder.
        device: the model's device.
        background_codes int32 [G, n_cat] (MetadataEncoder.codes), background_numeric [G, n_num] (NaN = missing): the rows that
            stand in for the columns outside a coalition.
        n_permutations: P, walked from both ends (shap's default 10).  seed: of the host draw of the permutations.
        output: "prob" or "logit".
        rows_per_head_call: most rows one `model.fuse` call gets, rounded down to a multiple of G (at least G).
        out_width: width of the encoded metadata rows, padded with zeros or cut; must equal model.vocab_size (the default).
        """
        self.model, self.encoder, self.device = model, encoder, device
        n_cat, n_num = len(encoder.categories_), len(encoder.mean_)
        self.n_players = n_cat + n_num
        if self.n_players < 1:
            raise ValueError("MetadataShapley: the encoder has no column")
        bg_codes, bg_numeric = torch.as_tensor(background_codes), torch.as_tensor(background_numeric)
        G = int(bg_codes.shape[0]) if bg_codes.dim() == 2 else -1
        if G < 1 or tuple(bg_codes.shape) != (G, n_cat) or tuple(bg_numeric.shape) != (G, n_num):
            raise ValueError(f"MetadataShapley: the background must be G >= 1 rows of codes [G, {n_cat}] and numeric [G, {n_num}], got "
                             f"{tuple(bg_codes.shape)} and {tuple(bg_numeric.shape)}")
        self.n_background = G
        self.background_codes = bg_codes.to(torch.int32).contiguous()
        self.background_numeric = bg_numeric.to(torch.float32).contiguous()
        if int(n_permutations) < 1:
            raise ValueError(f"MetadataShapley: n_permutations must be >= 1, got {n_permutations}")
        if output not in OUTPUTS:
            raise ValueError(f"MetadataShapley: output must be 'prob' or 'logit', got {output!r}")
        self.output = output
        self.permutations = self.draw_permutations(self.n_players, int(n_permutations), seed)
        rows = mh.rows_per_call("MetadataShapley", "rows_per_head_call", rows_per_head_call, self.default_rows_per_head_call)
        self.rows_per_head_call = max(rows // G, 1) * G                       # whole coalitions: the reduce takes no split one
        self.out_width = int(out_width) if out_width is not None else int(getattr(model, "vocab_size", encoder.width))
        self.reset()

    @staticmethod
    def draw_permutations(n_players, n_permutations, seed):
        """int32 [P, M]: rng = np.random.default_rng(seed), then rng.permutation(M) per p."""
        rng = np.random.default_rng(seed)
        return np.stack([rng.permutation(n_players) for _ in range(n_permutations)]).astype(np.int32)

    def rows_per_sample(self):
        """1 + G + P 2 (M - 1) G: v(all), v(empty) and the interior coalitions of the P antithetic walks."""
        G, P, M = self.n_background, len(self.permutations), self.n_players
        return 1 + G + P * 2 * (M - 1) * G

    def column_names(self, categorical_columns, numeric_columns):
        """The players' names in the order of `values`' second axis: the categorical columns, then the numeric ones."""
        cats, nums = mh.check_columns("column_names", self.encoder, categorical_columns, numeric_columns)
        return cats + nums

    # ---- per batch
    def explain(self, images, codes, numeric):
        """One batch: images [B, ...] as the model takes them, codes int32 [B, n_cat] (MetadataEncoder.codes), numeric [B, n_num]
        (NaN = missing).  Adds the batch's |values| to the running sums and returns a ShapleyResult."""
        model, enc = self.model, self.encoder
        mh.check_metadata_model("MetadataShapley", model, "explain")
        if self.out_width != model.vocab_size:
            raise ValueError(f"MetadataShapley: out_width {self.out_width} is not the model's vocab_size {model.vocab_size}")
        B = int(images.shape[0])
        codes, numeric = mh.batch_codes("MetadataShapley.explain", B, enc, codes, numeric)
        C, G, M, perms = int(model.num_classes), self.n_background, self.n_players, self.permutations
        if self.abs_sum is not None and tuple(self.abs_sum.shape) != (M, C):
            raise ValueError(f"MetadataShapley.explain: the sums hold {tuple(self.abs_sum.shape)} players x classes; call reset() first")
        K = 2 * len(perms) * (M - 1)
        coalition_rows, total = B * (K + 1) * G, B * self.rows_per_sample()

        with torch.no_grad():
            img_feat = model.encode_image(images)
            dev = img_feat.device
            _, mean, scale = enc._tables(dev)
            codes = codes.to(device=dev, dtype=torch.int32).contiguous()
            numeric = numeric.to(device=dev, dtype=torch.float32).contiguous()
            bg_codes, bg_numeric = self.background_codes.to(dev), self.background_numeric.to(dev)
            off_host = enc.col_offsets()
            if self.abs_sum is None:
                self.abs_sum = torch.zeros((M, C), dtype=torch.float64, device=dev)
            v = torch.empty((B, K + 2, C), dtype=torch.float64, device=dev)
            out = None
            for r0 in range(0, total, self.rows_per_head_call):
                r1 = min(r0 + self.rows_per_head_call, total)
                metas = ops.shapley_coalitions(codes, numeric, bg_codes, bg_numeric, off_host, mean, scale, enc.nan_fill, perms,
                                               self.out_width, row0=r0, row1=r1)
                # the image-feature tile of THIS call only: row -> its sample, in the walk's row order
                rows = torch.arange(r0, r1, device=dev)
                sample = torch.where(rows < coalition_rows, torch.div(rows, (K + 1) * G, rounding_mode="floor"), rows - coalition_rows)
                logits = mh.head_logits(model, img_feat.index_select(0, sample), metas)
                out = ops.shapley_reduce(logits, v, perms, G, r0, output=OUTPUTS[self.output], finish=r1 == total,
                                         abs_sum=self.abs_sum)
        values, base, full = out
        self.n_samples += B
        return ShapleyResult(values, base, full, self.abs_sum, self.n_samples)
