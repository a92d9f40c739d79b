"""Per-sample predictive uncertainty on the GPU: how sure the model is of ONE lesion, and what error rate remains when the
least-sure cases are handed to a dermatologist.

T stochastic passes of a batch come from one of three sources, and one kernel turns them into per-row statistics:

    pu = PredictiveUncertainty(model, device)
    for images, metadata, labels in loader:                      # per-sample results accumulate on the device
        r = pu.mc_dropout(images, metadata, passes=32, seed=0, labels=labels)
        # or: r = pu.tta(images, metadata, views="dihedral", labels=labels)
        # or: r = pu.from_logits(logits_TNC, labels=labels)       # e.g. the K fold models of one split
    rc = pu.risk_coverage(score="mutual_information")            # the whole fold
    pu.save(path)
    pu.reset()

`mc_dropout` encodes the batch's images ONCE (`MultimodalModel.encode_image`: the encoder holds more than 99.8 % of the model's
MACs and no dropout) and runs the fusion head on the T x B rows in a few large calls with the head's dropouts switched on
(`mc_dropout_mode`) and their masks drawn from a stream of their own (`mmskin._autograd.dropout_stream`).  `tta` writes the
dihedral views of the batch with one kernel (mmskin.ops.dihedral_views) and runs the model on them.  The reduction
(mmskin.ops.uncertainty_reduce) gives the mean probability, its spread over the passes, the votes and seven statistics per row,
in fp64; `risk_coverage` ranks the accumulated rows by one of the statistics (mmskin.ops.risk_coverage) and reports the area
under the risk-coverage curve, its optimum, and the AUROC with which the statistic detects the errors.  Eval mode, forward only;
nothing is copied to the host until the caller reads a result.
"""
import contextlib

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._autograd import dropout_stream
from ._lib import MMSkinError
from ._metadata_head import rows_per_call
from .sweep import MetadataSweep

STATS = ops.UNCERTAINTY_STATS
# a statistic that GROWS with certainty is ranked by its negative (exact, and the order of the rows is what counts)
_CERTAINTY = ("confidence", "margin")
VIEW_SETS = {"dihedral": ops.VIEWS_DIHEDRAL, "flips": ops.VIEWS_FLIPS}


@contextlib.contextmanager
def mc_dropout_mode(model):
    """Monte-Carlo dropout on an eval-mode model: inside the block `training` is True on every nn.Dropout instance (HipDropout
    included) outside `model.image_encoder`, and on nothing else -- normalisation layers, stochastic depth and the encoder stay
    in eval mode.  Every flag is restored on exit, also after an exception.  Yields the list of modules it switched.

    The TabTransformer's attention-probability dropout (and that of every nn.MultiheadAttention) is a float that the attention
    module applies under its OWN `training` flag, not an nn.Dropout module: it stays off."""
    encoder = getattr(model, "image_encoder", None)
    inside = {id(m) for m in encoder.modules()} if isinstance(encoder, nn.Module) else set()
    switched = [m for m in model.modules() if isinstance(m, nn.Dropout) and id(m) not in inside]
    before = [m.training for m in switched]
    try:
        for m in switched:
            m.training = True
        yield switched
    finally:
        for m, flag in zip(switched, before):
            m.training = flag


class UncertaintyResult:
    """What one `mc_dropout` / `tta` / `from_logits` call returns, for ITS rows, all on the device: `logits` fp32 [T, B, C];
    `mean_prob`, `prob_std` fp64 [B, C]; `votes` int32 [B, C]; `pred` int32 [B] (-1: a non-finite logit); `stats` fp64 [B, 7] with
    the columns mmskin.uncertainty.STATS (`stat(name)` picks one); `eval_logits` fp32 [B, C] and `pred_eval` int32 [B], the
    deterministic pass (None where the source has none); `n_samples`, the rows accumulated so far."""

    def __init__(self, logits, reduced, eval_logits, pred_eval, n_samples):
        self.logits = logits
        self.mean_prob, self.prob_std, self.votes, self.pred, self.stats = reduced
        self.eval_logits, self.pred_eval, self.n_samples = eval_logits, pred_eval, n_samples

    def stat(self, name):
        return self.stats[:, STATS.index(name)]


class RiskCoverage:
    """The risk-coverage ranking of a fold by one score (larger = less sure).  `counts` int32 [N, 4] and `summary` fp64 [8] stay
    on the device; the named values (`aurc`, `optimal_aurc`, `e_aurc`, `error_auroc`, `error_rate`, `n`, `n_wrong`, `n_distinct`)
    are read from `summary` on first use."""

    def __init__(self, score_name, counts, summary):
        self.score_name, self.counts, self.summary = score_name, counts, summary
        self._host = None

    def __getattr__(self, name):
        if name in ops.RISK_COVERAGE_SUMMARY:
            if self._host is None:
                self._host = self.summary.cpu().numpy()
            v = float(self._host[ops.RISK_COVERAGE_SUMMARY.index(name)])
            return int(v) if name in ("n", "n_wrong", "n_distinct") else v
        raise AttributeError(name)

    def curve(self):
        """(coverage, risk) fp64 [n_distinct] on the device: one point per distinct score, ascending -- the fraction of the fold at
        or below that score, and the error rate among those rows.  Taken from the integer counts; the last point is
        (1, error rate)."""
        c = self.counts.long()
        n_lt, n_eq, e_lt, e_eq = c.unbind(1)
        N = c.shape[0]
        row_of = torch.zeros(N, dtype=torch.int64, device=c.device)
        row_of[n_lt] = torch.arange(N, device=c.device)               # any row of a tie group: they hold the same four integers
        rows = row_of[torch.unique(n_lt)]                              # the groups by ascending score
        kept = (n_lt + n_eq)[rows]
        return kept.double() / N, (e_lt + e_eq)[rows].double() / kept.double()

    def risk_at_coverage(self, coverage):
        """the selective risk at the lowest threshold that keeps at least `coverage` of the fold (0 < coverage <= 1)"""
        if not 0.0 < coverage <= 1.0:
            raise ValueError(f"risk_at_coverage: coverage must lie in (0, 1], got {coverage}")
        cov, risk = (t.cpu().numpy() for t in self.curve())
        return float(risk[min(int(np.searchsorted(cov, coverage, side="left")), len(cov) - 1)])

    def coverage_at_risk(self, risk):
        """the largest coverage of the curve whose selective risk is at most `risk`; 0.0 when no threshold reaches it"""
        cov, r = (t.cpu().numpy() for t in self.curve())
        ok = np.nonzero(r <= risk)[0]
        return float(cov[ok[-1]]) if len(ok) else 0.0


class PredictiveUncertainty:
    # Rows per fusion-head call: MetadataSweep's (the head is launch-bound at these sizes)
    default_rows_per_head_call = MetadataSweep.default_rows_per_head_call
    # Images per model call of `tta`: the 8 views of a batch of 64 in two calls; a bound on activation memory, not a tuned value
    default_images_per_model_call = 256

    def __init__(self, model, device, rows_per_head_call=None, images_per_model_call=None):
        """
        model: the loaded model, in eval mode.  `mc_dropout` needs MultimodalModel's encode_image / fuse split; `tta` takes any
            module called as model(images, metadata); `from_logits` does not touch it (None is allowed).
        device: the model's device.
        rows_per_head_call: most rows (passes x batch) one `model.fuse` call of `mc_dropout` gets; whole passes per call, so a
            batch larger than this runs one pass per call.
        images_per_model_call: most images one model call of `tta` gets.
        """
        self.model, self.device = model, device
        self.rows_per_head_call = rows_per_call("PredictiveUncertainty", "rows_per_head_call", rows_per_head_call, self.default_rows_per_head_call)
        self.images_per_model_call = rows_per_call("PredictiveUncertainty", "images_per_model_call", images_per_model_call,
                                                   self.default_images_per_model_call)
        self.reset()

    def reset(self):
        """Forget the accumulated rows (a new fold)."""
        self._rows = {k: [] for k in ("mean_prob", "prob_std", "votes", "pred", "stats", "labels", "pred_eval")}
        self.n_samples = 0
        self.n_classes = None

    # ---- accumulated per-sample results, device tensors in the order the rows came
    def _cat(self, key):
        parts = self._rows[key]
        return None if not parts else (parts[0] if len(parts) == 1 else torch.cat(parts, dim=0))

    mean_prob = property(lambda self: self._cat("mean_prob"))
    prob_std = property(lambda self: self._cat("prob_std"))
    votes = property(lambda self: self._cat("votes"))
    pred = property(lambda self: self._cat("pred"))
    stats = property(lambda self: self._cat("stats"))
    labels = property(lambda self: self._cat("labels"))
    pred_eval = property(lambda self: self._cat("pred_eval"))

    # ---- checks shared by the sources
    def _labels(self, what, labels, B):
        if labels is None:
            if self._rows["labels"]:
                raise ValueError(f"{what}: the accumulated rows carry labels; call reset() before rows without")
            return None
        if self.n_samples and not self._rows["labels"]:
            raise ValueError(f"{what}: the accumulated rows carry no labels; call reset() before rows with labels")
        labels = torch.as_tensor(labels)
        if tuple(labels.shape) != (B,) or labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise ValueError(f"{what}: labels must be an integer tensor of shape {(B,)}, got {labels.dtype} {tuple(labels.shape)}")
        return labels

    def _eval_model(self, what, needs_split):
        model = self.model
        if needs_split and not (callable(getattr(model, "encode_image", None)) and callable(getattr(model, "fuse", None))):
            raise TypeError(f"{what} needs a model split at encode_image / fuse (MultimodalModel), got {type(model).__name__}")
        if not needs_split and not callable(model):
            raise TypeError(f"{what} needs a module called as model(images, metadata), got {type(model).__name__}")
        if getattr(model, "training", False):
            raise MMSkinError("PredictiveUncertainty runs in eval mode: call model.eval() first")
        return model

    @staticmethod
    def _tile(metadata, times, dev):
        """the metadata of `times` copies of the batch, copy-major (row t * B + b is row b): a tensor, or a mapping of tensors"""
        if hasattr(metadata, "items"):
            return {k: torch.as_tensor(v).to(dev).repeat(times, *([1] * (torch.as_tensor(v).dim() - 1))) for k, v in metadata.items()}
        m = torch.as_tensor(metadata).to(dev)
        return m.repeat(times, *([1] * (m.dim() - 1)))

    @staticmethod
    def _rows_of(metadata, r0, r1):
        return {k: v[r0:r1] for k, v in metadata.items()} if hasattr(metadata, "items") else metadata[r0:r1]

    def _reduce(self, what, logits, labels, eval_logits):
        """logits fp32 [T, B, C] on the device -> the result of this call; its rows join the accumulated ones"""
        T, B, C = logits.shape
        if self.n_classes is not None and C != self.n_classes:
            raise ValueError(f"{what}: the accumulated rows have {self.n_classes} classes, these have {C}; call reset() first")
        reduced = ops.uncertainty_reduce(logits)
        pred_eval = None
        if eval_logits is not None:
            pred_eval = ops.uncertainty_reduce(eval_logits.unsqueeze(0))[3]     # the first arg-max, by the same kernel
        if self._rows["pred_eval"] and pred_eval is None or self.n_samples and not self._rows["pred_eval"] and pred_eval is not None:
            raise ValueError(f"{what}: rows with and without a deterministic pass do not mix; call reset() first")
        for key, t in zip(("mean_prob", "prob_std", "votes", "pred", "stats"), reduced):
            self._rows[key].append(t)
        if labels is not None:
            self._rows["labels"].append(labels.to(device=logits.device, dtype=torch.int64))
        if pred_eval is not None:
            self._rows["pred_eval"].append(pred_eval)
        self.n_samples += B
        self.n_classes = C
        return UncertaintyResult(logits, reduced, eval_logits, pred_eval, self.n_samples)

    # ---- the three sources of the T passes
    def mc_dropout(self, images, metadata, passes=32, seed=0, labels=None):
        """Monte-Carlo dropout of one batch: the images are encoded once, the fusion head runs `passes` times on them (row t * B + b
        of the head calls is pass t of row b) with its dropouts on, and one more time with them off (`eval_logits`, `pred_eval`).
        Equal (seed, passes, batch, rows_per_head_call) repeat the result bit for bit.  The masks are a function of the seed and
        of the position of an element in the sequence of dropout calls, so ANOTHER rows_per_head_call (another number of passes
        per head call) draws other masks: equally valid samples, not the same ones."""
        model = self._eval_model("PredictiveUncertainty.mc_dropout", needs_split=True)
        T = int(passes)
        ops.uncertainty_check_limits("PredictiveUncertainty.mc_dropout", T=T)
        B = int(images.shape[0])
        labels = self._labels("PredictiveUncertainty.mc_dropout", labels, B)
        with torch.no_grad():
            img_feat = model.encode_image(images)
            dev = img_feat.device
            meta = self._tile(metadata, 1, dev)
            eval_logits = model.fuse(img_feat, meta).float().contiguous()
            per_call = max(self.rows_per_head_call // B, 1)                    # whole passes per head call
            feats = img_feat.repeat(min(per_call, T), 1)
            metas = self._tile(metadata, min(per_call, T), dev)
            parts = []
            with mc_dropout_mode(model), dropout_stream(seed):
                for t0 in range(0, T, per_call):
                    rows = min(per_call, T - t0) * B
                    parts.append(model.fuse(feats[:rows], self._rows_of(metas, 0, rows)).float())
            logits = (parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)).reshape(T, B, -1).contiguous()
            return self._reduce("PredictiveUncertainty.mc_dropout", logits, labels, eval_logits)

    def tta(self, images, metadata, views="dihedral", labels=None):
        """Test-time augmentation of one batch: `views` is "dihedral" (all 8 views: square images), "flips" (views 0, 2, 4, 6:
        identity, half turn, mirror, flip; any shape) or a list of view ids (mmskin.h: v = quarter turns + 4 for the mirror).  One
        kernel writes the views, the model runs on them in chunks of images_per_model_call images with the metadata rows tiled;
        pass t of the result is the t-th selected view in ascending id.  `eval_logits` is the identity view when it is selected."""
        model = self._eval_model("PredictiveUncertainty.tta", needs_split=False)
        if isinstance(views, str):
            if views not in VIEW_SETS:
                raise ValueError(f"PredictiveUncertainty.tta: views must be one of {sorted(VIEW_SETS)} or a list of view ids, got {views!r}")
            mask = VIEW_SETS[views]
        else:
            ids = [int(v) for v in views]
            if not ids or any(not 0 <= v < 8 for v in ids) or len(set(ids)) != len(ids):
                raise ValueError(f"PredictiveUncertainty.tta: view ids must be distinct values of 0 .. 7, got {list(views)}")
            mask = sum(1 << v for v in ids)
        B = int(images.shape[0])
        labels = self._labels("PredictiveUncertainty.tta", labels, B)
        with torch.no_grad():
            images = torch.as_tensor(images).to(self.device).contiguous()
            stack = ops.dihedral_views(images, mask)                            # refuses a quarter turn of a non-square batch
            V = stack.shape[0]
            stack = stack.reshape(V * B, *images.shape[1:])
            metas = self._tile(metadata, V, images.device)
            step = self.images_per_model_call
            parts = [model(stack[r0:r0 + step], self._rows_of(metas, r0, r0 + step)).float() for r0 in range(0, V * B, step)]
            logits = (parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)).reshape(V, B, -1).contiguous()
            eval_logits = logits[0].contiguous() if mask & 1 else None
            return self._reduce("PredictiveUncertainty.tta", logits, labels, eval_logits)

    def from_logits(self, logits, labels=None):
        """T passes from any source: logits fp32 [T, N, C] on the device (e.g. the K fold models of one split, stacked)."""
        if not torch.is_tensor(logits) or logits.dim() != 3 or logits.dtype != torch.float32:
            raise ValueError("PredictiveUncertainty.from_logits: logits must be an fp32 [T, N, C] device tensor, got "
                             f"{getattr(logits, 'dtype', type(logits).__name__)} {tuple(getattr(logits, 'shape', ()))}")
        labels = self._labels("PredictiveUncertainty.from_logits", labels, int(logits.shape[1]))
        with torch.no_grad():
            return self._reduce("PredictiveUncertainty.from_logits", logits.detach(), labels, None)

    # ---- the fold
    def score(self, name):
        """fp64 [n_samples] on the device: the accumulated statistic `name`, oriented so that larger = less sure"""
        if name not in STATS:
            raise ValueError(f"PredictiveUncertainty: score must be one of {STATS}, got {name!r}")
        if not self.n_samples:
            raise ValueError("PredictiveUncertainty: no rows have been accumulated")
        col = self.stats[:, STATS.index(name)]
        return (-col if name in _CERTAINTY else col).contiguous()

    def risk_coverage(self, score="mutual_information"):
        """Rank the accumulated rows by `score` (one of mmskin.uncertainty.STATS; confidence and margin by their negative) and
        return the RiskCoverage of the fold: an error is pred != label.  Needs labels on every accumulated row; a NaN score (a row
        with a non-finite logit) is refused."""
        s = self.score(score)
        if not self._rows["labels"]:
            raise ValueError("PredictiveUncertainty.risk_coverage needs labels: pass labels= with every batch")
        ops.risk_coverage_check_limits("PredictiveUncertainty.risk_coverage", self.n_samples)
        if bool(torch.isnan(s).any()):
            raise ValueError(f"PredictiveUncertainty.risk_coverage: the score {score!r} holds NaN (a row with a non-finite logit)")
        wrong = (self.pred.long() != self.labels).to(torch.uint8).contiguous()
        counts = ops.risk_coverage(s, wrong)
        return RiskCoverage(score, counts, ops.risk_coverage_summary(counts, wrong))

    def save(self, path):
        """Write the accumulated per-sample results to `path` (numpy .npz): mean_prob, prob_std, votes, pred, stats, stat_names, and
        labels / pred_eval where they were given."""
        if not self.n_samples:
            raise ValueError("PredictiveUncertainty.save: no rows have been accumulated")
        out = {k: getattr(self, k).cpu().numpy() for k in ("mean_prob", "prob_std", "votes", "pred", "stats")}
        for k in ("labels", "pred_eval"):
            if self._rows[k]:
                out[k] = getattr(self, k).cpu().numpy()
        np.savez(path, stat_names=np.array(STATS), **out)
