"""Bootstrap confidence intervals for the metrics of a validation fold, and a paired comparison of two models on it, on the GPU.

`mmskin.evaluate.evaluate_model` returns point estimates on a fold of a few hundred to a few thousand lesions; the reference
states uncertainty only across its five folds (src/scripts/aggreation/).  The non-parametric bootstrap resamples the fold's rows
with replacement B times and scores every resample; the spread of those B values is the metric's sampling uncertainty.  Here a
resample is a vector of integer weights w_b (how often each row was drawn) that one workgroup builds in LDS from a counter-based
generator of (seed, replicate, draw) and turns into the replicate's exact integers: the weighted confusion matrix and the weighted
Mann-Whitney counts of the one-vs-rest AUC (csrc/bootstrap.hip; the definitions are in include/mmskin.h and DESIGN.md section 23).
The metrics follow `criterion.metrics_from_confusion`, `evaluate.auc_from_counts` and `evaluate.per_class_auc`, in fp64.

    bs = BootstrapMetrics(n_resamples=2000, seed=0, confidence=0.95)
    res = bs.evaluate(probs, labels)                       # what evaluate_model returned, or bs.from_fold_dir(folder)
    res.point["balanced_accuracy"], res.interval("balanced_accuracy")
    res.low["per_class_recall"], res.high["per_class_recall"]             # [K]: sensitivity per class
    cmp = bs.compare(probs_a, probs_b, labels)             # the same resamples for both: a paired test
    cmp.point["auc"], cmp.low["auc"], cmp.high["auc"], cmp.p_value["auc"]

The weights depend on (seed, replicate, N) -- stratified: and on the labels -- never on the scores, so two score tables on one
fold see the same resamples and their per-replicate difference is a paired difference.  Rows whose label lies outside [0, K)
are dropped first, as in EpochMeter.  A metric that is undefined in a replicate (a class that drew no row) is NaN there and
leaves the summary's `n_valid`; stratified resampling keeps every class's count and has no such replicates.  The row index of a
draw is the multiply-high (u N) >> 32 of a 32-bit u: its bias is below N / 2^32.  GPU only.
"""
import os

import numpy as np
import torch

from . import ops
from ._lib import MMSkinError

METRICS = ops.BOOTSTRAP_METRICS
CLASS_METRICS = ops.BOOTSTRAP_CLASS_METRICS


def _by_metric(table, K):
    """a [7 + 2 K, ...] array -> {name: [...] for the scalar metrics, name: [K, ...] moved to [..., K] for the per-class ones}"""
    out = {m: table[k] for k, m in enumerate(METRICS)}
    for j, m in enumerate(CLASS_METRICS):
        out[m] = np.moveaxis(table[7 + j * K:7 + (j + 1) * K], 0, -1)
    return out


def _scalars(d):
    return {m: (float(v) if np.ndim(v) == 0 else np.ascontiguousarray(v)) for m, v in d.items()}


class BootstrapResult:
    """What `BootstrapMetrics.evaluate` returns, all on the host.  Dicts keyed by the names of ops.BOOTSTRAP_METRICS (floats) and
    ops.BOOTSTRAP_CLASS_METRICS (float64 [K]): `point` (the fold itself), `mean`, `std` (ddof = 1), `low`, `high` (the percentile
    interval at `confidence`) and `n_valid` (the replicates in which the metric is defined).  `replicates`: float64 [B] per metric,
    [B, K] for the per-class ones.  With return_counts=True also `confusion` int32 [B, K, K], `counts` dict(pos, neg, wins2: int64
    [B, K]) and their `point_confusion` [K, K] / `point_counts`."""

    def __init__(self, point, replicates, summary, K, confidence, integers=None):
        self.num_classes, self.confidence = K, confidence
        self.point = _scalars(_by_metric(point[:, 0], K))
        self.replicates = {m: np.ascontiguousarray(v) for m, v in _by_metric(replicates, K).items()}
        rows = {name: _scalars(_by_metric(summary[k], K)) for k, name in enumerate(ops.BOOTSTRAP_SUMMARY)}
        self.mean, self.std, self.low, self.high = rows["mean"], rows["std"], rows["low"], rows["high"]
        self.n_valid = {m: (int(v) if np.ndim(v) == 0 else v.astype(np.int64)) for m, v in rows["n_valid"].items()}
        if integers is not None:
            self.point_confusion, self.point_counts, self.confusion, self.counts = integers

    def interval(self, metric):
        """(low, high) of the percentile interval: floats, or [K] arrays for a per-class metric"""
        return self.low[metric], self.high[metric]


class BootstrapComparison:
    """What `BootstrapMetrics.compare` returns: per metric, `point` = metric(A) - metric(B) on the fold, `low` / `high` = the
    percentile interval of the per-replicate differences, `mean`, `std`, `n_valid` (the replicates in which both are defined),
    `p_value` = min(1, 2 min((#{d <= 0} + 1) / (n + 1), (#{d >= 0} + 1) / (n + 1))) over those n replicates, and `replicates`
    (the differences).  `a` and `b` are the two BootstrapResults."""

    def __init__(self, a, b, point, delta, summary, sign_counts, K):
        self.a, self.b, self.num_classes = a, b, K
        self.point = _scalars(_by_metric(point[:, 0], K))
        self.replicates = {m: np.ascontiguousarray(v) for m, v in _by_metric(delta, K).items()}
        rows = {name: _scalars(_by_metric(summary[k], K)) for k, name in enumerate(ops.BOOTSTRAP_SUMMARY)}
        self.mean, self.std, self.low, self.high = rows["mean"], rows["std"], rows["low"], rows["high"]
        self.n_valid = {m: (int(v) if np.ndim(v) == 0 else v.astype(np.int64)) for m, v in rows["n_valid"].items()}
        n = summary[0]
        p = np.minimum(1.0, 2.0 * np.minimum((sign_counts[:, 0] + 1) / (n + 1), (sign_counts[:, 1] + 1) / (n + 1)))
        self.p_value = _scalars(_by_metric(p, K))


class BootstrapMetrics:
    def __init__(self, n_resamples=2000, seed=0, confidence=0.95, stratified=False, replicates_per_call=None):
        """
        n_resamples: B replicates, 1 .. ops.BOOTSTRAP_MAX_RESAMPLES.  seed: of the device generator.
        confidence: of the percentile interval, in (0, 1).
        stratified: resample within each class, so that every replicate keeps the fold's class counts.
        replicates_per_call: replicates per kernel launch (None: all at once); it cuts the study and changes no result.
        """
        self.n_resamples, self.seed, self.stratified = int(n_resamples), int(seed), bool(stratified)
        ops.bootstrap_check_limits("BootstrapMetrics", B=self.n_resamples)
        self.confidence = float(confidence)
        if not 0.0 < self.confidence < 1.0:
            raise ValueError(f"BootstrapMetrics: confidence must lie in (0, 1), got {confidence}")
        if replicates_per_call is not None and int(replicates_per_call) < 1:
            raise ValueError(f"BootstrapMetrics: replicates_per_call must be >= 1, got {replicates_per_call}")
        self.replicates_per_call = None if replicates_per_call is None else int(replicates_per_call)

    # ------------------------------------------------------------------------------------------ arguments
    @staticmethod
    def _integer_rows(name, v, N):
        t = torch.as_tensor(v)
        if tuple(t.shape) != (N,) or t.dtype.is_floating_point or t.dtype == torch.bool or t.dtype.is_complex:
            raise ValueError(f"BootstrapMetrics: {name} must be an integer {(N,)} array, got {t.dtype} {tuple(t.shape)}")
        return t

    def _fold(self, what, scores, labels, preds):
        """the checked arguments as host-or-device tensors with the rows outside [0, K) dropped: (scores fp32 [N, K], labels,
        preds or None).  Everything here is an argument error (ValueError) or a limit (MMSkinError) and needs no device."""
        s = torch.as_tensor(scores)
        if s.dim() != 2 or s.dtype != torch.float32:
            raise ValueError(f"BootstrapMetrics.{what}: scores must be an fp32 [N, K] array, got {s.dtype} {tuple(s.shape)}")
        rows, K = s.shape
        y = self._integer_rows("labels", labels, rows)
        p = None if preds is None else self._integer_rows("preds", preds, rows)
        ops.bootstrap_check_limits(f"BootstrapMetrics.{what}", K=K)
        if y.device != s.device or (p is not None and p.device != s.device):
            raise ValueError(f"BootstrapMetrics.{what}: scores, labels and preds must live on one device")
        keep = (y >= 0) & (y < K)
        if not bool(keep.all()):
            s, y, p = s[keep], y[keep], (None if p is None else p[keep])
        ops.bootstrap_check_limits(f"BootstrapMetrics.{what}", N=int(s.shape[0]))
        if bool(torch.isnan(s).any()):
            raise ValueError(f"BootstrapMetrics.{what}: the scores hold a NaN")
        if p is not None and bool(((p < 0) | (p >= K)).any()):
            raise ValueError(f"BootstrapMetrics.{what}: a prediction lies outside [0, {K})")
        return s, y, p

    @staticmethod
    def _to_device(s, y, p):
        if not torch.cuda.is_available():
            raise MMSkinError("BootstrapMetrics needs a HIP device; there is no CPU fallback")
        dev = s.device if s.is_cuda else torch.device("cuda", torch.cuda.current_device())
        return s.to(dev).contiguous(), y.to(dev), (None if p is None else p.to(dev))

    # ------------------------------------------------------------------------------------------ the study
    def _tables(self, s, y, p):
        return ops.bootstrap_tables(s, y, p)

    def _study(self, tables):
        """device tensors: point metrics [M, 1], metrics [M, B], summary [5, M] and the four integer arrays"""
        K, B, dev = tables["K"], self.n_resamples, tables["labels"].device
        mode = ops.BOOTSTRAP_STRATIFIED if self.stratified else ops.BOOTSTRAP_PLAIN
        point_conf, point_counts = ops.bootstrap_accumulators(1, K, dev)
        ops.bootstrap_replicates(tables, self.seed, ops.BOOTSTRAP_POINT, point_conf, point_counts)
        point = ops.bootstrap_finalize(point_conf, point_counts, self.confidence)[0]
        conf, counts = ops.bootstrap_accumulators(B, K, dev)
        step = self.replicates_per_call or B
        for b0 in range(0, B, step):
            ops.bootstrap_replicates(tables, self.seed, mode, conf, counts, b0, min(b0 + step, B))
        metrics, summary = ops.bootstrap_finalize(conf, counts, self.confidence)
        return point, metrics, summary, (point_conf, point_counts, conf, counts)

    def _result(self, study, K, return_counts):
        point, metrics, summary, ints = study
        integers = None
        if return_counts:
            pc, pn, c, n = (t.cpu().numpy() for t in ints)
            split = lambda a: {"pos": a[..., :K].copy(), "neg": a[..., K:2 * K].copy(), "wins2": a[..., 2 * K:].copy()}
            integers = (pc[0], split(pn[0]), c, split(n))
        return BootstrapResult(point.cpu().numpy(), metrics.cpu().numpy(), summary.cpu().numpy(), K, self.confidence, integers)

    def evaluate(self, scores, labels, preds=None, return_counts=False):
        """scores fp32 [N, K] (soft-max rows), labels integer [N], preds integer [N] or None (the first arg-max of each row): numpy
        arrays or tensors, on the host or the device.  Returns a BootstrapResult."""
        s, y, p = self._to_device(*self._fold("evaluate", scores, labels, preds))
        with torch.no_grad():
            tables = self._tables(s, y, p)
            return self._result(self._study(tables), tables["K"], return_counts)

    def compare(self, scores_a, scores_b, labels, preds_a=None, preds_b=None):
        """Two score tables fp32 [N, K] on the same labels: the per-replicate differences metric(A) - metric(B) under the same
        resamples.  Returns a BootstrapComparison."""
        fa = self._fold("compare", scores_a, labels, preds_a)
        fb = self._fold("compare", scores_b, labels, preds_b)
        if fa[0].shape != fb[0].shape:
            raise ValueError(f"BootstrapMetrics.compare: the score tables differ in shape: {tuple(fa[0].shape)} and {tuple(fb[0].shape)}")
        fa, fb = self._to_device(*fa), self._to_device(*fb)
        with torch.no_grad():
            ta, tb = self._tables(*fa), self._tables(*fb)
            K = ta["K"]
            sa, sb = self._study(ta), self._study(tb)
            point = ops.bootstrap_compare(sa[0], sb[0], self.confidence)[0]
            delta, summary, signs = ops.bootstrap_compare(sa[1], sb[1], self.confidence)
            return BootstrapComparison(self._result(sa, K, False), self._result(sb, K, False), point.cpu().numpy(), delta.cpu().numpy(),
                                       summary.cpu().numpy(), signs.cpu().numpy(), K)

    def from_fold_dir(self, path, return_counts=False):
        """`evaluate` on the probabilities.npy, labels.npy and predictions.npy that evaluate_model wrote into `path`"""
        load = lambda name: np.load(os.path.join(path, name))
        return self.evaluate(load("probabilities.npy").astype(np.float32, copy=False), load("labels.npy"), load("predictions.npy"),
                             return_counts=return_counts)
