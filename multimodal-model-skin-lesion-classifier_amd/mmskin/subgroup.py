"""Subgroup audit of a validation fold, on the GPU: for WHOM is the model good?

`BootstrapMetrics` says how good a fold is and how sure that number is.  `SubgroupAudit` asks the same of every group of rows --
Fitzpatrick type, sex, age band, body region: the reference's METADATA_GROUPS["demographics"] -- and of the differences between
them.  It is the same bootstrap: one workgroup per replicate draws the weights w_b of `mmskin_bootstrap_weights` on the WHOLE fold
and scores every group under them as exact integers (the confusion cells of the group's rows, and the Mann-Whitney counts of the
one-vs-rest AUC over the pairs that lie inside the group; csrc/subgroup.hip, include/mmskin.h).  So a group's
replicate, another group's and the fold's own are one resample: `difference` and `versus_overall` are paired differences, and
`compare` puts two models' gaps under the same resamples.

    groups, names = group_ids(frame["fitspatrick"])                       # or group_ids(frame["age"], bins=[40, 70])
    audit = SubgroupAudit(n_resamples=2000, seed=0, min_rows=10)
    res = audit.evaluate(probs, labels, groups, group_names=names)        # or audit.from_fold_dir(folder, groups)
    res.overall.point["balanced_accuracy"], res.overall.interval("balanced_accuracy")
    res.by_name("5.0").low["per_class_recall"], res.group[2].n_rows
    res.gap.point["auc"], res.gap.interval("auc"), res.lowest_share["auc"]
    res.difference(0, 3).p_value["per_class_fpr"], res.versus_overall(2).low["accuracy"]
    audit.compare(probs_a, probs_b, labels, groups).p_value["balanced_accuracy"]     # does model A have the smaller gap?

The metrics are those of `BootstrapMetrics` plus, per class, the false-positive rate and the predicted rate.  `point` is always the
fold's own value (every weight 1), never a mean of replicates.  A metric that is undefined for a group in a replicate (the group
drew no row of a class, or fewer than `min_rows` rows at all) is NaN there and leaves that group's `n_valid`; `gap`, `lowest` and
`highest` of a replicate range over the groups that are defined in it.

READ `gap` WITH CARE: the largest minus the smallest of G noisy numbers is biased upward.  Groups that perform identically still
show a positive gap, the more so the smaller and the more numerous they are; its `point` and its interval describe the observed
spread, not the spread of the true group values.  `difference(a, b)` of two groups named in advance has no such bias.

Rows whose label lies outside [0, K) are dropped first, with their group ids; a row whose group id is negative (unknown) stays in
the fold -- it is drawn, it counts in `overall` -- and belongs to no group.  GPU only.
"""
import os

import numpy as np
import torch

from . import ops
from ._lib import MMSkinError

METRICS = ops.BOOTSTRAP_METRICS
CLASS_METRICS = ops.SUBGROUP_CLASS_METRICS
_FIELDS = ("mean", "std", "low", "high")


def _missing(v):
    if v is None:
        return True
    if isinstance(v, str):
        return v.strip() == ""
    try:
        return bool(v != v)
    except (TypeError, ValueError):
        return False


def group_ids(values, bins=None):
    """A metadata column -> (ids int32 [N], names list).  Without `bins` the column is categorical: the sorted distinct values are
    the groups 0 .. G-1 and their str() the names.  With `bins` (ascending edges) it is numeric: id = np.digitize(value, bins), the
    G = len(bins) + 1 groups named "< e0", "[e0, e1)", ..., ">= e_last".  NaN, None and "" (blank strings) give -1: no group."""
    vals = list(values.tolist() if isinstance(values, np.ndarray) else values)
    gone = np.array([_missing(v) for v in vals], dtype=bool)
    ids = np.full(len(vals), -1, dtype=np.int32)
    if bins is not None:
        edges = np.asarray(bins, dtype=np.float64)
        if edges.ndim != 1 or len(edges) < 1 or np.isnan(edges).any() or (np.diff(edges) <= 0).any():
            raise ValueError(f"group_ids: bins must be ascending edges, got {bins}")
        kept = np.array([float(v) for v, g in zip(vals, gone) if not g], dtype=np.float64)
        ids[~gone] = np.digitize(kept, edges).astype(np.int32)
        e = [f"{x:g}" for x in edges]
        return ids, [f"< {e[0]}"] + [f"[{a}, {b})" for a, b in zip(e[:-1], e[1:])] + [f">= {e[-1]}"]
    distinct = {v for v, g in zip(vals, gone) if not g}
    try:
        distinct = sorted(distinct)
    except TypeError:                                                # mixed types: order them by their names
        distinct = sorted(distinct, key=str)
    index = {v: k for k, v in enumerate(distinct)}
    ids[~gone] = [index[v] for v, g in zip(vals, gone) if not g]
    return ids, [str(v) for v in distinct]


def _by_metric(table, K):
    """a [7 + 4 K, ...] array -> {name: [...] for the scalar metrics, name: [K, ...] moved to [..., K] for the per-class ones}"""
    out = {m: table[k] for k, m in enumerate(METRICS)}
    for j, m in enumerate(CLASS_METRICS):
        out[m] = np.moveaxis(table[7 + j * K:7 + (j + 1) * K], 0, -1)
    return out


def _scalars(d):
    return {m: (float(v) if np.ndim(v) == 0 else np.ascontiguousarray(v)) for m, v in d.items()}


def _counts(d):
    return {m: (int(v) if np.ndim(v) == 0 else v.astype(np.int64)) for m, v in d.items()}


class SubgroupTable:
    """One row set's study -- the fold (`overall`), a group, or `gap` / `lowest` / `highest` -- on the host.  Dicts keyed by the
    names of ops.BOOTSTRAP_METRICS (floats) and ops.SUBGROUP_CLASS_METRICS (float64 [K]): `point` (the fold's own value), `mean`,
    `std` (ddof = 1), `low`, `high` (the percentile interval at `confidence`), `n_valid` (the replicates in which the metric is
    defined) and `replicates` (float64 [B], [B, K] for the per-class ones).  A group also has `name`, `n_rows` and `class_counts`
    int64 [K] (on the fold itself), and with return_counts=True `confusion` int32 [B, K, K], `counts` dict(pos, neg, wins2: int64
    [B, K]) and their `point_confusion` / `point_counts`."""

    def __init__(self, point, replicates, summary, K, confidence):
        self.num_classes, self.confidence = K, confidence
        self.point = _scalars(_by_metric(point, K))
        self.replicates = {m: np.ascontiguousarray(v) for m, v in _by_metric(replicates, K).items()}
        rows = {name: _scalars(_by_metric(summary[k], K)) for k, name in enumerate(ops.BOOTSTRAP_SUMMARY)}
        self.mean, self.std, self.low, self.high = (rows[f] for f in _FIELDS)
        self.n_valid = _counts(rows["n_valid"])

    def interval(self, metric):
        """(low, high) of the percentile interval: floats, or [K] arrays for a per-class metric"""
        return self.low[metric], self.high[metric]


class SubgroupDifference(SubgroupTable):
    """A paired difference a - b of two metric tables under the same resamples: the fields of SubgroupTable on the per-replicate
    differences (`n_valid`: the replicates in which both sides are defined) and `p_value` = min(1, 2 min((#{d <= 0} + 1) / (n + 1),
    (#{d >= 0} + 1) / (n + 1))) over those n replicates, BootstrapComparison's rule."""

    def __init__(self, point, delta, summary, sign_counts, K, confidence):
        super().__init__(point, delta, summary, K, confidence)
        n = summary[0]
        p = np.minimum(1.0, 2.0 * np.minimum((sign_counts[:, 0] + 1) / (n + 1), (sign_counts[:, 1] + 1) / (n + 1)))
        self.p_value = _scalars(_by_metric(p, K))


class SubgroupResult:
    """What `SubgroupAudit.evaluate` returns.  `overall`: the fold through the same kernels with one group.  `group`: a list of G
    SubgroupTables, `names` their names, `by_name(name)` one of them.  `gap`, `lowest`, `highest`: SubgroupTables over the groups
    defined in each replicate (gap = highest - lowest, NaN with fewer than two; see the module docstring on its bias).
    `lowest_share[metric]`: float64 [G] (per-class metrics: [K, G]), the share of the replicates with a defined lowest in which each
    group is it, ties going to the smallest id.  `difference(a, b)` and `versus_overall(g)` are paired SubgroupDifferences."""

    def __init__(self, K, G, names, confidence, overall, groups, spread, lowest_share, device_tables):
        self.num_classes, self.num_groups, self.names, self.confidence = K, G, list(names), confidence
        self.overall, self.group = overall, groups
        self.lowest, self.highest, self.gap = spread
        self.lowest_share = lowest_share
        self._dev = device_tables                                   # point [G + 1, M, 1] and metrics [G + 1, M, B]; the fold is row G

    def _index(self, g):
        if isinstance(g, str):
            if g not in self.names:
                raise KeyError(f"SubgroupResult: no group named {g!r}; the groups are {self.names}")
            return self.names.index(g)
        g = int(g)
        if not 0 <= g < self.num_groups:
            raise IndexError(f"SubgroupResult: group {g} is outside [0, {self.num_groups})")
        return g

    def by_name(self, name):
        return self.group[self._index(name)]

    def _delta(self, a, b):
        point, metrics = self._dev
        with torch.no_grad(), torch.cuda.device(metrics.device):
            p = ops.subgroup_compare(point[a], point[b], self.confidence)[0]
            delta, summary, signs = ops.subgroup_compare(metrics[a], metrics[b], self.confidence)
        return SubgroupDifference(p.cpu().numpy()[:, 0], delta.cpu().numpy(), summary.cpu().numpy(), signs.cpu().numpy(), self.num_classes,
                                  self.confidence)

    def difference(self, a, b):
        """group a - group b (ids or names), paired: point, interval, p-value"""
        return self._delta(self._index(a), self._index(b))

    def versus_overall(self, g):
        """group g - the fold, paired"""
        return self._delta(self._index(g), self.num_groups)


class SubgroupComparison(SubgroupDifference):
    """What `SubgroupAudit.compare` returns: gap(A) - gap(B) per metric and replicate under the same resamples, as a
    SubgroupDifference (a negative difference: model A treats the groups more evenly), with the two SubgroupResults `a` and `b`."""

    def __init__(self, a, b, *args):
        super().__init__(*args)
        self.a, self.b = a, b


class SubgroupAudit:
    def __init__(self, n_resamples=2000, seed=0, confidence=0.95, stratified=False, min_rows=1, replicates_per_call=None):
        """
        n_resamples: B replicates, 1 .. ops.BOOTSTRAP_MAX_RESAMPLES.  seed: of the device generator; the resamples are those of
        BootstrapMetrics with the same seed.  confidence: of the percentile interval, in (0, 1).
        stratified: resample within each class of the FOLD (a group's class counts still vary).
        min_rows: a group that drew fewer rows than this in a replicate is undefined (NaN) in it; >= 1.
        replicates_per_call: replicates per kernel launch (None: all at once); it cuts the study and changes no result.
        """
        self.n_resamples, self.seed, self.stratified = int(n_resamples), int(seed), bool(stratified)
        ops.subgroup_check_limits("SubgroupAudit", B=self.n_resamples)
        self.confidence = float(confidence)
        if not 0.0 < self.confidence < 1.0:
            raise ValueError(f"SubgroupAudit: confidence must lie in (0, 1), got {confidence}")
        self.min_rows = int(min_rows)
        if self.min_rows < 1:
            raise ValueError(f"SubgroupAudit: min_rows must be >= 1, got {min_rows}")
        if replicates_per_call is not None and int(replicates_per_call) < 1:
            raise ValueError(f"SubgroupAudit: replicates_per_call must be >= 1, got {replicates_per_call}")
        self.replicates_per_call = None if replicates_per_call is None else int(replicates_per_call)

    # ------------------------------------------------------------------------------------------ arguments
    def _fold(self, what, scores, labels, groups, preds, group_names):
        """the checked arguments with the rows whose label is outside [0, K) dropped: (scores fp32 [N, K], labels, groups, preds or
        None, G, names).  Everything here is an argument error (ValueError) or a limit (MMSkinError) and needs no device."""
        s = torch.as_tensor(scores)
        if s.dim() != 2 or s.dtype != torch.float32:
            raise ValueError(f"SubgroupAudit.{what}: scores must be an fp32 [N, K] array, got {s.dtype} {tuple(s.shape)}")
        rows, K = s.shape

        def integer_rows(name, v):
            t = torch.as_tensor(v)
            if tuple(t.shape) != (rows,) or t.dtype.is_floating_point or t.dtype == torch.bool or t.dtype.is_complex:
                raise ValueError(f"SubgroupAudit.{what}: {name} must be an integer {(rows,)} array, got {t.dtype} {tuple(t.shape)}")
            return t

        y, g = integer_rows("labels", labels), integer_rows("groups", groups)
        p = None if preds is None else integer_rows("preds", preds)
        ops.subgroup_check_limits(f"SubgroupAudit.{what}", K=K)
        if y.device != s.device or g.device != s.device or (p is not None and p.device != s.device):
            raise ValueError(f"SubgroupAudit.{what}: scores, labels, groups and preds must live on one device")
        keep = (y >= 0) & (y < K)
        if not bool(keep.all()):
            s, y, g, p = s[keep], y[keep], g[keep], (None if p is None else p[keep])
        ops.subgroup_check_limits(f"SubgroupAudit.{what}", N=int(s.shape[0]))
        if group_names is not None:
            names = [str(n) for n in group_names]
            if len(names) < 1 or len(set(names)) != len(names):
                raise ValueError(f"SubgroupAudit.{what}: group_names must be distinct and not empty, got {names}")
            G = len(names)
            if bool((g >= G).any()):
                raise ValueError(f"SubgroupAudit.{what}: a group id lies beyond the {G} group_names")
        else:
            G = max(int(g.max()) + 1, 1)
            names = [str(k) for k in range(min(G, ops.SUBGROUP_MAX_GROUPS + 1))]
        ops.subgroup_check_limits(f"SubgroupAudit.{what}", K=K, G=G)
        if bool(torch.isnan(s).any()):
            raise ValueError(f"SubgroupAudit.{what}: the scores hold a NaN")
        if p is not None and bool(((p < 0) | (p >= K)).any()):
            raise ValueError(f"SubgroupAudit.{what}: a prediction lies outside [0, {K})")
        return s, y, g, p, G, names

    @staticmethod
    def _to_device(s, y, g, p):
        if not torch.cuda.is_available():
            raise MMSkinError("SubgroupAudit needs a HIP device; there is no CPU fallback")
        dev = s.device if s.is_cuda else torch.device("cuda", torch.cuda.current_device())
        return s.to(dev).contiguous(), y.to(dev), g.to(dev), (None if p is None else p.to(dev))

    # ------------------------------------------------------------------------------------------ the study
    def _study(self, tables):
        """device tensors of one grouping: point metrics [G, M, 1], metrics [G, M, B], summary [G, 5, M] and the four integer arrays"""
        K, G, B, dev = tables["K"], tables["G"], self.n_resamples, tables["labels"].device
        mode = ops.BOOTSTRAP_STRATIFIED if self.stratified else ops.BOOTSTRAP_PLAIN
        point_conf, point_counts = ops.subgroup_accumulators(1, G, K, dev)
        ops.subgroup_replicates(tables, self.seed, ops.BOOTSTRAP_POINT, point_conf, point_counts)
        point = ops.subgroup_finalize(point_conf, point_counts, self.confidence, self.min_rows)[0]
        conf, counts = ops.subgroup_accumulators(B, G, K, dev)
        step = self.replicates_per_call or B
        for b0 in range(0, B, step):
            ops.subgroup_replicates(tables, self.seed, mode, conf, counts, b0, min(b0 + step, B))
        metrics, summary = ops.subgroup_finalize(conf, counts, self.confidence, self.min_rows)
        return point, metrics, summary, (point_conf, point_counts, conf, counts)

    def _audit(self, s, y, g, p, G, names, return_counts):
        """-> (SubgroupResult, device gap tables (point [M, 1], replicates [M, B]))"""
        K, conf = int(s.shape[1]), self.confidence
        with torch.no_grad(), torch.cuda.device(s.device):
            fold = self._study(ops.subgroup_tables(s, y, torch.zeros_like(g), 1, p))
            per = self._study(ops.subgroup_tables(s, y, g, G, p))
            spread_point = ops.subgroup_gaps(per[0], conf)
            spread = ops.subgroup_gaps(per[1], conf)
            device_tables = (torch.cat([per[0], fold[0]]), torch.cat([per[1], fold[1]]))

        def on_host(study):                                          # one copy per array, whatever G is
            point, metrics, summary, (pc, pn, c, n) = study
            ints = (pc, pn, c, n) if return_counts else (pn,)
            return [t.cpu().numpy() for t in (point, metrics, summary)] + [t.cpu().numpy() for t in ints]

        def tables_of(host, k):
            point, metrics, summary = host[:3]
            t = SubgroupTable(point[k, :, 0], metrics[k], summary[k], K, conf)
            pn = host[4] if return_counts else host[3]
            t.n_rows, t.class_counts = int(pn[0, k, :K].sum()), pn[0, k, :K].copy()
            if return_counts:
                split = lambda a: {"pos": a[..., :K].copy(), "neg": a[..., K:2 * K].copy(), "wins2": a[..., 2 * K:].copy()}
                pc, _, c, n = host[3:]
                t.point_confusion, t.point_counts = pc[0, k].copy(), split(pn[0, k])
                t.confusion, t.counts = np.ascontiguousarray(c[:, k]), split(n[:, k])
            return t

        fold_host, per_host = on_host(fold), on_host(per)
        overall = tables_of(fold_host, 0)
        groups = [tables_of(per_host, k) for k in range(G)]
        for t, name in zip(groups, names):
            t.name = name
        summaries = spread[4].cpu().numpy()
        spread_tables = tuple(SubgroupTable(spread_point[k][:, 0].cpu().numpy(), spread[k].cpu().numpy(), summaries[k], K, conf) for k in range(3))
        low_counts = spread[3].cpu().numpy().astype(np.float64)                               # [M, G]
        total = low_counts.sum(axis=1, keepdims=True)
        share = np.divide(low_counts, total, out=np.full_like(low_counts, np.nan), where=total > 0)
        lowest_share = {m: np.ascontiguousarray(v) for m, v in _by_metric(share, K).items()}
        for m in CLASS_METRICS:                                      # _by_metric moved the class axis last: [G, K] -> [K, G]
            lowest_share[m] = np.ascontiguousarray(lowest_share[m].T)
        res = SubgroupResult(K, G, names, conf, overall, groups, spread_tables, lowest_share, device_tables)
        return res, (spread_point[2], spread[2])

    def evaluate(self, scores, labels, groups, preds=None, group_names=None, return_counts=False):
        """scores fp32 [N, K] (soft-max rows), labels integer [N], groups integer [N] (0 .. G-1, negative: unknown), preds integer
        [N] or None (the first arg-max of each row): numpy arrays or tensors, on the host or the device.  group_names: G names (G =
        the largest id + 1 without them).  Returns a SubgroupResult."""
        s, y, g, p, G, names = self._fold("evaluate", scores, labels, groups, preds, group_names)
        s, y, g, p = self._to_device(s, y, g, p)
        return self._audit(s, y, g, p, G, names, return_counts)[0]

    def compare(self, scores_a, scores_b, labels, groups, preds_a=None, preds_b=None, group_names=None):
        """Two score tables fp32 [N, K] on the same labels and groups: does model A have the smaller gap?  gap(A) - gap(B) per
        metric and replicate under the same resamples.  Returns a SubgroupComparison."""
        fa = self._fold("compare", scores_a, labels, groups, preds_a, group_names)
        fb = self._fold("compare", scores_b, labels, groups, preds_b, group_names)
        if fa[0].shape != fb[0].shape:
            raise ValueError(f"SubgroupAudit.compare: the score tables differ in shape: {tuple(fa[0].shape)} and {tuple(fb[0].shape)}")
        (ra, ga), (rb, gb) = (self._audit(*self._to_device(*f[:4]), f[4], f[5], False) for f in (fa, fb))
        with torch.no_grad(), torch.cuda.device(ga[1].device):
            point = ops.subgroup_compare(ga[0], gb[0], self.confidence)[0]
            delta, summary, signs = ops.subgroup_compare(ga[1], gb[1], self.confidence)
        return SubgroupComparison(ra, rb, point.cpu().numpy()[:, 0], delta.cpu().numpy(), summary.cpu().numpy(), signs.cpu().numpy(),
                                  ra.num_classes, self.confidence)

    def from_fold_dir(self, path, groups, group_names=None, return_counts=False):
        """`evaluate` on the probabilities.npy, labels.npy and predictions.npy that evaluate_model wrote into `path`; `groups` are
        the group ids of those rows, in their order"""
        load = lambda name: np.load(os.path.join(path, name))
        return self.evaluate(load("probabilities.npy").astype(np.float32, copy=False), load("labels.npy"), groups, load("predictions.npy"),
                             group_names=group_names, return_counts=return_counts)
