"""Can a fold's probabilities be believed?  Reliability tables, ECE / MCE / class-wise ECE, Brier score and NLL of the soft-max rows
that `mmskin.evaluate.evaluate_model` returns, their bootstrap intervals, and post-hoc temperature scaling, on the GPU.

    cal = Calibration(n_bins=15, binning="uniform")                 # or "quantile"
    rep = cal.evaluate(probs, labels)                               # numpy or tensors, host or device
    rep.point["ece"], rep.point["per_class_ece"], rep.reliability["accuracy"], rep.class_reliability["count"]
    rep = cal.evaluate(probs, labels, n_resamples=2000, seed=0, confidence=0.95)
    rep.low["ece"], rep.high["ece"], rep.interval("brier")
    ts = TemperatureScaling().fit(scores, labels, from_logits=False)
    cal.evaluate(ts.apply(scores), labels)                          # the calibrated fold

There are K + 1 reliability tables: the top-label one (confidence = the row's largest probability, hit = the first arg-max is the
label) and one per class, one-vs-rest.  Bins are right-closed; a table entry is an exact integer (count, hits, and the sum of the
confidences in units of 2^-30), so every metric is a function of integers and does not depend on the order of summation
(csrc/calibration.hip; the definitions are in include/mmskin.h and DESIGN.md section 24).  The resamples are those of
`mmskin.bootstrap.BootstrapMetrics` for the same seed (ops.bootstrap_weights), so the two studies can be read side by side.
Quantile edges are fixed from the fold and NOT recomputed per replicate: the interval is that of the metric with these bins.
Rows whose label lies outside [0, K) are dropped first.  Inputs on the host take a numpy path for the plain evaluation (the same
integers); a resampled study and temperature scaling need a HIP device.
"""
import math
import os

import numpy as np
import torch

from . import ops
from ._lib import MMSkinError

METRICS = ops.CALIBRATION_METRICS
CLASS_METRICS = ops.CALIBRATION_CLASS_METRICS
_S = 1 << ops.CALIBRATION_CONF_SCALE_LOG2


def _by_metric(table, K):
    """a [6 + K, ...] array -> {name: [...] for the scalar metrics, "per_class_ece": [..., K]}"""
    out = {m: table[k] for k, m in enumerate(METRICS)}
    out[CLASS_METRICS[0]] = np.moveaxis(table[6:6 + K], 0, -1)
    return out


def _scalars(d):
    return {m: (float(v) if np.ndim(v) == 0 else np.ascontiguousarray(v)) for m, v in d.items()}


# ------------------------------------------------------------------------------------------------ the host path (unweighted)
def host_tables(probs, labels, edges):
    """int64 [K + 1, n_bins, 3] (count, hits, conf) of the fold in numpy: the integers of mmskin_calibration_codes / _bins"""
    N, K = probs.shape
    n_bins = edges.shape[1] - 1
    pred = probs.argmax(axis=1)
    conf = ops.calibration_confidences(probs)
    hit = np.concatenate([(pred == labels)[None], labels[None] == np.arange(K)[:, None]], axis=0)
    q = np.rint(conf.astype(np.float64) * _S).astype(np.int64)
    tables = np.zeros((K + 1, n_bins, 3), dtype=np.int64)
    for t in range(K + 1):
        b = np.searchsorted(edges[t, 1:n_bins], conf[t], side="left")
        tables[t, :, 0] = np.bincount(b, minlength=n_bins)
        tables[t, :, 1] = np.bincount(b[hit[t]], minlength=n_bins)
        np.add.at(tables[t, :, 2], b, q[t])
    return tables


def host_sums(probs, labels):
    """(Brier sum, NLL sum) of the fold in fp64"""
    p = probs.astype(np.float64)
    rows = np.arange(len(labels))
    onehot = np.zeros_like(p)
    onehot[rows, labels] = 1.0
    at_label = np.maximum(probs[rows, labels], np.finfo(np.float32).tiny).astype(np.float64)
    return float(((p - onehot) ** 2).sum()), float(-np.log(at_label).sum())


def metrics_from_tables(tables, sums):
    """float64 [6 + K]: the metric columns of mmskin_calibration_finalize from one replicate's integers, in Python integers"""
    K = tables.shape[0] - 1
    out = np.full(6 + K, np.nan)
    W = int(tables[0, :, 0].sum())
    if W == 0:
        return out
    for t in range(K + 1):
        gaps = [abs(int(h) * _S - int(c)) for _, h, c in tables[t]]
        ece = sum(gaps) / (_S * W)
        if t == 0:
            out[0] = ece
            out[1] = max(g / (_S * int(n)) for g, (n, _, _) in zip(gaps, tables[t]) if n > 0)
            out[3] = (int(tables[0, :, 2].sum()) - _S * int(tables[0, :, 1].sum())) / (_S * W)
        else:
            out[5 + t] = ece
    total = 0.0
    for c in range(K):
        total += out[6 + c]
    out[2] = total / K
    out[4], out[5] = sums[0] / W, sums[1] / W
    return out


def _reliability(tables, edges):
    count = tables[..., 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.where(count > 0, tables[..., 1] / count, np.nan)
        conf = np.where(count > 0, tables[..., 2] / (float(_S) * count), np.nan)
    return {"edges": edges.copy(), "count": count.copy(), "accuracy": acc, "confidence": conf}


class CalibrationReport:
    """What `Calibration.evaluate` returns, all on the host.  `point`: dict keyed by ops.CALIBRATION_METRICS (floats) and
    "per_class_ece" (float64 [K]).  `reliability`: dict(edges [n_bins + 1], count int64 [n_bins], accuracy, confidence float64
    [n_bins], NaN in empty bins) of the top-label table; `class_reliability`: the same per class, [K, ...].  `tables`: the integers,
    int64 [K + 1, n_bins, 3].  After a resampled study also `mean`, `std` (ddof = 1), `low`, `high`, `n_valid` and `replicates`
    (float64 [B], [B, K] per class), as in BootstrapResult."""

    def __init__(self, point, tables, edges, K, confidence=None, replicates=None, summary=None):
        self.num_classes, self.confidence, self.tables, self.edges = K, confidence, tables, edges
        self.point = _scalars(_by_metric(point, K))
        self.reliability = _reliability(tables[0], edges[0])
        self.class_reliability = _reliability(tables[1:], edges[1:])
        self.replicates = self.mean = self.std = self.low = self.high = self.n_valid = None
        if replicates is not None:
            self.replicates = {m: np.ascontiguousarray(v) for m, v in _by_metric(replicates, K).items()}
            rows = {name: _scalars(_by_metric(summary[k], K)) for k, name in enumerate(ops.BOOTSTRAP_SUMMARY)}
            self.mean, self.std, self.low, self.high = rows["mean"], rows["std"], rows["low"], rows["high"]
            self.n_valid = {m: (int(v) if np.ndim(v) == 0 else v.astype(np.int64)) for m, v in rows["n_valid"].items()}

    def interval(self, metric):
        """(low, high) of the percentile interval of a resampled study"""
        if self.low is None:
            raise ValueError("CalibrationReport.interval: the report holds no resampled study (n_resamples was None)")
        return self.low[metric], self.high[metric]


def _checked_scores(what, scores, labels, probabilities):
    """(scores fp32 [N, K], labels int64 [N]) as host-or-device tensors with the rows whose label lies outside [0, K) dropped.
    Everything here is an argument error (ValueError) or a limit (MMSkinError) and needs no device."""
    s = torch.as_tensor(scores)
    if s.dim() != 2 or s.dtype != torch.float32:
        raise ValueError(f"{what}: the scores must be an fp32 [N, K] array, got {s.dtype} {tuple(s.shape)}")
    rows, K = s.shape
    y = torch.as_tensor(labels)
    if tuple(y.shape) != (rows,) or y.dtype.is_floating_point or y.dtype == torch.bool or y.dtype.is_complex:
        raise ValueError(f"{what}: labels must be an integer {(rows,)} array, got {y.dtype} {tuple(y.shape)}")
    ops.calibration_check_limits(what, K=K)
    if y.device != s.device:
        raise ValueError(f"{what}: the scores and the labels must live on one device")
    y = y.long()
    keep = (y >= 0) & (y < K)
    if not bool(keep.all()):
        s, y = s[keep], y[keep]
    ops.calibration_check_limits(what, N=int(s.shape[0]))
    if bool(torch.isnan(s).any()):
        raise ValueError(f"{what}: the scores hold a NaN")
    if probabilities and bool(((s < 0) | (s > 1)).any()):
        raise ValueError(f"{what}: a probability lies outside [0, 1]")
    if not probabilities and bool(torch.isinf(s).any()):
        raise ValueError(f"{what}: a logit is infinite")
    return s.contiguous(), y.contiguous()


def read_fold_dir(path):
    """(probs fp32 [N, K], labels [N]) from the probabilities.npy and labels.npy that evaluate_model wrote into `path`"""
    load = lambda name: np.load(os.path.join(path, name))
    return load("probabilities.npy").astype(np.float32, copy=False), load("labels.npy")


def _device_of(t):
    if not torch.cuda.is_available():
        return None
    return t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())


class Calibration:
    def __init__(self, n_bins=15, binning="uniform", replicates_per_call=None):
        """n_bins: 1 .. ops.CALIBRATION_MAX_BINS bins per table.  binning: "uniform" (edges j / n_bins) or "quantile" (per table,
        about N / n_bins rows per bin; ops.calibration_edges).  replicates_per_call: replicates per kernel launch of a resampled
        study (None: all at once); it cuts the study and changes no result."""
        self.n_bins = int(n_bins)
        ops.calibration_check_limits("Calibration", n_bins=self.n_bins)
        if binning not in ops.CALIBRATION_BINNINGS:
            raise ValueError(f"Calibration: binning must be one of {ops.CALIBRATION_BINNINGS}, got {binning!r}")
        self.binning = binning
        if replicates_per_call is not None and int(replicates_per_call) < 1:
            raise ValueError(f"Calibration: replicates_per_call must be >= 1, got {replicates_per_call}")
        self.replicates_per_call = None if replicates_per_call is None else int(replicates_per_call)

    def evaluate(self, probs, labels, n_resamples=None, seed=0, confidence=0.95, stratified=False):
        """probs fp32 [N, K] (soft-max rows), labels integer [N]: numpy arrays or tensors, on the host or the device.  With
        n_resamples = B also the bootstrap of every metric over B resamples of the rows (the weights of ops.bootstrap_weights for
        `seed`, stratified by label on request), which inherits the bootstrap's row limit.  Returns a CalibrationReport."""
        s, y = _checked_scores("Calibration.evaluate", probs, labels, probabilities=True)
        K = int(s.shape[1])
        if n_resamples is not None:
            B, confidence = int(n_resamples), float(confidence)
            ops.calibration_check_limits("Calibration.evaluate", R=B)
            if not 0.0 < confidence < 1.0:
                raise ValueError(f"Calibration.evaluate: confidence must lie in (0, 1), got {confidence}")
            if s.shape[0] > ops.BOOTSTRAP_MAX_ROWS:
                raise MMSkinError(f"Calibration.evaluate: {s.shape[0]} rows; the resample weights are those of the bootstrap, which "
                                  f"holds 1 .. BOOTSTRAP_MAX_ROWS = {ops.BOOTSTRAP_MAX_ROWS} rows (the plain evaluation holds "
                                  f"{ops.CALIBRATION_MAX_ROWS})")
        dev = _device_of(s)
        if n_resamples is None and not s.is_cuda:                                            # the host path: the same integers
            p, lab = s.numpy(), y.numpy()
            edges = ops.calibration_edges(p, lab, self.n_bins, self.binning)
            tables = host_tables(p, lab, edges)
            return CalibrationReport(metrics_from_tables(tables, host_sums(p, lab)), tables, edges, K)
        if dev is None:
            raise MMSkinError("Calibration.evaluate: a resampled study needs a HIP device; there is no CPU fallback")
        with torch.no_grad(), torch.cuda.device(dev):
            s, y = s.to(dev), y.to(dev)
            edges = ops.calibration_edges(s, y, self.n_bins, self.binning)
            codes = ops.calibration_codes(s, y, edges)
            tables = ops.calibration_bins(codes, self.n_bins)
            point = ops.calibration_finalize(tables, ops.calibration_sums(s, y))[0][:, 0]
            host = lambda t: t.cpu().numpy()
            if n_resamples is None:
                return CalibrationReport(host(point), host(tables)[0], host(edges), K)
            N = int(s.shape[0])
            strata = ops.bootstrap_tables(s, y) if stratified else None
            rep_tables = torch.empty((B, K + 1, self.n_bins, 3), dtype=torch.int64, device=dev)
            rep_sums = torch.empty((B, 2), dtype=torch.float64, device=dev)
            step = self.replicates_per_call or B
            for b0 in range(0, B, step):
                w = ops.bootstrap_weights(seed, N, B, dev, b0, min(b0 + step, B), tables=strata)
                ops.calibration_bins(codes, self.n_bins, w, rep_tables, b0)
                rep_sums[b0:b0 + w.shape[0]] = ops.calibration_sums(s, y, w)
            metrics, summary = ops.calibration_finalize(rep_tables, rep_sums, confidence)
            return CalibrationReport(host(point), host(tables)[0], host(edges), K, confidence, host(metrics), host(summary))

    def from_fold_dir(self, path, **study):
        """`evaluate` on the probabilities.npy and labels.npy that evaluate_model wrote into `path`"""
        return self.evaluate(*read_fold_dir(path), **study)


class TemperatureScaling:
    """Post-hoc temperature scaling (Guo et al. 2017): the T > 0 that minimises the NLL of softmax(z / T) on a held-out fold.
    The NLL is convex in beta = 1 / T, so the solver runs on the sign of its derivative g(beta) = sum_i (E_pi[z] - z_y): one
    launch of ops.temperature_stats over 33 log-spaced candidates (and beta = 1, for `nll_before`) brackets the root, then
    safeguarded Newton steps -- a step that would leave the bracket is replaced by the bracket's geometric midpoint -- until
    |g| <= 1e-12 h beta (h the second derivative) or 30 launches.  The host drives it with one small read-back per launch.
    Special cases: g has one sign over the whole range (e.g. every row confidently right: the NLL falls all the way) -> the bound
    on that side, `at_bound` True; h = 0 and g = 0 everywhere (all logits of every row equal: T does nothing) -> T = 1.
    After `fit`: `temperature`, `beta`, `nll_before` (T = 1), `nll_after` (both means over the rows), `at_bound`, `n_launches`."""

    GRID, MAX_LAUNCHES, TOL = 33, 30, 1e-12

    def __init__(self, bounds=(1.0 / 64, 64.0)):
        lo, hi = float(bounds[0]), float(bounds[1])
        if not (0.0 < lo < hi < math.inf):
            raise ValueError(f"TemperatureScaling: bounds must satisfy 0 < low < high < inf, got {bounds}")
        self.bounds = (lo, hi)
        self.temperature = self.beta = self.nll_before = self.nll_after = self.at_bound = self.n_launches = None
        self.from_logits = False

    def fit(self, scores, labels, from_logits=False):
        """scores fp32 [N, K]: probabilities (soft-max is shift invariant: their logs serve as logits), or logits with from_logits"""
        s, y = _checked_scores("TemperatureScaling.fit", scores, labels, probabilities=not from_logits)
        dev = _device_of(s)
        if dev is None:
            raise MMSkinError("TemperatureScaling.fit needs a HIP device; there is no CPU fallback")
        self.from_logits = bool(from_logits)
        with torch.no_grad(), torch.cuda.device(dev):
            s, y = s.to(dev), y.to(dev)
            N = int(s.shape[0])
            launches = 0

            def stats(betas):
                nonlocal launches
                launches += 1
                return ops.temperature_stats(s, y, betas, from_probs=not from_logits).cpu().numpy()

            b_lo, b_hi = 1.0 / self.bounds[1], 1.0 / self.bounds[0]
            grid = np.exp(np.linspace(math.log(b_lo), math.log(b_hi), self.GRID))
            grid[0], grid[-1] = b_lo, b_hi
            first = stats(np.concatenate([grid, [1.0]]))
            self.nll_before = float(first[-1, 0]) / N
            g, h = first[:-1, 1], first[:-1, 2]
            self.at_bound = False
            if not h.any() and not g.any():
                beta, nll = 1.0, first[-1, 0]
            elif g[0] >= 0.0:                                                                # rising from the start: the smallest beta
                beta, nll, self.at_bound = b_lo, first[0, 0], True
            elif g[-1] <= 0.0:                                                               # still falling at the end
                beta, nll, self.at_bound = b_hi, first[-2, 0], True
            else:
                j = int(np.nonzero(g < 0.0)[0][-1])                                          # g[j] < 0 <= g[j + 1]
                lo, hi = grid[j], grid[j + 1]
                k = j if -g[j] < g[j + 1] else j + 1
                beta, nll, gk, hk = grid[k], first[k, 0], g[k], h[k]
                while abs(gk) > self.TOL * hk * beta and launches < self.MAX_LAUNCHES:
                    step = beta - gk / hk if hk > 0.0 else math.nan
                    beta = step if lo < step < hi else math.sqrt(lo * hi)
                    nll, gk, hk = stats([beta])[0]
                    if gk < 0.0:
                        lo = beta
                    else:
                        hi = beta
            self.beta, self.temperature = float(beta), 1.0 / float(beta)
            self.nll_after = float(nll) / N
            self.n_launches = launches
        return self

    def apply(self, scores, from_logits=None):
        """fp32 [N, K] = softmax(z / T) of scores like those `fit` saw (from_logits None: as fitted); a numpy array gives a numpy array"""
        if self.beta is None:
            raise ValueError("TemperatureScaling.apply: call fit first")
        logits = self.from_logits if from_logits is None else bool(from_logits)
        s = torch.as_tensor(scores)
        if s.dim() != 2 or s.dtype != torch.float32:
            raise ValueError(f"TemperatureScaling.apply: the scores must be an fp32 [N, K] array, got {s.dtype} {tuple(s.shape)}")
        ops.calibration_check_limits("TemperatureScaling.apply", N=int(s.shape[0]), K=int(s.shape[1]))
        dev = _device_of(s)
        if dev is None:
            raise MMSkinError("TemperatureScaling.apply needs a HIP device; there is no CPU fallback")
        with torch.no_grad(), torch.cuda.device(dev):
            out = ops.temperature_apply(s.to(dev).contiguous(), self.beta, from_probs=not logits)
        return out.cpu().numpy() if isinstance(scores, np.ndarray) else out.to(s.device)
