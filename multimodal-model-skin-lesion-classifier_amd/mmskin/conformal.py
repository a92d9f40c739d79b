"""Which diagnoses cannot be ruled out?  Split-conformal prediction sets from the soft-max rows that `mmskin.evaluate.evaluate_model`
returns: a set of classes per lesion that holds the true one with probability >= 1 - alpha, and the distribution of coverage and
set size over R random calibration / test splits of a fold, on the GPU.

    cp = ConformalPredictor(alpha=0.1, score="aps")                  # "lac", "aps" or "raps"
    rep = cp.study(probs, labels, n_resamples=2000, seed=0)          # numpy or tensors; or cp.from_fold_dir(folder, ...)
    rep.point["coverage"], rep.summary["mean"]["mean_set_size"], rep.summary["low"]["per_class_coverage"]
    rep.set_size_histogram, rep.class_coverage, rep.size_stratified_coverage, rep.replicates["covered"]
    cp.fit(cal_probs, cal_labels)                                    # cp.qhat_, cp.n_cal_
    mask, size = cp.predict_sets(test_probs)                         # device tensors: bit c of mask[i] = class c is in the set
    cp.predict_lists(test_probs, class_names=["ACK", "BCC", ...])

The scores (csrc/conformal.hip; the definitions are in include/mmskin.h and DESIGN.md section 27): "lac" 1 - p_y; "aps" the
probability of the classes ranked above y plus u p_y; "raps" that plus lam max(0, rank(y) - k_reg).  Classes are ranked by
descending probability, a tie going to the lower class index.  u in [0, 1) is a function of (seed, row index) alone; with
randomized=False u = 1, the conservative deterministic form.  The threshold qhat is the ceil((n + 1)(1 - alpha))-th smallest
calibration score, +inf (every class in every set) when that index exceeds n; mondrian=True keeps one threshold per class.
Every count of a study is an exact integer and depends on (inputs, seed, options) only.  Rows whose label lies outside [0, C) are
dropped first.  Everything here needs a HIP device; there is no CPU fallback.
"""
import json

import numpy as np
import torch

from . import ops
from ._lib import MMSkinError, call, load, ptr, stream
from .calibration import TemperatureScaling, read_fold_dir

MAX_ROWS = 32768                                                                             # MMSKIN_CONFORMAL_MAX_* of mmskin.h
MAX_CLASSES = 64
SCORES = ("lac", "aps", "raps")                                                              # MMSKIN_CONFORMAL_LAC, _APS, _RAPS
STRATIFIED, MONDRIAN = 1, 2                                                                  # MMSKIN_CONFORMAL_STRATIFIED, _MONDRIAN
METRICS = ("coverage", "mean_set_size", "singleton_rate", "singleton_accuracy", "empty_rate", "worst_class_coverage")   # columns 0 .. 5
CLASS_METRICS = ("per_class_coverage", "qhat")                                               # columns 6 .. 6 + C and 6 + C .. 6 + 2 C
COUNTS = ("n_test", "covered", "total_size", "empty", "singleton", "singleton_correct")     # counts 0 .. 5
_U64 = 2 ** 64 - 1


def cal_counts(labels, num_classes, n_cal):
    """int64 [C]: the calibration rows a stratified split takes of every class: floor(n_cal n_c / N) each, and one more for the
    n_cal - sum classes with the largest remainder n_cal n_c mod N, a tie going to the lower class (host; labels a numpy array)"""
    n = np.bincount(labels, minlength=num_classes).astype(np.int64)
    N = int(n.sum())
    base, rem = (n_cal * n) // N, (n_cal * n) % N
    extra = n_cal - int(base.sum())
    first = np.lexsort((np.arange(num_classes), -rem))[:extra]
    base[first] += 1
    return base


def _by_metric(table, C):
    """a [6 + 2 C, ...] array -> {name: ...}"""
    out = {m: table[k] for k, m in enumerate(METRICS)}
    out[CLASS_METRICS[0]] = np.moveaxis(table[6:6 + C], 0, -1)
    out[CLASS_METRICS[1]] = np.moveaxis(table[6 + C:6 + 2 * C], 0, -1)
    return out


def _scalars(d):
    return {m: (float(v) if np.ndim(v) == 0 else np.ascontiguousarray(v)) for m, v in d.items()}


def metrics_from_counts(counts, qhat):
    """float64 [6 + 2 C]: the metric columns of mmskin_conformal_finalize from one replicate's integers"""
    C = len(qhat)
    n, cov, total, empty, single, single_hit = (int(v) for v in counts[:6])
    rows, hit = counts[8 + 2 * C:8 + 3 * C], counts[8 + 3 * C:8 + 4 * C]
    out = np.full(6 + 2 * C, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[6:6 + C] = np.where(rows > 0, hit / rows, np.nan)
    out[6 + C:] = qhat
    if n > 0:
        out[:5] = cov / n, total / n, single / n, (single_hit / single if single else np.nan), empty / n
        out[5] = np.nanmin(out[6:6 + C])
    return out


class ConformalReport:
    """What `ConformalPredictor.study` returns, all on the host.  `point`: the metrics of replicate 0 (the identity-order split),
    keyed by METRICS (floats), "per_class_coverage" and "qhat" (float64 [C]).  `summary`: {"n_valid", "mean", "std", "low", "high"}
    -> the same keys, over the replicates.  `replicates`: the raw integers, {name: int64 [R]} for COUNTS and "set_size_histogram",
    "size_covered" [R, C + 1], "class_rows", "class_covered", "class_in" [R, C] (`counts`: the same as one int64 [R, 8 + 5 C] table in
    the layout of mmskin.h); `qhat` float64 [R, C].  Pooled over the replicates:
    `set_size_histogram` int64 [C + 1], `class_coverage` float64 [C], `size_stratified_coverage` dict(covered, total int64 [C + 1],
    coverage float64 [C + 1], NaN where no set has that size)."""

    def __init__(self, counts, qhat, summary, options):
        R, C = qhat.shape
        self.num_classes, self.options, self.qhat, self.counts = C, dict(options), qhat, counts
        at = 6
        self.replicates = {name: counts[:, k].copy() for k, name in enumerate(COUNTS)}
        for name, width in (("set_size_histogram", C + 1), ("size_covered", C + 1), ("class_rows", C), ("class_covered", C), ("class_in", C)):
            self.replicates[name] = counts[:, at:at + width].copy()
            at += width
        self.point = _scalars(_by_metric(metrics_from_counts(counts[0], qhat[0]), C))
        self.summary = {name: _scalars(_by_metric(summary[k], C)) for k, name in enumerate(ops.BOOTSTRAP_SUMMARY)}
        rep = self.replicates
        self.set_size_histogram = rep["set_size_histogram"].sum(axis=0)
        covered, rows = rep["size_covered"].sum(axis=0), rep["class_rows"].sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.class_coverage = np.where(rows > 0, rep["class_covered"].sum(axis=0) / rows, np.nan)
            self.size_stratified_coverage = {"covered": covered, "total": self.set_size_histogram,
                                             "coverage": np.where(self.set_size_histogram > 0, covered / self.set_size_histogram, np.nan)}

    def to_dict(self):
        """plain lists and floats, for json"""
        plain = lambda v: v.tolist() if isinstance(v, np.ndarray) else ({k: plain(x) for k, x in v.items()} if isinstance(v, dict) else v)
        return {"options": plain(self.options), "num_classes": self.num_classes, "point": plain(self.point), "summary": plain(self.summary),
                "set_size_histogram": plain(self.set_size_histogram), "class_coverage": plain(self.class_coverage),
                "size_stratified_coverage": plain(self.size_stratified_coverage), "replicates": plain(self.replicates),
                "qhat": plain(self.qhat)}

    def save(self, path):
        """the report as json (NaN and Infinity as Python writes them)"""
        with open(path, "w") as f:
            json.dump(self.to_dict(), f)


def _checked_probs(what, probs):
    p = torch.as_tensor(probs)
    if p.dim() != 2 or p.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: probs must be an fp32 or fp64 [N, C] array, got {p.dtype} {tuple(p.shape)}")
    if not 2 <= p.shape[1] <= MAX_CLASSES:
        raise MMSkinError(f"{what}: num_classes = {p.shape[1]}; a set is one 64-bit mask, which holds 2 .. CONFORMAL_MAX_CLASSES = {MAX_CLASSES}")
    if bool(torch.isnan(p).any()):
        raise ValueError(f"{what}: probs hold a NaN")
    if bool(((p < 0) | (p > 1)).any()):
        raise ValueError(f"{what}: a probability lies outside [0, 1]")
    return p


def _checked_fold(what, probs, labels):
    """(probs [N, C], labels int64 [N]) on one device, the rows whose label lies outside [0, C) dropped"""
    p = _checked_probs(what, probs)
    y = torch.as_tensor(labels)
    if tuple(y.shape) != (p.shape[0],) or y.dtype.is_floating_point or y.dtype == torch.bool or y.dtype.is_complex:
        raise ValueError(f"{what}: labels must be an integer {(p.shape[0],)} array, got {y.dtype} {tuple(y.shape)}")
    if y.device != p.device:
        raise ValueError(f"{what}: probs and labels must live on one device")
    y = y.long()
    keep = (y >= 0) & (y < p.shape[1])
    if not bool(keep.all()):
        p, y = p[keep], y[keep]
    if not 1 <= p.shape[0] <= MAX_ROWS:
        raise MMSkinError(f"{what}: n_rows = {p.shape[0]}; a replicate's split lives in LDS, which holds 1 .. CONFORMAL_MAX_ROWS = {MAX_ROWS}")
    return p, y


def _device_of(what, t):
    if not torch.cuda.is_available():
        raise MMSkinError(f"{what} needs a HIP device; there is no CPU fallback")
    return t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())


class ConformalPredictor:
    def __init__(self, alpha=0.1, score="aps", randomized=True, lam=0.01, k_reg=1, mondrian=False):
        """alpha: the miscoverage, in (0, 1).  score: "lac", "aps" or "raps"; lam >= 0 and k_reg >= 0 are read by "raps" only.
        randomized: u from (seed, row) instead of u = 1 ("aps", "raps").  mondrian: one threshold per class."""
        self.alpha, self.lam, self.k_reg = float(alpha), float(lam), int(k_reg)
        if not 0.0 < self.alpha < 1.0:
            raise ValueError(f"ConformalPredictor: alpha must lie in (0, 1), got {alpha}")
        if score not in SCORES:
            raise ValueError(f"ConformalPredictor: score must be one of {SCORES}, got {score!r}")
        if not (0.0 <= self.lam < float("inf")):
            raise ValueError(f"ConformalPredictor: lam must be finite and >= 0, got {lam}")
        if self.k_reg < 0:
            raise ValueError(f"ConformalPredictor: k_reg must be >= 0, got {k_reg}")
        self.score, self.randomized, self.mondrian = score, bool(randomized), bool(mondrian)
        self.qhat_ = self.n_cal_ = self.seed_ = self.num_classes_ = None

    # ------------------------------------------------------------------------------------------------ the library calls
    def _score_args(self, seed, row0):
        return SCORES.index(self.score), int(self.randomized), self.lam, self.k_reg, int(seed) & _U64, int(row0)

    def _scored(self, p, y, seed, R):
        """(workspace, order, members, class_start) of a fold on the device: the scores class-major inside the workspace, the rows
        by ascending true-label score (mondrian: by class first), and the rows grouped by label.  Device sorts, once per call."""
        N, C = p.shape
        dev = p.device
        workspace = torch.empty(int(load().mmskin_conformal_workspace_bytes(N, C, R)), dtype=torch.uint8, device=dev)
        score = torch.empty((N, C), dtype=torch.float64, device=dev)
        call("mmskin_conformal_score", ptr(p), int(p.dtype == torch.float64), N, C, *self._score_args(seed, 0), ptr(score), None,
             ptr(workspace), stream())
        order = torch.sort(score.gather(1, y[:, None])[:, 0], stable=True).indices
        if self.mondrian:
            order = order[torch.sort(y[order], stable=True).indices]
        members = torch.sort(y, stable=True).indices
        class_start = torch.zeros(C + 1, dtype=torch.int64, device=dev)
        class_start[1:] = torch.cumsum(torch.bincount(y, minlength=C), dim=0)
        i32 = lambda t: t.to(torch.int32).contiguous()
        return workspace, i32(order), i32(members), i32(class_start)

    def scores(self, probs, seed=0, row_offset=0):
        """(score fp64 [N, C], rank uint8 [N, C]) on the device: the nonconformity of every class as if it were the label, and its
        rank in the row's descending order (1 = the largest probability; a tie goes to the lower class index)"""
        p = _checked_probs("ConformalPredictor.scores", probs)
        dev = _device_of("ConformalPredictor.scores", p)
        with torch.no_grad(), torch.cuda.device(dev):
            p = p.to(dev).contiguous()
            N, C = p.shape
            score = torch.empty((N, C), dtype=torch.float64, device=dev)
            rank = torch.empty((N, C), dtype=torch.uint8, device=dev)
            if N:
                call("mmskin_conformal_score", ptr(p), int(p.dtype == torch.float64), N, C, *self._score_args(seed, row_offset), ptr(score),
                     ptr(rank), None, stream())
        return score, rank

    # ------------------------------------------------------------------------------------------------ fit / predict
    def fit(self, probs, labels, seed=0):
        """The threshold(s) from a calibration fold, every row calibrating.  Sets `qhat_` (a float, or float64 [C] with mondrian),
        `n_cal_` and `seed_` (the seed of the rows' u).  Returns self."""
        p, y = _checked_fold("ConformalPredictor.fit", probs, labels)
        dev = _device_of("ConformalPredictor.fit", p)
        with torch.no_grad(), torch.cuda.device(dev):
            p, y = p.to(dev).contiguous(), y.to(dev).contiguous()
            N, C = p.shape
            workspace, order, _, class_start = self._scored(p, y, seed, 1)
            qhat = torch.empty(C, dtype=torch.float64, device=dev)
            call("mmskin_conformal_fit", N, C, self.alpha, MONDRIAN if self.mondrian else 0, ptr(y), ptr(order), ptr(class_start), ptr(workspace),
                 ptr(qhat), stream())
            q = qhat.cpu().numpy()
        self.qhat_ = q if self.mondrian else float(q[0])
        self.n_cal_, self.seed_, self.num_classes_ = int(N), int(seed), int(C)
        return self

    def predict_sets(self, probs, row_offset=0, seed=None):
        """(mask int64 [M], size int32 [M]) on the device: bit c of mask[i] (read as unsigned) says class c is in the set of row i.
        Row i draws the u of row `row_offset + i` under `seed` (None: the seed of `fit`), so the rows of a fold keep their u."""
        if self.qhat_ is None:
            raise ValueError("ConformalPredictor.predict_sets: call fit first")
        p = _checked_probs("ConformalPredictor.predict_sets", probs)
        if p.shape[1] != self.num_classes_:
            raise ValueError(f"ConformalPredictor.predict_sets: probs have {p.shape[1]} classes, fit saw {self.num_classes_}")
        if int(row_offset) < 0:
            raise ValueError(f"ConformalPredictor.predict_sets: row_offset must be >= 0, got {row_offset}")
        dev = _device_of("ConformalPredictor.predict_sets", p)
        with torch.no_grad(), torch.cuda.device(dev):
            p = p.to(dev).contiguous()
            M, C = p.shape
            qhat = torch.from_numpy(np.broadcast_to(np.asarray(self.qhat_, dtype=np.float64), (C,)).copy()).to(dev)
            mask = torch.empty(M, dtype=torch.int64, device=dev)
            size = torch.empty(M, dtype=torch.int32, device=dev)
            if M:
                call("mmskin_conformal_apply", ptr(p), int(p.dtype == torch.float64), M, C,
                     *self._score_args(self.seed_ if seed is None else seed, row_offset), ptr(qhat), ptr(mask), ptr(size), stream())
        return mask, size

    def predict_lists(self, probs, class_names=None, **where):
        """the sets on the host: per row the list of class indices (or of their names) in ascending class order"""
        mask = self.predict_sets(probs, **where)[0].cpu().numpy().view(np.uint64)
        name = (lambda c: c) if class_names is None else (lambda c: class_names[c])
        return [[name(c) for c in range(self.num_classes_) if (int(m) >> c) & 1] for m in mask]

    # ------------------------------------------------------------------------------------------------ the study
    def study(self, probs, labels, n_cal=None, n_resamples=2000, seed=0, confidence=0.95, stratified=False, replicates_per_call=None,
              temperature=None):
        """Coverage and set size over `n_resamples` random splits of the fold into n_cal calibration rows (default N // 2) and
        N - n_cal test rows; replicate 0 is the identity-order split.  stratified: every class keeps its share of the calibration
        rows (`cal_counts`).  replicates_per_call cuts the study into launches and changes no result.  temperature: a T > 0 or a
        fitted TemperatureScaling; the fp32 rows are rescaled by its `apply` before they are scored.  Returns a ConformalReport."""
        what = "ConformalPredictor.study"
        if temperature is not None:
            scaling = temperature
            if not isinstance(temperature, TemperatureScaling):
                scaling = TemperatureScaling()
                scaling.beta = 1.0 / float(temperature)
                if not 0.0 < scaling.beta < float("inf"):
                    raise ValueError(f"{what}: temperature must be finite and positive, got {temperature}")
            probs = scaling.apply(probs, from_logits=False)
        p, y = _checked_fold(what, probs, labels)
        N, C = p.shape
        R, confidence = int(n_resamples), float(confidence)
        n_cal = N // 2 if n_cal is None else int(n_cal)
        if not 1 <= n_cal <= N - 1:
            raise ValueError(f"{what}: n_cal must leave a calibration and a test row: 1 .. {N - 1}, got {n_cal}")
        ops.bootstrap_check_limits(what, B=R)
        if not 0.0 < confidence < 1.0:
            raise ValueError(f"{what}: confidence must lie in (0, 1), got {confidence}")
        if replicates_per_call is not None and int(replicates_per_call) < 1:
            raise ValueError(f"{what}: replicates_per_call must be >= 1, got {replicates_per_call}")
        dev = _device_of(what, p)
        flags = (STRATIFIED if stratified else 0) | (MONDRIAN if self.mondrian else 0)
        with torch.no_grad(), torch.cuda.device(dev):
            p, y = p.to(dev).contiguous(), y.to(dev).contiguous()
            workspace, order, members, class_start = self._scored(p, y, seed, R)
            take = torch.from_numpy(cal_counts(y.cpu().numpy(), C, n_cal).astype(np.int32)).to(dev) if stratified else None
            qhat = torch.empty((R, C), dtype=torch.float64, device=dev)
            counts = torch.empty((R, 8 + 5 * C), dtype=torch.int64, device=dev)
            step = int(replicates_per_call) if replicates_per_call else R
            for r0 in range(0, R, step):
                call("mmskin_conformal_study", int(seed) & _U64, N, C, R, n_cal, self.alpha, flags, ptr(y), ptr(order), ptr(members),
                     ptr(class_start), ptr(take), r0, min(r0 + step, R), ptr(workspace), ptr(qhat), ptr(counts), stream())
            summary = torch.empty((5, 6 + 2 * C), dtype=torch.float64, device=dev)
            q_lo, q_hi = ops.bootstrap_quantiles(confidence)
            call("mmskin_conformal_finalize", ptr(counts), ptr(qhat), N, C, R, q_lo, q_hi, ptr(workspace), ptr(summary), stream())
            options = dict(alpha=self.alpha, score=self.score, randomized=self.randomized, lam=self.lam, k_reg=self.k_reg,
                           mondrian=self.mondrian, stratified=bool(stratified), n_rows=int(N), n_cal=n_cal, n_resamples=R, seed=int(seed),
                           confidence=confidence)
            return ConformalReport(counts.cpu().numpy(), qhat.cpu().numpy(), summary.cpu().numpy(), options)

    def from_fold_dir(self, path, **study):
        """`study` on the probabilities.npy and labels.npy that evaluate_model wrote into `path`"""
        return self.study(*read_fold_dir(path), **study)
