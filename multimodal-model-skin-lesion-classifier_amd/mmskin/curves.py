"""One-vs-rest ROC and precision-recall curves of a fold, with their operating points, without leaving the GPU: what the reference
draws per class with sklearn.metrics.roc_curve on the saved probabilities (utils/save_model_and_metrics.py:104-150).

    fc = FoldCurves.from_probs(probs, labels, specificities=(0.8, 0.9, 0.95), sensitivities=(0.8, 0.9, 0.95))
    fc = FoldCurves.from_fold_dir(folder)                    # probabilities.npy / labels.npy of evaluate_model
    fpr, tpr, thresholds = fc.roc(c)                         # == sklearn roc_curve(labels == c, probs[:, c], drop_intermediate=False)
    precision, recall, thresholds = fc.precision_recall(c)   # == sklearn precision_recall_curve(labels == c, probs[:, c])
    fc.auc, fc.average_precision                             # float64 [C]
    fc.youden, fc.sens_at_spec, fc.spec_at_sens              # dicts of arrays: value, threshold, index
    fc.tp, fc.fp, fc.thr, fc.n_points, fc.pos, fc.neg        # the raw arrays (host)
    fc.save(folder)                                          # curves.npz: what a plotting script needs

Per class c the stored curve is the list of the distinct scores of column c in descending order (thr[c, :n_points[c]]) with the
true and the false positives at each threshold (tp, fp: exact integers); the ROC start (0, 0) at threshold +inf and the
precision-recall end (1, 0) are added by the accessors.  The definitions, the tie rules of the operating points and the layout of
the summary are in include/mmskin.h and DESIGN.md section 25.  auc[c] is the trapezoid area as an integer over 2 pos neg and
equals evaluate.per_class_auc bit for bit.  Device tensors take csrc/curves.hip (N^2 C compares, no sort); CPU tensors and numpy
arrays take a numpy path that gives the same integers by sorting.  Rows whose label lies outside [0, C) are dropped; a NaN among
the remaining scores is a ValueError.  A class without a positive or without a negative row keeps its integers, its summary
values are NaN and its indices -1.  Plots stay out of scope.
"""
import os

import numpy as np
import torch

from . import ops
from ._lib import MMSkinError  # noqa: F401  (the limit errors raised through ops.curves_check_limits)

FILE_NAME = "curves.npz"


# ------------------------------------------------------------------------------------------------ the host path
def host_curves(probs, labels):
    """the integers of mmskin_ovr_curves in numpy, by one stable sort per class: (thr fp32 [C, N], tp int32 [C, N], fp int32 [C, N],
    n_points int32 [C], counts int64 [2 C + 1] = pos, neg, nan)"""
    N, C = probs.shape
    valid = (labels >= 0) & (labels < C)
    p, y = probs[valid], labels[valid]
    pos = np.bincount(y, minlength=C).astype(np.int64)
    neg = int(valid.sum()) - pos
    thr = np.zeros((C, N), dtype=np.float32)
    tp, fp = np.zeros((C, N), dtype=np.int32), np.zeros((C, N), dtype=np.int32)
    n_points = np.zeros(C, dtype=np.int32)
    for c in range(C):
        keep = ~np.isnan(p[:, c])                                    # a NaN is neither greater nor equal: no threshold, in no count
        s, own = p[keep, c], y[keep] == c
        order = np.argsort(-s, kind="stable")                        # descending; equal scores keep their row order
        s, own = s[order], own[order]
        if not len(s):
            continue
        first = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))   # where a tie group starts: its lowest row
        last = np.concatenate([first[1:], [len(s)]]) - 1
        n = len(first)
        n_points[c], thr[c, :n] = n, s[first]
        tp[c, :n] = np.cumsum(own)[last]
        fp[c, :n] = np.cumsum(~own)[last]
    return thr, tp, fp, n_points, np.concatenate([pos, neg, [int(np.isnan(p).sum())]]).astype(np.int64)


def host_summary(thr, tp, fp, n_points, counts, specificities, sensitivities):
    """float64 [C, 5 + 3 (A + B)]: the columns of mmskin_ovr_curves_summary from the integers, with the same decisions"""
    C = len(n_points)
    A, B = len(specificities), len(sensitivities)
    out = np.full((C, 5 + 3 * (A + B)), np.nan)
    for c in range(C):
        pos, neg = int(counts[c]), int(counts[C + c])
        if pos == 0 or neg == 0:
            continue
        n = int(n_points[c])
        t, f = tp[c, :n].astype(np.int64), fp[c, :n].astype(np.int64)
        t_prev, f_prev = np.concatenate([[0], t[:-1]]), np.concatenate([[0], f[:-1]])
        dpos, dneg = np.float64(pos), np.float64(neg)
        out[c, 0] = np.float64(int(((f - f_prev) * (t + t_prev)).sum())) / (2.0 * dpos * dneg)
        out[c, 1] = float((((t - t_prev) / dpos) * (t / np.maximum(t + f, 1).astype(np.float64))).sum())
        if n:
            j = t * neg - f * pos                                    # Youden's J over pos neg, exact: below 2^62
            k = int(np.argmax(j))                                    # the first maximum
            out[c, 2:5] = np.float64(int(j[k])) / (dpos * dneg), thr[c, k], k
        for a, q in enumerate(specificities):
            ok = (neg - f).astype(np.float64) >= np.float64(q) * dneg
            cell = out[c, 5 + 3 * a:8 + 3 * a]
            if ok.any():
                k = int(np.flatnonzero(ok & (t == t[ok].max()))[0])
                cell[:] = t[k] / dpos, thr[c, k], k
            else:
                cell[:] = 0.0, np.inf, -1
        for b, s in enumerate(sensitivities):
            ok = t.astype(np.float64) >= np.float64(s) * dpos
            cell = out[c, 5 + 3 * (A + b):8 + 3 * (A + b)]
            if ok.any():
                k = int(np.flatnonzero(ok & (f == f[ok].min()))[0])
                cell[:] = (neg - f[k]) / dneg, thr[c, k], k
            else:
                cell[:] = np.nan, np.nan, -1
    return out


# ------------------------------------------------------------------------------------------------ the public class
def _requests(what, name, values):
    v = np.asarray(values, dtype=np.float64)
    if v.ndim != 1 or not np.isfinite(v).all() or ((v < 0) | (v > 1)).any():
        raise ValueError(f"{what}: {name} must be a sequence of numbers in [0, 1], got {values!r}")
    return v


def _index(col):
    return np.where(np.isnan(col), -1, col).astype(np.int64)


class FoldCurves:
    """The curves of one fold, all on the host.  thr fp32 [C, N], tp / fp int32 [C, N] (slots at and past n_points[c] are zero),
    n_points int32 [C], pos / neg int64 [C]; auc, average_precision float64 [C]; youden = dict(value [C], threshold [C], index
    [C]); sens_at_spec / spec_at_sens = dict(value, threshold, index), each [C, len(request)], for the requested `specificities`
    / `sensitivities`.  An index points into the stored arrays of its class; -1 is the (0, 0) start of the ROC (threshold +inf)
    or an undefined class."""

    def __init__(self, thr, tp, fp, n_points, pos, neg, summary, specificities, sensitivities):
        self.thr, self.tp, self.fp, self.n_points, self.pos, self.neg = thr, tp, fp, n_points, pos, neg
        self.num_classes = len(n_points)
        self.specificities, self.sensitivities = specificities, sensitivities
        A, B = len(specificities), len(sensitivities)
        self.auc, self.average_precision = summary[:, 0].copy(), summary[:, 1].copy()
        self.youden = {"value": summary[:, 2].copy(), "threshold": summary[:, 3].copy(), "index": _index(summary[:, 4])}
        block = lambda lo, n: {"value": summary[:, lo:lo + 3 * n:3].copy(), "threshold": summary[:, lo + 1:lo + 3 * n:3].copy(),
                               "index": _index(summary[:, lo + 2:lo + 3 * n:3])}
        self.sens_at_spec, self.spec_at_sens = block(5, A), block(5 + 3 * A, B)

    @classmethod
    def from_probs(cls, probs, labels, specificities=(0.8, 0.9, 0.95), sensitivities=(0.8, 0.9, 0.95)):
        """probs fp32 [N, C], labels integer [N]: numpy arrays or tensors, on the host or on one device"""
        what = "FoldCurves.from_probs"
        s, y = torch.as_tensor(probs), torch.as_tensor(labels)
        if s.dim() != 2 or s.dtype != torch.float32:
            raise ValueError(f"{what}: probs must be an fp32 [N, C] array, got {s.dtype} {tuple(s.shape)}")
        N, C = s.shape
        if tuple(y.shape) != (N,) or y.dtype.is_floating_point or y.dtype == torch.bool or y.dtype.is_complex:
            raise ValueError(f"{what}: labels must be an integer [N] = {(N,)} array, got {y.dtype} {tuple(y.shape)}")
        if y.device != s.device:
            raise ValueError(f"{what}: probs live on {s.device}, labels on {y.device}")
        spec, sens = _requests(what, "specificities", specificities), _requests(what, "sensitivities", sensitivities)
        ops.curves_check_limits(what, N=N, C=C, n_spec=len(spec), n_sens=len(sens))
        s, y = s.detach().contiguous(), y.detach().long().contiguous()
        if s.is_cuda:
            with torch.no_grad(), torch.cuda.device(s.device):
                raw = ops.ovr_curves(s, y)
                summary = ops.ovr_curves_summary(raw, spec, sens).cpu().numpy()
                thr, tp, fp, n_points, counts = (t.cpu().numpy() for t in raw)
        else:
            thr, tp, fp, n_points, counts = host_curves(s.numpy(), y.numpy())
            summary = None
        if counts[2 * C] > 0:
            raise ValueError(f"{what}: the probabilities of the rows that count hold {int(counts[2 * C])} NaN")
        if summary is None:
            summary = host_summary(thr, tp, fp, n_points, counts, spec, sens)
        return cls(thr, tp, fp, n_points, counts[:C].copy(), counts[C:2 * C].copy(), summary, spec, sens)

    @classmethod
    def from_fold_dir(cls, path, **requests):
        """`from_probs` on the probabilities.npy and labels.npy that evaluate_model wrote into `path`"""
        load = lambda name: np.load(os.path.join(path, name))
        return cls.from_probs(load("probabilities.npy").astype(np.float32, copy=False), load("labels.npy"), **requests)

    def _class(self, c):
        c = int(c)
        if not 0 <= c < self.num_classes:
            raise ValueError(f"FoldCurves: class {c} is outside 0 .. {self.num_classes - 1}")
        n = int(self.n_points[c])
        return c, self.tp[c, :n].astype(np.float64), self.fp[c, :n].astype(np.float64), self.thr[c, :n]

    def roc(self, c):
        """(fpr, tpr, thresholds) of class c against the rest, from (0, 0) at threshold +inf: sklearn's roc_curve with
        drop_intermediate=False.  A class without negatives (positives) has NaN in fpr (tpr)."""
        c, tp, fp, thr = self._class(c)
        with np.errstate(invalid="ignore", divide="ignore"):
            fpr, tpr = fp / np.float64(self.neg[c]), tp / np.float64(self.pos[c])
        return np.concatenate([[0.0], fpr]), np.concatenate([[0.0], tpr]), np.concatenate([np.array([np.inf], dtype=thr.dtype), thr])

    def precision_recall(self, c):
        """(precision, recall, thresholds) of class c against the rest, thresholds ascending, ending in (1, 0): sklearn's
        precision_recall_curve.  A class without positives has NaN in recall."""
        c, tp, fp, thr = self._class(c)
        with np.errstate(invalid="ignore", divide="ignore"):
            precision, recall = tp / (tp + fp), tp / np.float64(self.pos[c])
        return np.concatenate([precision[::-1], [1.0]]), np.concatenate([recall[::-1], [0.0]]), thr[::-1].copy()

    def save(self, folder):
        """curves.npz in `folder`: the raw arrays and every summary value -> the path written"""
        path = os.path.join(folder, FILE_NAME)
        arrays = dict(thr=self.thr, tp=self.tp, fp=self.fp, n_points=self.n_points, pos=self.pos, neg=self.neg, auc=self.auc,
                      average_precision=self.average_precision, specificities=self.specificities, sensitivities=self.sensitivities)
        for name, group in (("youden", self.youden), ("sens_at_spec", self.sens_at_spec), ("spec_at_sens", self.spec_at_sens)):
            arrays.update({f"{name}_{k}": v for k, v in group.items()})
        np.savez(path, **arrays)
        return path
