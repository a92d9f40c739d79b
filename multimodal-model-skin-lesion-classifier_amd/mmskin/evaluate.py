"""Evaluation of a fold in one forward pass: the reference's utils/model_metrics.py with nothing read back between batches.

    ovr_auc_counts(probs, labels)                  pos / neg / wins2 per class and the NaN count, exact integers
    auc_from_counts(counts, num_classes)           the `auc` of the reference's metrics dict from those integers
    per_class_auc(counts)                          wins2 / (2 pos neg), NaN where a class has no positive or no negative row
    evaluate_model(model, dataloader, targets, device, fold_num, base_dir, model_name="None")
                                                   drop-in for utils/model_metrics.py:15-134; curves=True adds the fold's ROC and
                                                   precision-recall curves (mmskin.curves.FoldCurves)

wins2[c] sums, over the pairs (row i with label c, row j with another label), 2 [p[i, c] > p[j, c]] + [p[i, c] == p[j, c]], so
auc[c] = wins2[c] / (2 pos[c] neg[c]) is the Mann-Whitney statistic: what sklearn's roc_auc_score computes by trapezoids, ties at
half weight.  On a HIP device the integers come from one launch of csrc/auc.hip (mmskin_ovr_auc_counts, N^2 compares); CPU
tensors take a numpy path that gives the same integers by sorting.  Rows whose label lies outside [0, C) count nowhere, as in
EpochMeter.  Under data parallelism the counts are NOT additive across ranks (a pair may straddle two ranks): gather the
probabilities and labels first.

    metrics, labels, preds, probs = evaluate_model(model, val_loader, targets, device, fold, out_dir, "resnet-50")
    metrics, labels, preds, probs, names = evaluate_model(..., extras=True, image_names=True)   # + loss, confusion, per_class_auc
"""
import os

import numpy as np
import torch

from ._lib import MMSkinError, call, ptr, stream
from .criterion import EpochMeter, metrics_from_confusion

MAX_CLASSES = 1024                                       # the kernel's and the meter's range
MAX_ROWS = 2 ** 31 - 1


def _host_counts(probs, labels):
    """the kernel's integers in numpy: per class, the negatives' scores sorted once, the positives placed by searchsorted"""
    N, C = probs.shape
    valid = (labels >= 0) & (labels < C)
    p, y = probs[valid], labels[valid]
    pos = np.bincount(y, minlength=C).astype(np.int64)
    neg = int(valid.sum()) - pos
    wins2 = np.zeros(C, dtype=np.int64)
    for c in range(C):
        keep = ~np.isnan(p[:, c])                                    # a NaN is neither greater nor equal: it wins and loses nothing
        col, own = p[keep, c], y[keep] == c
        positives, negatives = col[own], np.sort(col[~own])
        if len(positives) and len(negatives):
            below, not_above = np.searchsorted(negatives, positives, side="left"), np.searchsorted(negatives, positives, side="right")
            wins2[c] = int(below.sum()) + int(not_above.sum())       # 2 below + ties = below + (below + ties)
    return {"pos": pos, "neg": neg, "wins2": wins2, "nan": int(np.isnan(p).sum())}


def ovr_auc_counts(probs, labels):
    """probs fp32 [N, C] contiguous, labels integer [N], on one device -> dict(pos int64 [C], neg int64 [C], wins2 int64 [C],
    nan int) on the host.  2 <= C <= 1024, 1 <= N < 2^31 (MMSkinError otherwise, on either path)."""
    if probs.dim() != 2 or probs.dtype != torch.float32:
        raise ValueError(f"ovr_auc_counts: probs must be an fp32 [N, C] tensor, got {probs.dtype} {tuple(probs.shape)}")
    N, C = probs.shape
    if tuple(labels.shape) != (N,) or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f"ovr_auc_counts: labels must be an integer [N] = {(N,)} tensor, got {labels.dtype} {tuple(labels.shape)}")
    if labels.device != probs.device:
        raise ValueError(f"ovr_auc_counts: probs live on {probs.device}, labels on {labels.device}")
    if not probs.is_contiguous():
        raise MMSkinError(f"ovr_auc_counts: probs must be contiguous, got strides {probs.stride()} for shape {tuple(probs.shape)}")
    if not probs.is_cuda:
        if not (2 <= C <= MAX_CLASSES and 1 <= N <= MAX_ROWS):
            raise MMSkinError(f"ovr_auc_counts: [N, C] = {(N, C)} is outside 1 <= N < 2^31, 2 <= C <= {MAX_CLASSES}")
        return _host_counts(probs.detach().numpy(), labels.detach().long().numpy())
    labels = labels.detach().long().contiguous()                     # int64 labels as torch hands them over: no copy
    block = torch.empty(3 * C + 1, dtype=torch.int64, device=probs.device)
    call("mmskin_ovr_auc_counts", ptr(probs.detach()), ptr(labels), N, C, ptr(block), stream())
    host = block.cpu().numpy()
    return {"pos": host[:C].copy(), "neg": host[C:2 * C].copy(), "wins2": host[2 * C:3 * C].copy(), "nan": int(host[3 * C])}


def per_class_auc(counts):
    """float64 [C]: wins2 / (2 pos neg); NaN for a class without a positive or without a negative row"""
    pos, neg, wins2 = (np.asarray(counts[k], dtype=np.float64) for k in ("pos", "neg", "wins2"))
    pairs = 2.0 * pos * neg
    return np.divide(wins2, pairs, out=np.full(pos.shape, np.nan), where=pairs > 0)


def auc_from_counts(counts, num_classes):
    """The `auc` entry of utils/model_metrics.py:106-119.  Two classes: roc_auc_score(labels, probs[:, 1]), the AUC of class 1.
    More: roc_auc_score(one-hot labels, probs, average="weighted", multi_class="ovr"), the mean of the per-class AUCs weighted by
    pos[c] over the classes that have a positive and a negative row.  NaN when no class has both (what scikit-learn 1.7 returns
    there); None when a counted probability is NaN (roc_auc_score raises, the reference's `except` yields None)."""
    if len(counts["pos"]) != num_classes:
        raise ValueError(f"auc_from_counts: counts hold {len(counts['pos'])} classes, num_classes is {num_classes}")
    if counts["nan"] > 0:
        return None
    auc = per_class_auc(counts)
    if num_classes == 2:
        return float(auc[1])
    ok = ~np.isnan(auc)
    if not ok.any():
        return float("nan")
    weight = np.asarray(counts["pos"], dtype=np.float64)[ok]
    return float((auc[ok] * weight).sum() / weight.sum())


def _dataset_rows(dataloader):
    try:
        return len(dataloader.dataset)
    except (AttributeError, TypeError):
        return None


def evaluate_model(model, dataloader, targets, device, fold_num: int, base_dir: str, model_name: str = "None", *, extras=False,
                   image_names=False, curves=False):
    """utils/model_metrics.py:15-134 in one forward pass -> (metrics, all_labels [N], all_preds [N], all_probs [N, C]) as numpy
    arrays, with labels.npy / predictions.npy / probabilities.npy / targets.npy written to base_dir/{model_name}_fold_{fold_num}.

    The loader yields (image_names, images, metadata, labels).  Per batch the logits go through EpochMeter.update (confusion
    matrix, loss and soft-max rows in one launch) and the labels into an [N] device buffer; after the last batch one AUC launch
    and one arg-max follow, then the host copies.  The buffers are sized from len(dataloader.dataset) where that exists (fewer
    rows may arrive, e.g. under drop_last; more is an error), otherwise the per-batch device tensors are kept and concatenated.
    A model on the CPU takes the host paths of the meter and of ovr_auc_counts.

    metrics: fold, accuracy, balanced_accuracy, precision, recall, f1_score, auc -- the discrete ones from the meter's
    confusion matrix (metrics_from_confusion), auc from auc_from_counts.  The confusion matrix takes the first arg-max of the
    LOGITS, the returned predictions the arg-max of the probabilities: they differ only where two logits round to one
    probability.  Labels outside [0, C) count in no metric (sklearn would count them as errors).
    extras=True adds loss (mean cross-entropy), confusion [C, C] and per_class_auc [C] to metrics; image_names=True appends the
    names in loader order to the returned tuple, which is all save_predictions.py needs to write predictions_eval_fold_N.csv.
    curves=True adds metrics["curves"], the mmskin.curves.FoldCurves of the fold (one-vs-rest ROC and precision-recall curves
    with their operating points) built from the device buffers before they are copied, and writes curves.npz beside the .npy
    files; where the probabilities hold a NaN it is None and nothing is written, as for `auc`."""
    folder_path = os.path.join(base_dir, f"{model_name}_fold_{fold_num}")
    os.makedirs(folder_path, exist_ok=True)
    model.eval()
    expected = _dataset_rows(dataloader)
    meter = probs_buf = labels_buf = None
    prob_chunks, label_chunks, names, row = [], [], [], 0
    with torch.no_grad():
        for batch_names, images, metadata, labels in dataloader:
            images = images.to(device, non_blocking=True)
            metadata = metadata.to(device, non_blocking=True)
            labels = labels.to(device, non_blocking=True)
            logits = model(images, metadata)                         # [B, C]
            B = logits.shape[0]
            if meter is None:
                meter = EpochMeter(logits.shape[1], logits.device)
                if expected is not None:
                    probs_buf = meter.probs(expected)
                    labels_buf = torch.empty(expected, dtype=torch.int64, device=logits.device)
            labels = labels.to(logits.device)
            if probs_buf is None:
                prob_chunks.append(meter.probs(B))                   # a fresh [B, C] buffer that this update fills
                label_chunks.append(labels.long())
            elif row + B > expected:
                raise ValueError(f"evaluate_model: the loader yielded more than the len(dataloader.dataset) = {expected} rows")
            else:
                labels_buf[row:row + B].copy_(labels)
            meter.update(logits, labels)
            row += B
            if image_names:
                names.extend(batch_names)
    if meter is None:
        raise ValueError("evaluate_model: the dataloader yielded no batch")
    probs = probs_buf[:row] if probs_buf is not None else torch.cat(prob_chunks)
    labels = labels_buf[:row] if labels_buf is not None else torch.cat(label_chunks)
    num_classes = meter.num_classes
    counts = ovr_auc_counts(probs, labels)
    fold_curves = None
    if curves and counts["nan"] == 0:
        from .curves import FoldCurves
        fold_curves = FoldCurves.from_probs(probs, labels)
    preds = probs.argmax(dim=1)
    summary = meter.compute()
    all_labels, all_preds, all_probs = labels.cpu().numpy(), preds.cpu().numpy(), probs.cpu().numpy()

    targets = np.arange(num_classes) if targets is None else np.array(targets)[:num_classes]
    np.save(os.path.join(folder_path, "labels.npy"), all_labels)
    np.save(os.path.join(folder_path, "predictions.npy"), all_preds)
    np.save(os.path.join(folder_path, "probabilities.npy"), all_probs)
    np.save(os.path.join(folder_path, "targets.npy"), targets)

    metrics = {"fold": fold_num}
    metrics.update(metrics_from_confusion(summary["confusion"]))
    metrics["auc"] = auc_from_counts(counts, num_classes)
    if metrics["auc"] is None:
        print("[WARN] AUC computation failed: the probabilities contain NaN")
    if extras:
        metrics.update(loss=summary["loss"], confusion=summary["confusion"], per_class_auc=per_class_auc(counts))
    if curves:
        metrics["curves"] = fold_curves
        if fold_curves is not None:
            fold_curves.save(folder_path)
    out = (metrics, all_labels, all_preds, all_probs)
    return out + (names,) if image_names else out
