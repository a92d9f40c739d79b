"""The criterion of the training step on the HIP path, and the epoch meter that rides on its forward launch.

    CrossEntropyLoss(weight=None, reduction='mean')        torch's nn.CrossEntropyLoss (train_pad_20.py:52)
    FocalLoss(alpha=None, gamma=2, reduction='mean')       the reference's models/focalLoss.py
    SoftTargetCrossEntropy(weight=None)                    the reference's models/softtargetsCrossEntropy.py
    EpochMeter(num_classes, device)                        loss, accuracy, ... of an epoch with ONE device-to-host copy

On a HIP device each criterion is one forward and one backward launch of csrc/criterion.hip (mmskin_criterion_forward /
_backward: the formulas, the ignored-label rule and the fixed reduction order are stated in include/mmskin.h).  The loss is
fp32, also for bf16 logits; dlogits has the logits' dtype.  CPU tensors take the same formulas through torch ops and autograd
(host_loss below), so a device="cpu" loop computes what the reference's criterion computes.

    criterion = FocalLoss(alpha=class_weights, gamma=2)
    criterion.meter = meter = EpochMeter(num_classes, device)     # instead of running_loss += loss.item() per step
    for image, metadata, label in loader:
        criterion(model(image, metadata), label).backward()
    print(meter.compute()["loss"])                                  # the epoch's only host read

    meter.reset(); probs = meter.probs(len(val_set))                # evaluation without a .cpu() per batch
    with torch.no_grad():
        for image, metadata, label in val_loader:
            meter.update(model(image, metadata), label)
    metrics = meter.compute()                                       # with the AUC and the .npy files: mmskin.evaluate.evaluate_model
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._autograd import no_second_order
from ._lib import call, ptr, stream

CE, FOCAL, SOFT = 0, 1, 2                               # MMSKIN_CRITERION_* in mmskin.h
REDUCTIONS = {"none": 0, "sum": 1, "mean": 2}           # MMSKIN_REDUCE_*

_tickets = {}


def _ticket(device):
    """the zeroed int32 that the forward kernel's last-workgroup election counts in and leaves zero: one per (device, stream),
    because calls that share it must be ordered"""
    key = (device.index, stream().value)
    t = _tickets.get(key)
    if t is None:
        t = _tickets[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return t


def _reduction_code(reduction):
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {sorted(REDUCTIONS)}, got {reduction!r}")
    return REDUCTIONS[reduction]


def _check_gamma(gamma):
    gamma = float(gamma)
    if not (gamma == 0.0 or gamma >= 1.0):
        raise ValueError(f"FocalLoss: gamma must be 0 or >= 1 (the derivative is unbounded at pt = 1 for 0 < gamma < 1), got {gamma}")
    return gamma


def _dtype_code(t):
    return _lib.BF16 if t.dtype == torch.bfloat16 else _lib.F32


def host_loss(logits, targets, weight, kind, reduction, gamma=0.0):
    """The three criteria in torch ops, differentiable by autograd: the CPU path of the modules below."""
    if kind == CE:
        return F.cross_entropy(logits, targets, weight=weight, reduction=reduction)
    if kind == SOFT:
        weighted = targets if weight is None else targets * weight
        return -(weighted * F.log_softmax(logits, dim=-1)).sum(dim=-1).mean()
    ce = F.cross_entropy(logits, targets, reduction="none")
    rows = ce if weight is None else weight[targets] * ce
    if gamma != 0:
        rows = (-torch.expm1(-ce)).pow(gamma) * rows
    return rows.mean() if reduction == "mean" else rows.sum() if reduction == "sum" else rows


def _device_forward(logits, targets, weight, kind, reduction, gamma, meter):
    """one launch: (loss fp32 [] or [B], the scratch buffer the backward reads)"""
    if logits.dim() != 2 or logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"criterion: logits must be an fp32 or bf16 [B, C] tensor, got {logits.dtype} {tuple(logits.shape)}")
    B, C = logits.shape
    if kind == SOFT:
        if tuple(targets.shape) != (B, C):
            raise ValueError(f"criterion: soft targets must be [B, C] = {(B, C)}, got {tuple(targets.shape)}")
    elif tuple(targets.shape) != (B,):
        raise ValueError(f"criterion: labels must be an integer [B] = {(B,)} tensor, got {targets.dtype} {tuple(targets.shape)}")
    if targets.device != logits.device or (weight is not None and tuple(weight.shape) != (C,)):
        raise ValueError(f"criterion: targets must live on {logits.device} and class weights must be [C] = {(C,)}")
    floats = _lib.load().mmskin_criterion_scratch_floats(B, C, kind)
    scratch = torch.empty(max(int(floats), 1), dtype=torch.float32, device=logits.device)
    loss = torch.empty((B,) if reduction == REDUCTIONS["none"] else (), dtype=torch.float32, device=logits.device)
    block = probs = None
    if meter is not None:
        block = meter._block_for(logits, C)
        if meter._probs is not None:
            probs = meter._next_probs(B)
    call("mmskin_criterion_forward", ptr(logits), _dtype_code(logits), ptr(targets), ptr(weight), kind, reduction, gamma, B, C, ptr(loss),
         ptr(scratch), ptr(_ticket(logits.device)), ptr(block), ptr(probs), stream())
    return loss, scratch


@no_second_order
class _Criterion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, weight, kind, reduction, gamma, meter):
        logits = logits.contiguous()
        if kind != SOFT and targets.dtype.is_floating_point:
            raise ValueError(f"criterion: labels must be integers, got {targets.dtype}")
        targets = (targets.float() if kind == SOFT else targets.long()).contiguous()     # int64 labels as torch hands them over: no copy
        loss, scratch = _device_forward(logits, targets, weight, kind, reduction, gamma, meter)
        ctx.save_for_backward(logits, targets, weight, scratch)
        ctx.args = (kind, reduction, gamma)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits, targets, weight, scratch = ctx.saved_tensors
        kind, reduction, gamma = ctx.args
        B, C = logits.shape
        g = g.float().contiguous()
        dlogits = torch.empty_like(logits)
        call("mmskin_criterion_backward", ptr(logits), _dtype_code(logits), ptr(targets), ptr(weight), kind, reduction, gamma, B, C, ptr(g),
             ptr(scratch), ptr(dlogits), stream())
        return dlogits, None, None, None, None, None, None


class _ClassWeighted(nn.Module):
    """Base of the three criteria: hands the class weights out as fp32 on the logits' device (moved once, then cached) and
    routes device tensors to the kernel, CPU tensors to host_loss.  `meter` is an EpochMeter or None."""

    meter = None

    def _weights_on(self, w, device):
        if w is None:
            return None
        if not isinstance(w, torch.Tensor):
            raise TypeError(f"{type(self).__name__}: class weights must be a tensor, got {type(w).__name__}")
        if w.device == device and w.dtype == torch.float32 and w.is_contiguous():
            return w.detach()
        key = (id(w), w._version, device)
        if getattr(self, "_moved_key", None) != key:
            self._moved_key, self._moved = key, w.detach().to(device=device, dtype=torch.float32).contiguous()
        return self._moved

    def _run(self, logits, targets, w, kind, reduction, gamma=0.0):
        code = _reduction_code(reduction)
        w = self._weights_on(w, logits.device)
        if logits.is_cuda:
            return _Criterion.apply(logits, targets, w, kind, code, gamma, self.meter)
        loss = host_loss(logits, targets, w, kind, reduction, gamma)
        if self.meter is not None:
            mean = loss if reduction == "mean" else host_loss(logits, targets, w, kind, "mean", gamma)
            self.meter._update_host(logits, None if kind == SOFT else targets, mean.detach())
        return loss


class CrossEntropyLoss(_ClassWeighted):
    """nn.CrossEntropyLoss(weight, reduction) on class-index targets.  On the HIP path EVERY label outside [0, C) is ignored, as
    torch ignores its ignore_index -100: labels are never inspected on the host."""

    def __init__(self, weight=None, reduction="mean"):
        super().__init__()
        _reduction_code(reduction)
        self.register_buffer("weight", weight)
        self.reduction = reduction

    def forward(self, input, target):
        return self._run(input, target, self.weight, CE, self.reduction)


class FocalLoss(_ClassWeighted):
    """(1 - pt)^gamma (alpha[y] ce) with pt = exp(-ce), the focal loss of the reference's models/focalLoss.py; gamma is 0 or
    >= 1.  As there, any reduction other than 'mean' and 'sum' returns the per-row values."""

    def __init__(self, alpha=None, gamma=2, reduction="mean"):
        super().__init__()
        _check_gamma(gamma)
        self.alpha = alpha
        self.gamma = gamma
        self.reduction = reduction

    def forward(self, inputs, targets):
        reduction = self.reduction if self.reduction in ("mean", "sum") else "none"
        return self._run(inputs, targets, self.alpha, FOCAL, reduction, _check_gamma(self.gamma))


class SoftTargetCrossEntropy(_ClassWeighted):
    """mean over the batch of -sum_c t[c] log_softmax(z)[c] w[c] (the reference's models/softtargetsCrossEntropy.py)."""

    def __init__(self, weight=None):
        super().__init__()
        self.weight = weight

    def forward(self, inputs, targets):
        return self._run(inputs, targets, self.weight, SOFT, "mean")


def metrics_from_confusion(confusion):
    """accuracy, balanced_accuracy, precision, recall, f1_score of a confusion matrix [true][predicted], as
    utils/model_metrics.py:91-101 gets them from sklearn: average="weighted" and zero_division=0, the binary variants
    (positive class 1) when there are two classes, and balanced_accuracy_score's mean recall over the classes that occur."""
    cm = np.asarray(confusion, dtype=np.float64)
    n = cm.sum()
    tp, true_n, pred_n = np.diag(cm), cm.sum(axis=1), cm.sum(axis=0)

    def ratio(a, b):                                     # zero_division=0
        return np.divide(a, b, out=np.zeros(a.shape, dtype=np.float64), where=b > 0)

    precision, recall, f1 = ratio(tp, pred_n), ratio(tp, true_n), ratio(2 * tp, true_n + pred_n)
    present = true_n > 0
    out = {"accuracy": float(tp.sum() / n) if n else float("nan"),
           "balanced_accuracy": float(recall[present].mean()) if present.any() else float("nan")}
    if cm.shape[0] == 2:
        pick = lambda v: float(v[1])
    else:
        pick = lambda v: float((v * true_n).sum() / n) if n else 0.0
    out.update(precision=pick(precision), recall=pick(recall), f1_score=pick(f1))
    return out


class EpochMeter:
    """Accumulates on the device, across forward launches, the loss sum, the row count and the confusion matrix of an epoch.

    Attach it to a criterion (criterion.meter = m) or call m.update(logits, labels) under torch.no_grad() (plain cross-entropy,
    forward only).  Rows whose label lies outside [0, C) count nowhere; soft targets feed the loss and the row count only.
    Nothing reaches the host before compute()."""

    HEADER = 16                                          # double loss_sum, int64 rows (mmskin.h); then int32 confusion[C][C]

    def __init__(self, num_classes, device):
        if not 2 <= int(num_classes) <= 1024:
            raise ValueError(f"EpochMeter: num_classes must be 2 .. 1024, got {num_classes}")
        self.num_classes = int(num_classes)
        self.block = torch.zeros(self.HEADER + 4 * self.num_classes ** 2, dtype=torch.uint8, device=torch.device(device))
        self._probs, self._row = None, 0

    def _block_for(self, logits, C):
        if C != self.num_classes or logits.device != self.block.device:
            raise ValueError(f"EpochMeter({self.num_classes}, {self.block.device}) was handed logits with {C} classes on {logits.device}")
        return self.block

    def probs(self, n):
        """-> a fresh fp32 [n, C] device buffer; the updates that follow fill its rows in order with softmax(logits)"""
        self._probs, self._row = torch.empty((int(n), self.num_classes), dtype=torch.float32, device=self.block.device), 0
        return self._probs

    def _next_probs(self, B):
        if self._row + B > self._probs.shape[0]:
            raise ValueError(f"EpochMeter.probs({self._probs.shape[0]}) is full: rows {self._row} .. {self._row + B} were asked for")
        view = self._probs[self._row:self._row + B]
        self._row += B
        return view

    def _update_host(self, logits, labels, mean_loss):
        """the same bookkeeping for CPU tensors, in torch and numpy"""
        with torch.no_grad():
            C, host = self.num_classes, self.block.numpy()
            self._block_for(logits, logits.shape[1])
            n = logits.shape[0]
            if labels is not None:
                valid = (labels >= 0) & (labels < C)
                cells = (labels[valid] * C + logits.float().argmax(dim=1)[valid]).numpy()
                host[self.HEADER:].view(np.int32)[:] += np.bincount(cells, minlength=C * C).astype(np.int32)
                n = int(valid.sum())
            if n:
                host[:8].view(np.float64)[0] += float(mean_loss) * n
                host[8:16].view(np.int64)[0] += n
            if self._probs is not None:
                self._next_probs(logits.shape[0]).copy_(torch.softmax(logits.float(), dim=1))

    def update(self, logits, labels):
        """forward-only cross-entropy of one batch into the accumulators -> the batch's mean loss (a scalar on the device)"""
        with torch.no_grad():
            if not logits.is_cuda:
                loss = host_loss(logits, labels, None, CE, "mean")
                self._update_host(logits, labels, loss)
                return loss
            return _Criterion.apply(logits, labels, None, CE, REDUCTIONS["mean"], 0.0, self)

    def reset(self):
        self.block.zero_()
        self._row = 0

    def compute(self):
        """the one device-to-host copy -> dict(loss, rows, accuracy, balanced_accuracy, precision, recall, f1_score, confusion)"""
        host = self.block.cpu().numpy()
        loss_sum, rows = float(host[:8].view(np.float64)[0]), int(host[8:16].view(np.int64)[0])
        confusion = host[self.HEADER:].view(np.int32).reshape(self.num_classes, self.num_classes).astype(np.int64)
        out = {"loss": loss_sum / rows if rows else float("nan"), "rows": rows}
        out.update(metrics_from_confusion(confusion))
        out["confusion"] = confusion
        return out
