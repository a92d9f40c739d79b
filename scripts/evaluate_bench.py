"""What evaluate_model on the device (mmskin.evaluate, csrc/auc.hip) costs next to the reference's way of evaluating a fold.

    python scripts/evaluate_bench.py [--runs 20] [--warmup 3] [--batch 256]

For N = 5 000 and N = 50 000 rows of C = 6 classes, with a stub model that hands back stored device logits (so that the encoder,
the same on both sides, is left out) and a loader of host batches (names, row indices, metadata, labels):
(a) `device`: mmskin.evaluate.evaluate_model -- per batch one EpochMeter launch and a device copy of the labels, then one AUC
    launch, one arg-max and the host copies.
(b) `reference`: the loop of utils/model_metrics.py restated here -- per batch soft-max, arg-max and three .cpu() copies, then
    the metrics on the host, by scikit-learn where it is importable and otherwise by the numpy paths of mmskin.evaluate.
    Both write the four .npy files.  Wall time around a call that ends in host copies, the two alternating in one loop: the
    median of --runs (>= 20) after --warmup, with the minimum and maximum beside it.
(c) `kernel`: mmskin_ovr_auc_counts alone on the N x C probabilities, device events around one call (its memset included).
Needs a GPU: no fallback.  The host side of (b) depends on the machine's CPU.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "multimodal-model-skin-lesion-classifier_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"


class StoredLogits(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.register_buffer("logits", logits)

    def forward(self, images, metadata):
        return self.logits[images]


class Loader(list):
    def __init__(self, labels, batch):
        n = len(labels)
        super().__init__(([str(i) for i in range(a, min(a + batch, n))], torch.arange(a, min(a + batch, n)), torch.zeros(min(a + batch, n) - a, 1),
                          labels[a:a + batch]) for a in range(0, n, batch))
        self.dataset = range(n)


def host_metrics(labels, preds, probs):
    C = probs.shape[1]
    try:
        from sklearn import metrics as sk
        from sklearn.preprocessing import label_binarize
    except ImportError:
        from mmskin import evaluate as ev
        from mmskin.criterion import metrics_from_confusion
        cm = np.zeros((C, C), dtype=np.int64)
        np.add.at(cm, (labels, preds), 1)
        out = metrics_from_confusion(cm)
        out["auc"] = ev.auc_from_counts(ev.ovr_auc_counts(torch.from_numpy(probs), torch.from_numpy(labels)), C)
        return out, "numpy"
    avg = {} if C == 2 else {"average": "weighted"}
    out = {"accuracy": sk.accuracy_score(labels, preds), "balanced_accuracy": sk.balanced_accuracy_score(labels, preds),
           "precision": sk.precision_score(labels, preds, zero_division=0, **avg), "recall": sk.recall_score(labels, preds, zero_division=0, **avg),
           "f1_score": sk.f1_score(labels, preds, zero_division=0, **avg)}
    out["auc"] = sk.roc_auc_score(labels, probs[:, 1]) if C == 2 else sk.roc_auc_score(label_binarize(labels, classes=np.arange(C)), probs,
                                                                                         average="weighted", multi_class="ovr")
    return out, "scikit-learn"


def reference_way(model, loader, folder):
    model.eval()
    all_labels, all_preds, all_probs = [], [], []
    with torch.no_grad():
        for _, images, metadata, labels in loader:
            images, metadata, labels = images.to(DEV, non_blocking=True), metadata.to(DEV, non_blocking=True), labels.to(DEV, non_blocking=True)
            probs = torch.softmax(model(images, metadata), dim=1)
            preds = torch.argmax(probs, dim=1)
            all_labels.append(labels.cpu())
            all_preds.append(preds.cpu())
            all_probs.append(probs.cpu())
    labels, preds, probs = torch.cat(all_labels).numpy(), torch.cat(all_preds).numpy(), torch.cat(all_probs).numpy()
    os.makedirs(folder, exist_ok=True)
    for name, arr in (("labels", labels), ("predictions", preds), ("probabilities", probs), ("targets", np.arange(probs.shape[1]))):
        np.save(os.path.join(folder, name + ".npy"), arr)
    return host_metrics(labels, preds, probs)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rows", type=int, nargs="+", default=[5000, 50000])
    ap.add_argument("--classes", type=int, default=6)
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20 (the figure is a median)")
    if not torch.cuda.is_available():
        sys.exit("evaluate_bench: no GPU visible; this measurement has no CPU fallback")
    from mmskin import evaluate as ev
    from mmskin._lib import call, ptr, stream

    C = args.classes
    out = {"what": "evaluate", "device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup, "batch": args.batch, "classes": C,
           "rows": {}}
    with tempfile.TemporaryDirectory() as td:
        for N in args.rows:
            g = torch.Generator().manual_seed(N)
            labels = torch.randint(0, C, (N,), generator=g)
            logits = torch.randn((N, C), generator=g)
            logits[torch.arange(N), labels] += 1.0
            model, loader = StoredLogits(logits.to(DEV)), Loader(labels, args.batch)
            ways = {"device": lambda: ev.evaluate_model(model, loader, None, DEV, 0, td, "device")[0],
                    "reference": lambda: reference_way(model, loader, os.path.join(td, "reference_fold_0"))[0]}
            ms, last = {k: [] for k in ways}, {}
            for i in range(args.warmup + args.runs):
                for name, fn in ways.items():                          # alternating: both see the same machine state
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[name] = fn()
                    if i >= args.warmup:
                        ms[name].append((time.perf_counter() - t0) * 1e3)
            rec = {name: spread(v) for name, v in ms.items()}
            rec["reference_host_metrics_by"] = reference_way(model, loader, os.path.join(td, "reference_fold_0"))[1]
            rec["auc"] = {name: last[name]["auc"] for name in ways}
            rec["max_metric_difference"] = max(abs(last["device"][k] - float(last["reference"][k])) for k in last["reference"])

            probs = torch.softmax(logits.to(DEV), dim=1).contiguous()
            y = labels.to(DEV)
            block = torch.empty(3 * C + 1, dtype=torch.int64, device=DEV)
            us = []
            for i in range(args.warmup + args.runs):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call("mmskin_ovr_auc_counts", ptr(probs), ptr(y), N, C, ptr(block), stream())
                b.record()
                b.synchronize()
                if i >= args.warmup:
                    us.append(a.elapsed_time(b) * 1e3)
            rec["kernel"] = {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                             "compares": int(N) * int(N)}
            out["rows"][str(N)] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
