"""Bootstrap-interval timing on two folds: N = 460, K = 6 (a PAD-UFES-20 validation fold) and N = 5000, K = 8 (an ISIC-2019 one),
B = 2000 replicates each, plain and stratified resampling.

    python scripts/bootstrap_bench.py [--shapes 460:6 5000:8] [--resamples 2000] [--host-replicates 32] [--runs 5] [--warmup 2]

Per shape and mode, each figure the median of repeated runs after warm-ups, from device events (the event pair brackets finished
work on the stream; inputs are already on the device):
  prep         mmskin.ops.bootstrap_tables: the per-class sorts, tie groups and member lists (torch sorts, once per call)
  replicates   mmskin.ops.bootstrap_replicates on all B replicates: the hot path, one workgroup per replicate
  finalize     mmskin.ops.bootstrap_finalize: metrics, the sorted columns and the summary
  evaluate     mmskin.bootstrap.BootstrapMetrics.evaluate from device tensors to the host result (prep, the point estimate, the
               replicates, finalize and the copies)
  host_loop    for context: sklearn's balanced_accuracy_score and roc_auc_score with sample_weight on `--host-replicates`
               replicates with numpy's multinomial weights, wall clock, SCALED to B -- an extrapolation, labelled so
Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "multimodal-model-skin-lesion-classifier_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"


def timed(fn, warmup, runs):
    ms = []
    for i in range(warmup + runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return ms


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def fold(N, K, rng):
    labels = rng.integers(0, K, N).astype(np.int64)
    raw = rng.random((N, K)) + 0.8 * np.eye(K)[labels]
    return (raw / raw.sum(axis=1, keepdims=True)).astype(np.float32), labels


def host_loop(scores, labels, replicates, rng):
    from sklearn.metrics import balanced_accuracy_score, roc_auc_score
    N, K = scores.shape
    preds, onehot, s64 = scores.argmax(axis=1), np.eye(K)[labels], scores.astype(np.float64)
    t0 = time.perf_counter()
    for _ in range(replicates):
        w = rng.multinomial(N, np.full(N, 1.0 / N)).astype(np.float64)
        balanced_accuracy_score(labels, preds, sample_weight=w)
        roc_auc_score(onehot, s64, multi_class="ovr", average="weighted", sample_weight=w)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["460:6", "5000:8"])
    ap.add_argument("--resamples", type=int, default=2000)
    ap.add_argument("--host-replicates", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bootstrap_bench: no GPU visible; this measurement has no CPU fallback")
    from mmskin import ops
    from mmskin.bootstrap import BootstrapMetrics

    rng = np.random.default_rng(0)
    B = args.resamples
    keep = [None]
    for shape in args.shapes:
        N, K = (int(v) for v in shape.split(":"))
        scores, labels = fold(N, K, rng)
        sd, yd = torch.from_numpy(scores).to(DEV), torch.from_numpy(labels).to(DEV)
        host_ms = host_loop(scores, labels, args.host_replicates, rng)
        for stratified in (False, True):
            mode = ops.BOOTSTRAP_STRATIFIED if stratified else ops.BOOTSTRAP_PLAIN
            out = {"what": "bootstrap_intervals", "rows": N, "classes": K, "resamples": B, "stratified": stratified,
                   "device": torch.cuda.get_device_name(0)}
            out["prep"] = stats(timed(lambda i: keep.__setitem__(0, ops.bootstrap_tables(sd, yd)), args.warmup, args.runs))
            tables = keep[0]
            conf, counts = ops.bootstrap_accumulators(B, K, DEV)
            out["replicates"] = stats(timed(lambda i: ops.bootstrap_replicates(tables, i, mode, conf, counts), args.warmup, args.runs))
            out["finalize"] = stats(timed(lambda i: keep.__setitem__(0, ops.bootstrap_finalize(conf, counts)), args.warmup, args.runs))
            bs = BootstrapMetrics(B, seed=0, stratified=stratified)
            out["evaluate"] = stats(timed(lambda i: keep.__setitem__(0, bs.evaluate(sd, yd)), args.warmup, args.runs))
            res = keep[0]
            out["host_loop"] = {"median_ms": round(host_ms * B / args.host_replicates, 1), "scaled": True, "timed_replicates": args.host_replicates,
                                "note": f"sklearn with sample_weight timed on {args.host_replicates} replicates, EXTRAPOLATED to {B}"}
            out["speedup_vs_host_loop"] = round(out["host_loop"]["median_ms"] / out["evaluate"]["median_ms"], 1)
            out["balanced_accuracy"] = [res.point["balanced_accuracy"], *res.interval("balanced_accuracy")]
            out["auc"] = [res.point["auc"], *res.interval("auc")]
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
