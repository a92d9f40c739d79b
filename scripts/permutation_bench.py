"""Metadata permutation-importance timing on a fold like PAD-UFES-20's (460 validation samples, 91 encoded columns: 18 one-hot
blocks of 88 cells and 3 numerics, so 21 groups; 10 repeats): densenet169 + gfcam (the configuration of the reference's
interpretability scripts) and the headline ResNet-50 + crossattention.

    python scripts/permutation_bench.py [--configs densenet169:gfcam resnet-50:crossattention] [--samples 460] [--repeats 10]
                                        [--rows 8192] [--image-batch 64] [--baseline-cells 3] [--runs 3] [--warmup 1]

Per configuration, each figure the median of repeated runs after warm-ups, from device events (every timed call ends with its
result on the host or the device; the event pair brackets finished work), as time PER STUDY (all R x G cells of the fold):
  fit          mmskin.permutation.MetadataPermutationImportance.fit: every image encoded once, the indices kernel, then per block
               of `rows` the rows kernel, the fusion head and the scores kernel, and the finalize kernels
  baseline     the naive loop on the public API: one mmskin.evaluate.evaluate_model pass over the fold per (repeat, group) with
               that group's columns shuffled, on the same HIP model -- timed on `--baseline-cells` cells and SCALED to R x G (the
               output says so)
  kernels      the entry points alone on the whole study (logits given): indices, rows, scores, finalize
Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "multimodal-model-skin-lesion-classifier_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
BLOCKS = [3, 3, 3, 3, 3, 3, 3, 3, 2, 15, 6, 6, 6, 6, 6, 6, 6, 5]             # 18 categorical columns, 88 one-hot cells
VOCAB = sum(BLOCKS) + 3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["densenet169:gfcam", "resnet-50:crossattention"])
    ap.add_argument("--samples", type=int, default=460)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--image-batch", type=int, default=64)
    ap.add_argument("--baseline-cells", type=int, default=3)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("permutation_bench: no GPU visible; this measurement has no CPU fallback")
    from mmskin import ops
    from mmskin.evaluate import evaluate_model
    from mmskin.permutation import MetadataPermutationImportance
    from models import multimodalIntraInterModal as M

    rng = np.random.default_rng(0)
    S, R, hw = args.samples, args.repeats, args.size
    x = np.zeros((S, VOCAB), dtype=np.float32)
    group = np.zeros(VOCAB, dtype=np.int32)
    at = 0
    for g, width in enumerate(BLOCKS):
        x[np.arange(S), at + rng.integers(0, width, S)] = 1.0
        group[at:at + width] = g
        at += width
    x[:, at:] = rng.normal(0, 1, (S, 3))
    group[at:] = len(BLOCKS) + np.arange(3)
    G = len(BLOCKS) + 3
    labels = rng.integers(0, 6, S).astype(np.int64)
    keep = [None]

    for config in args.configs:
        cnn, fusion = config.split(":")
        torch.manual_seed(0)
        model = M.MultimodalModel(num_classes=6, num_heads=8, device=DEV, cnn_model_name=cnn, text_model_name="one-hot-encoder",
                                  vocab_size=VOCAB, attention_mecanism=fusion, n=2).to(DEV).eval()
        images = torch.randn(S, 3, hw, hw, device=DEV)
        pi = MetadataPermutationImportance(model, groups=group, n_repeats=R, seed=0, rows_per_call=args.rows, image_batch_size=args.image_batch)
        out = {"what": "metadata_permutation_importance", "encoder": cnn, "fusion": fusion, "samples": S, "height": hw, "width": hw,
               "columns": VOCAB, "groups": G, "repeats": R, "rows": R * G * S, "rows_per_call": max(args.rows // S, 1) * S,
               "image_batch": args.image_batch, "device": torch.cuda.get_device_name(0), "backbone_dtype": model.image_encoder.compute_dtype,
               "linear_dtype": ops.get_linear_dtype()}
        out["fit"] = stats(timed(lambda i: keep.__setitem__(0, pi.fit(images, x, labels)), args.warmup, args.runs))
        res = keep[0]

        xd, yd = torch.from_numpy(x).to(DEV), torch.from_numpy(labels).to(DEV)
        gd = torch.from_numpy(group).to(DEV)
        perm = ops.permutation_indices(0, R, G, S, DEV)
        cells = min(args.baseline_cells, R * G)
        names = [str(i) for i in range(S)]
        tmp = tempfile.mkdtemp(prefix="permutation_bench_")

        def baseline(i):
            for cell in range(cells):
                metas = ops.permuted_rows(xd, gd, perm, row0=cell * S, row1=(cell + 1) * S)
                loader = [(names[a:a + args.image_batch], images[a:a + args.image_batch], metas[a:a + args.image_batch], yd[a:a + args.image_batch])
                          for a in range(0, S, args.image_batch)]
                keep[0] = evaluate_model(model, loader, None, DEV, cell, tmp, "bench")

        base_ms = timed(baseline, 1, max(args.runs // 2, 1))
        factor = R * G / cells
        out["baseline"] = dict(stats([m * factor for m in base_ms]), scaled=True, timed_cells=cells,
                               note=f"evaluate_model passes timed on {cells} cells, scaled to {R * G}")
        with torch.no_grad():
            K = int(model.num_classes)
            logits = torch.randn(R * G * S, K, device=DEV)
            confusion, counts = ops.permutation_accumulators(R, G, K, DEV)
            base = torch.zeros(3, dtype=torch.float64, device=DEV)
            out["kernel_indices"] = stats(timed(lambda i: ops.permutation_indices(0, R, G, S, DEV), args.warmup, args.runs))
            out["kernel_rows"] = stats(timed(lambda i: keep.__setitem__(0, ops.permuted_rows(xd, gd, perm)), args.warmup, args.runs))
            out["kernel_scores"] = stats(timed(lambda i: ops.permutation_scores(logits, yd, confusion, counts, 0), args.warmup, args.runs))
            out["kernel_finalize"] = stats(timed(lambda i: keep.__setitem__(0, ops.permutation_finalize(confusion, counts, base)), args.warmup,
                                                 args.runs))
        out["speedup_vs_baseline"] = round(out["baseline"]["median_ms"] / out["fit"]["median_ms"], 1)
        out["baseline_metrics"] = res.baseline
        out["top_group"] = res.ranking("balanced_accuracy")[0]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
