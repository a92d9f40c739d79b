"""Metadata-LIME timing at the reference's setting (lime's defaults: 5000 neighbourhood rows, num_features 15) on the PAD-UFES-20
width of 91 encoded columns: densenet169 + gfcam (the configuration of the reference's interpretability scripts) and the headline
ResNet-50 + crossattention.

    python scripts/lime_bench.py [--configs densenet169:gfcam resnet-50:crossattention] [--batch 2] [--rows 8192]
                                 [--samples 5000] [--features 15] [--baseline-rows 256] [--runs 5] [--warmup 2]

Per configuration, each figure the median of repeated runs after warm-ups, from device events (every timed call ends with its
result on the device; the event pair brackets finished work), as time PER EXPLAINED SAMPLE:
  lime         mmskin.lime.MetadataLime.explain: one image encoding per batch, the neighbourhood kernel, the fusion head in `rows`
               blocks, the reduce kernel per block, the solve
  baseline     the straightforward loop on the public API, model(image, row) at the reference's batch 1, one forward per
               neighbourhood row -- timed on `--baseline-rows` rows and SCALED to the sample's row count (the output says so)
  kernels      the three entry points alone on a batch's rows (logits given): neighbourhood, reduce, solve
  head_call    one `rows`-sized model.fuse call
Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "multimodal-model-skin-lesion-classifier_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
VOCAB = 91


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


def stats(ms, per=1):
    return {"median_ms": round(statistics.median(ms) / per, 4), "min_ms": round(min(ms) / per, 4), "max_ms": round(max(ms) / per, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["densenet169:gfcam", "resnet-50:crossattention"])
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--features", type=int, default=15)
    ap.add_argument("--baseline-rows", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lime_bench: no GPU visible; this measurement has no CPU fallback")
    from mmskin import ops
    from mmskin.lime import MetadataLime
    from models import multimodalIntraInterModal as M

    # encoded training rows like PAD-UFES-20's: 88 one-hot cells, 3 standardised numerics
    rng = np.random.default_rng(0)
    p = rng.uniform(0.05, 0.95, VOCAB - 3)
    train = np.concatenate([(rng.random((1000, VOCAB - 3)) < p).astype(np.float32), rng.normal(0, 1, (1000, 3)).astype(np.float32)], axis=1)
    B, N, K, hw = args.batch, args.samples, args.features, args.size
    x = torch.from_numpy(train[:B].copy()).to(DEV)
    keep = [None, None]

    for config in args.configs:
        cnn, fusion = config.split(":")
        torch.manual_seed(0)
        model = M.MultimodalModel(num_classes=6, num_heads=8, device=DEV, cnn_model_name=cnn, text_model_name="one-hot-encoder",
                                  vocab_size=VOCAB, attention_mecanism=fusion, n=2).to(DEV).eval()
        images = torch.randn(B, 3, hw, hw, device=DEV)
        ex = MetadataLime(model, None, DEV, train, num_samples=N, num_features=K, seed=0, rows_per_head_call=args.rows)
        out = {"what": "metadata_lime", "encoder": cnn, "fusion": fusion, "batch": B, "height": hw, "width": hw, "features": VOCAB,
               "rows_per_sample": N, "num_features": K, "rows_per_head_call": ex.rows_per_head_call,
               "device": torch.cuda.get_device_name(0), "backbone_dtype": model.image_encoder.compute_dtype,
               "linear_dtype": ops.get_linear_dtype()}

        def explain(i):
            ex.reset()                                                       # the same draws every run
            keep[0] = ex.explain(images, x)

        out["lime_per_sample"] = stats(timed(explain, args.warmup, args.runs), per=B)
        res = keep[0]

        mean, scale = torch.from_numpy(ex.mean).to(DEV), torch.from_numpy(ex.scale).to(DEV)
        n_base = min(args.baseline_rows, N)
        metas, _ = ops.lime_neighbourhood(x[:1], mean, scale, N, 0, row0=0, row1=n_base)

        def baseline(i):
            with torch.no_grad():
                keep[1] = torch.cat([torch.softmax(model(images[:1], metas[r:r + 1]).float(), dim=-1) for r in range(n_base)])

        base_ms = timed(baseline, 1, max(args.runs // 2, 1))
        factor = N / n_base
        out["baseline_per_sample"] = dict(stats([m * factor for m in base_ms]), scaled=True, timed_rows=n_base,
                                          note=f"batch-1 forwards timed on {n_base} rows, scaled to {N}")
        with torch.no_grad():
            out["encode_image"] = stats(timed(lambda i: keep.__setitem__(1, model.encode_image(images)), args.warmup, args.runs))
            step = min(args.rows, B * N)
            block, _ = ops.lime_neighbourhood(x, mean, scale, N, 0, row0=0, row1=step)
            feats = keep[1][:1].expand(step, -1).contiguous()
            head = timed(lambda i: keep.__setitem__(1, model.fuse(feats, block)), args.warmup, args.runs)
            out["head_call"] = dict(stats(head), rows=step, rows_per_s=round(step / (statistics.median(head) * 1e-3)))
            # the kernels alone, on the whole batch's rows
            C = int(model.num_classes)
            logits = torch.randn(B * N, C, device=DEV)
            rows_w = [None]
            out["kernel_neighbourhood"] = stats(timed(lambda i: rows_w.__setitem__(0, ops.lime_neighbourhood(x, mean, scale, N, 0)), args.warmup,
                                                      args.runs), per=B)
            rows, w = rows_w[0]
            acc = ops.lime_accumulator(B, N, VOCAB, C, DEV)
            out["kernel_reduce"] = stats(timed(lambda i: ops.lime_reduce(rows, w, logits, mean, scale, acc, B, N, 0), args.warmup, args.runs), per=B)
            acc.zero_()
            ops.lime_reduce(rows, w, logits, mean, scale, acc, B, N, 0)
            out["kernel_solve"] = stats(timed(lambda i: keep.__setitem__(1, ops.lime_solve(acc, x, mean, scale, N, C, K)), args.warmup, args.runs),
                                        per=B)
        out["speedup_vs_baseline"] = round(out["baseline_per_sample"]["median_ms"] / out["lime_per_sample"]["median_ms"], 1)
        out["max_abs_coef"] = float(res.coef.abs().max())
        out["min_score"], out["max_score"] = float(res.score.min()), float(res.score.max())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
