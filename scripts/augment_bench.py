"""Training-time augmentation timing: `TrainAugment.apply` on a raw uint8 batch (default 256 x 224 x 224 x 3), to set it against
the ~17 ms train step it feeds.

    python scripts/augment_bench.py [--batch 256] [--size 224] [--runs 30] [--warmup 5] [--seed 0]

Two figures, both from device events, each the median over `--runs` (>= 20) after `--warmup` runs:
  apply    the whole Python call: host packing of the parameter table, then the library call
  call     `mmskin_train_augment_u8` alone with the table already packed (validation, the table's upload, the kernel),
           next to the bytes the kernel must move once (read N*H*W*3, write N*H*W*3; halo and bilinear re-reads excluded)
Every run reads and writes buffers of its own (allocated and filled before the timed window), so no run finds its input or
output in a cache left by the previous one.  The probabilities are the reference's (skinLesionDatasets.py:74-113), so the
mix of cheap (copy) and expensive (rotate + blur + HSV) samples is the one a train loop sees.  Needs a GPU: no fallback.
"""
import argparse
import ctypes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20 (the figure is a median)")
    if not torch.cuda.is_available():
        sys.exit("augment_bench: no GPU visible; this measurement has no CPU fallback")
    from mmskin._lib import call, ptr, stream
    from mmskin.preprocess import TrainAugment, pack_augment_params

    n, h, w = args.batch, args.size, args.size
    aug = TrainAugment()
    params = aug.sample(n, h, w, torch.Generator().manual_seed(args.seed))
    table = pack_augment_params(params, h, w)
    scratch = torch.empty(table.nbytes, dtype=torch.uint8, device=DEV)
    host = ctypes.c_void_p(table.ctypes.data)
    total = args.warmup + args.runs
    g = torch.Generator(device=DEV).manual_seed(args.seed)
    # one source and one destination per run and per figure, all written before any timing starts
    srcs = [torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8, device=DEV) for _ in range(2 * total)]
    dsts = [torch.zeros((n, h, w, 3), dtype=torch.uint8, device=DEV) for _ in range(total)]
    torch.cuda.synchronize()

    def timed(fn):
        ms = []
        for i in range(total):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(i)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                ms.append(a.elapsed_time(b))
        return ms

    outs = []                            # apply allocates its result: kept alive, so every run writes memory of its own
    apply_ms = timed(lambda i: outs.append(aug.apply(srcs[i], params)))
    call_ms = timed(lambda i: call("mmskin_train_augment_u8", ptr(srcs[total + i]), n, h, w, host, ptr(scratch), ptr(dsts[i]),
                                     stream()))
    nbytes = 2 * n * h * w * 3
    c_med = statistics.median(call_ms)
    print(json.dumps({
        "what": "train_augment_u8", "batch": n, "height": h, "width": w, "runs": args.runs, "warmup": args.warmup,
        "device": torch.cuda.get_device_name(0),
        "stage_share": {k: round(float(params[k].double().mean()), 3) for k in ("rotate", "hflip", "vflip", "blur", "dropout", "hsv", "bc")},
        "apply_ms_median": round(statistics.median(apply_ms), 4), "apply_ms_min": round(min(apply_ms), 4),
        "apply_ms_max": round(max(apply_ms), 4),
        "call_ms_median": round(c_med, 4), "call_ms_min": round(min(call_ms), 4), "call_ms_max": round(max(call_ms), 4),
        "bytes_moved_once": nbytes, "call_gb_per_s": round(nbytes / (c_med * 1e-3) / 1e9, 1),
    }))


if __name__ == "__main__":
    main()
