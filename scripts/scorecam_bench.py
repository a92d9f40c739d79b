"""Score-CAM timing on the configuration every Score-CAM script of the reference uses: densenet169 + one-hot metadata +
crossattention, one 224 x 224 image, hook on image_encoder.features[-1] (C = 1664 channels, 7 x 7 map).

    python scripts/scorecam_bench.py [--chunks 64 128 256] [--runs 7] [--warmup 2] [--kernel-runs 20] [--baseline-runs 3]

Per chunk size, each figure the median of repeated runs after warm-ups, from device events (the heat map's copy to the
host ends every whole call, so the events bracket finished work):
  call      mmskin.cam.ScoreCAM.generate_heatmap, the whole call
  mask      the mask kernel alone over all C channels (ceil(C / chunk) launches), with the bytes it writes over the time
  combine   mmskin_scorecam_combine alone (both launches)
and once:
  baseline  the reference's per-channel loop driven through the same HIP model: C batch-1 forwards with the hook on, a
            `.item()` and a full-size `.cpu().numpy()` per channel, the weighted sum in numpy -- what a user gets without
            mmskin.cam
Every kernel run writes buffers of its own, allocated before the timed window.  Needs a GPU: no fallback.
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


def per_channel_loop(model, layer, image, metadata, target):
    """the reference's algorithm, one channel at a time (ScoreCam.py:91-155)"""
    store = {}
    handle = layer.register_forward_hook(lambda mod, i, o: store.__setitem__("f", o.detach()))
    try:
        model(image, metadata)
        fmap = store["f"]
        up = torch.nn.Upsample(size=image.shape[2:], mode="bilinear")
        weights, maps = [], []
        for c in range(fmap.shape[1]):
            cam = up(fmap[:, c:c + 1])
            lo, hi = cam.min(), cam.max()
            cam = (cam - lo) / (hi - lo) if hi - lo != 0 else torch.zeros_like(cam)
            with torch.no_grad():
                weights.append(torch.softmax(model(image * cam, metadata), dim=1)[0, target].item())
            maps.append(cam.squeeze().cpu().numpy())
    finally:
        handle.remove()
    heat = np.zeros_like(maps[0])
    for w, m in zip(weights, maps):
        heat += w * m
    heat = np.maximum(heat, 0)
    return (heat - heat.min()) / (heat.max() - heat.min())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-runs", type=int, default=20)
    ap.add_argument("--baseline-runs", type=int, default=3)
    ap.add_argument("--target", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scorecam_bench: no GPU visible; this measurement has no CPU fallback")
    from mmskin import ops
    from mmskin.cam import ScoreCAM
    from models import multimodalIntraInterModal as M

    torch.manual_seed(0)
    model = M.MultimodalModel(num_classes=6, num_heads=2, device=DEV, cnn_model_name="densenet169", text_model_name="one-hot-encoder",
                              vocab_size=86, attention_mecanism="crossattention").to(DEV).eval()
    layer = model.image_encoder.features[-1]
    hw = args.size
    image = torch.randn(1, 3, hw, hw, device=DEV)
    metadata = torch.randn(1, 86, device=DEV)
    common = {"what": "scorecam", "encoder": "densenet169", "fusion": "crossattention", "height": hw, "width": hw,
              "device": torch.cuda.get_device_name(0), "backbone_dtype": model.image_encoder.compute_dtype}

    heats = {}
    for chunk in args.chunks:
        cam = ScoreCAM(model, layer, DEV, chunk=chunk)
        try:
            call_ms = timed(lambda i: heats.__setitem__(chunk, cam.generate_heatmap(image, metadata, args.target)), args.warmup, args.runs)
            fmap = cam.features[0].float().contiguous()
            scores = cam.scores.clone()
        finally:
            cam.remove_hook()
        C = fmap.shape[0]
        minmax = ops.scorecam_minmax(fmap, (hw, hw))
        n_launch = -(-C // chunk)
        total = 3 + args.kernel_runs
        outs = [[torch.empty((chunk, 3, hw, hw), device=DEV) for _ in range(n_launch)] for _ in range(total)]
        torch.cuda.synchronize()

        def masks(i):
            for k in range(n_launch):
                ops.scorecam_mask(fmap, minmax, image[0], k * chunk, min(chunk, C - k * chunk), chunk, out=outs[i][k])

        mask_ms = timed(masks, 3, args.kernel_runs)
        del outs
        keep = []
        combine_ms = timed(lambda i: keep.append(ops.scorecam_combine(fmap, minmax, scores, (hw, hw))), 3, args.kernel_runs)
        written = n_launch * chunk * 3 * hw * hw * 4
        m_med = statistics.median(mask_ms)
        print(json.dumps(dict(common, chunk=chunk, channels=C, map=list(fmap.shape[1:]), masked_forwards=n_launch * chunk,
                              call=stats(call_ms), mask=stats(mask_ms), mask_launches=n_launch, mask_bytes_written=written,
                              mask_gb_per_s=round(written / (m_med * 1e-3) / 1e9, 1), combine=stats(combine_ms))), flush=True)

    if args.baseline_runs > 0:
        out = {}
        base_ms = timed(lambda i: out.__setitem__("h", per_channel_loop(model, layer, image, metadata, args.target)), 1, args.baseline_runs)
        diffs = {str(c): float(np.abs(h - out["h"]).max()) for c, h in heats.items()}
        print(json.dumps(dict(common, baseline_per_channel_loop=stats(base_ms), max_abs_heat_diff_vs_baseline=diffs)), flush=True)


if __name__ == "__main__":
    main()
