"""CAM-faithfulness timing on the configuration the Score-CAM scripts of the reference use: densenet169 + one-hot metadata +
crossattention, 224 x 224 images, S = 32 steps, blur baseline 11 / 5 (RISE's).

    python scripts/faithfulness_bench.py [--images 4] [--steps 32] [--chunks 64 128 256] [--runs 5] [--warmup 2]
                                         [--kernel-runs 20] [--baseline-runs 2]

Per chunk size, each figure the median of repeated runs after warm-ups, from device events (every timed call ends in a copy
of its result to the host, so the events bracket finished work):
  call      mmskin.faithfulness.CamFaithfulness.evaluate + .cpu(), the whole call: N * (2 S + 3) perturbed forwards
and once, each kernel alone on the call's own shapes:
  rank      mmskin_faith_rank over the N maps
  blur      mmskin_faith_blur over the N images
  perturb   mmskin_faith_perturb over all rows (ceil(rows / chunk) launches), with the bytes it writes over the time
  curves    mmskin_faith_curves (both launches)
and once:
  baseline  a reference-style loop through the same HIP model: per image torch.argsort of the map, per step an index mask on
            the flattened image, a batch-1 forward and an `.item()` -- what a user writes without mmskin.faithfulness
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


def reference_style_loop(model, images, metadata, saliency, baseline, steps):
    """deletion and insertion curves one image and one step at a time"""
    N, _, H, W = images.shape
    HW = H * W
    curves = np.zeros((2, N, steps + 1))
    with torch.no_grad():
        targets = model(images, metadata).argmax(dim=1).tolist()
        for n in range(N):
            order = torch.argsort(saliency[n].flatten(), descending=True, stable=True)
            for which, (start, finish) in enumerate(((images[n], baseline[n]), (baseline[n], images[n]))):
                for k in range(steps + 1):
                    x = start.clone().reshape(3, HW)
                    idx = order[:(k * HW) // steps]
                    x[:, idx] = finish.reshape(3, HW)[:, idx]
                    probs = torch.softmax(model(x.reshape(1, 3, H, W), metadata[n:n + 1]).float(), dim=1)
                    curves[which, n, k] = probs[0, targets[n]].item()
    return curves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--chunks", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-runs", type=int, default=20)
    ap.add_argument("--baseline-runs", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("faithfulness_bench: no GPU visible; this measurement has no CPU fallback")
    from mmskin import ops
    from mmskin.faithfulness import CamFaithfulness
    from models import multimodalIntraInterModal as M

    torch.manual_seed(0)
    model = M.MultimodalModel(num_classes=6, num_heads=2, device=DEV, cnn_model_name="densenet169", text_model_name="one-hot-encoder",
                              vocab_size=86, attention_mecanism="crossattention").to(DEV).eval()
    N, S, hw = args.images, args.steps, args.size
    images = torch.randn(N, 3, hw, hw, device=DEV)
    metadata = torch.randn(N, 86, device=DEV)
    # CAM-like maps: a 7x7 random map upsampled, rectified (about half the pixels tie at zero) and scaled into [0, 1]
    coarse = torch.relu(torch.randn(N, 1, 7, 7, device=DEV))
    saliency = torch.nn.functional.interpolate(coarse, size=(hw, hw), mode="bilinear")[:, 0].contiguous()
    saliency = saliency / saliency.amax(dim=(1, 2), keepdim=True)
    common = {"what": "cam_faithfulness", "encoder": "densenet169", "fusion": "crossattention", "height": hw, "width": hw, "images": N,
              "steps": S, "rows": N * (2 * S + 3), "device": torch.cuda.get_device_name(0),
              "backbone_dtype": model.image_encoder.compute_dtype}

    results = {}
    for chunk in args.chunks:
        scorer = CamFaithfulness(model, DEV, steps=S, chunk=chunk)
        call_ms = timed(lambda i: results.__setitem__(chunk, scorer.evaluate(images, metadata, saliency).cpu()), args.warmup, args.runs)
        print(json.dumps(dict(common, chunk=chunk, forwards=-(-N * (2 * S + 3) // chunk), call=stats(call_ms),
                              ms_per_image=round(statistics.median(call_ms) / N, 3))), flush=True)

    # the four kernels alone
    chunk = args.chunks[-1]
    scorer = CamFaithfulness(model, DEV, steps=S, chunk=chunk)
    total = 3 + args.kernel_runs
    rank_out = [torch.empty((N, hw, hw), device=DEV, dtype=torch.int32) for _ in range(total)]
    rank_ms = timed(lambda i: ops.faith_rank(saliency, out=rank_out[i]), 3, args.kernel_runs)
    blur_out = [torch.empty_like(images) for _ in range(total)]
    blur_ms = timed(lambda i: ops.faith_blur(images, scorer.taps, out=blur_out[i]), 3, args.kernel_runs)
    rows = torch.from_numpy(scorer.row_table(N)).to(DEV)
    R = rows.shape[0]
    n_launch = -(-R // chunk)
    outs = [[torch.empty((chunk, 3, hw, hw), device=DEV) for _ in range(n_launch)] for _ in range(total)]
    torch.cuda.synchronize()

    def perturbs(i):
        for k in range(n_launch):
            ops.faith_perturb(images, blur_out[0], rank_out[0], saliency, rows[k * chunk:], S, min(chunk, R - k * chunk), chunk, out=outs[i][k])

    perturb_ms = timed(perturbs, 3, args.kernel_runs)
    del outs
    logits = torch.randn(R, 6, device=DEV)
    keep = []
    curves_ms = timed(lambda i: keep.append(ops.faith_curves(logits, S, N)), 3, args.kernel_runs)
    written = n_launch * chunk * 3 * hw * hw * 4
    p_med = statistics.median(perturb_ms)
    print(json.dumps(dict(common, chunk=chunk, rank=stats(rank_ms), blur=stats(blur_ms), perturb=stats(perturb_ms),
                          perturb_launches=n_launch, perturb_bytes_written=written,
                          perturb_gb_per_s=round(written / (p_med * 1e-3) / 1e9, 1), curves=stats(curves_ms))), flush=True)

    if args.baseline_runs > 0:
        base = ops.faith_blur(images, scorer.taps)
        out = {}
        base_ms = timed(lambda i: out.__setitem__("c", reference_style_loop(model, images, metadata, saliency, base, S)), 1,
                        args.baseline_runs)
        diffs = {}
        for c, res in results.items():
            got = np.stack([res.deletion.numpy(), res.insertion.numpy()])
            diffs[str(c)] = float(np.abs(got - out["c"]).max())
        print(json.dumps(dict(common, baseline_reference_style_loop=stats(base_ms), baseline_forwards=N * (2 * S + 2) + 1,
                              max_abs_curve_diff_vs_baseline=diffs)), flush=True)


if __name__ == "__main__":
    main()
