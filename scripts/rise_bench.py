"""RISE timing at the paper's working point: n_masks = 4000, grid 8, p1 = 0.5, 224 x 224 images, on resnet-50 and on one
transformer encoder (swin_tiny), each with one-hot metadata and crossattention.

    python scripts/rise_bench.py [--images 2] [--masks 4000] [--chunk 256] [--encoders resnet-50 swin_tiny_patch4_window7_224]
                                 [--runs 3] [--warmup 1] [--kernel-runs 10] [--baseline-runs 2]

Per encoder, each figure the median of repeated runs after warm-ups, from device events (every timed call ends in a copy of
its result to the host, so the events bracket finished work):
  call      mmskin.rise.RISE.generate_batch + .cpu(), the whole call: N * n_masks masked forwards and the clean one
  baseline  the same computation composed from torch ops on the same HIP model: a mask tensor [n_masks, H, W] kept in HBM
            (made once, outside the timed window, by F.interpolate of random cells and a crop per mask -- the published code's
            way), per chunk a multiply and a forward, then soft-max and a weighted einsum.  `baseline_masks` times making the
            mask tensor.
and once, the kernels alone on the call's own shapes:
  apply       mmskin_rise_apply over all rows (ceil(rows / chunk) launches), with the bytes it writes over the time
  accumulate  mmskin_rise_accumulate (its four launches)
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

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

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


def torch_masks(n_masks, grid, p1, H, W, seed):
    """the published generator: random grid x grid cells, upsampled bilinearly to (grid + 1) cells' size, cropped at a random
    shift -> fp32 [n_masks, H, W] on the device"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ch, cw = -(-H // grid), -(-W // grid)
    cells = (torch.rand(n_masks, 1, grid, grid, device=DEV, generator=g) < p1).float()
    up = F.interpolate(cells, size=((grid + 1) * ch, (grid + 1) * cw), mode="bilinear", align_corners=False)[:, 0]
    dy = torch.randint(0, ch, (n_masks,), device=DEV, generator=g).tolist()
    dx = torch.randint(0, cw, (n_masks,), device=DEV, generator=g).tolist()
    return torch.stack([up[j, dy[j]:dy[j] + H, dx[j]:dx[j] + W] for j in range(n_masks)]).contiguous()


def composed_torch(model, images, metadata, masks, chunk, p1):
    """RISE with the masks in HBM: per image and chunk of masks one multiply and one forward, then a weighted einsum"""
    N, n_masks = images.shape[0], masks.shape[0]
    with torch.no_grad():
        target = model(images, metadata).argmax(dim=1)
        w = torch.empty((N, n_masks), device=DEV, dtype=torch.float64)
        for n in range(N):
            for j0 in range(0, n_masks, chunk):
                m = masks[j0:j0 + chunk]
                x = m[:, None] * images[n][None]
                probs = torch.softmax(model(x, metadata[n:n + 1].expand(m.shape[0], -1)).double(), dim=1)
                w[n, j0:j0 + chunk] = probs[:, target[n]]
        return torch.einsum("nj,jhw->nhw", w, masks.double()) / (n_masks * p1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--masks", type=int, default=4000)
    ap.add_argument("--grid", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--encoders", nargs="+", default=["resnet-50", "swin_tiny_patch4_window7_224"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-runs", type=int, default=10)
    ap.add_argument("--baseline-runs", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rise_bench: no GPU visible; this measurement has no CPU fallback")
    from mmskin import ops
    from mmskin.rise import RISE
    from models import multimodalIntraInterModal as M

    N, n_masks, grid, chunk, hw, p1 = args.images, args.masks, args.grid, args.chunk, args.size, 0.5
    torch.manual_seed(0)
    images = torch.randn(N, 3, hw, hw, device=DEV)
    metadata = torch.randn(N, 86, device=DEV)
    common = {"what": "rise", "height": hw, "width": hw, "images": N, "n_masks": n_masks, "grid": grid, "chunk": chunk,
              "rows": N * n_masks, "device": torch.cuda.get_device_name(0)}

    for name in args.encoders:
        model = M.MultimodalModel(num_classes=6, num_heads=2, device=DEV, cnn_model_name=name, text_model_name="one-hot-encoder",
                                  vocab_size=86, attention_mecanism="crossattention").to(DEV).eval()
        rise = RISE(model, DEV, n_masks=n_masks, grid=grid, p1=p1, chunk=chunk)
        keep = {}
        call_ms = timed(lambda i: keep.__setitem__("r", rise.generate_batch(images, metadata).cpu()), args.warmup, args.runs)
        line = dict(common, encoder=name, backbone_dtype=getattr(model.image_encoder, "compute_dtype", None),
                    forwards=-(-N * n_masks // chunk) + 1, call=stats(call_ms), ms_per_image=round(statistics.median(call_ms) / N, 3))
        if args.baseline_runs > 0:
            made = {}
            mask_ms = timed(lambda i: made.__setitem__("m", torch_masks(n_masks, grid, p1, hw, hw, i)), 0, 1)
            base_ms = timed(lambda i: keep.__setitem__("b", composed_torch(model, images, metadata, made["m"], chunk, p1).cpu()), 1,
                            args.baseline_runs)
            line.update(baseline_composed_torch=stats(base_ms), baseline_masks=stats(mask_ms), baseline_mask_bytes=made["m"].numel() * 4,
                        baseline_over_call=round(statistics.median(base_ms) / statistics.median(call_ms), 3))
            del made
        print(json.dumps(line), flush=True)
        del model, rise
        torch.cuda.empty_cache()

    # the kernels alone
    R = N * n_masks
    n_launch = -(-R // chunk)
    total = 2 + args.kernel_runs
    base = torch.zeros_like(images)
    outs = [torch.empty((chunk, 3, hw, hw), device=DEV) for _ in range(min(n_launch, 4))]          # four rotating chunk buffers
    torch.cuda.synchronize()

    def applies(i):
        for k in range(n_launch):
            ops.rise_apply(images, base, 0, grid, p1, n_masks, k * chunk, min(chunk, R - k * chunk), chunk, out=outs[k % len(outs)])

    apply_ms = timed(applies, 2, args.kernel_runs)
    logits, clean = torch.randn(n_launch * chunk, 6, device=DEV), torch.randn(N, 6, device=DEV)
    acc_out = [(torch.empty((N, hw, hw), device=DEV, dtype=torch.float64), torch.empty((hw, hw), device=DEV, dtype=torch.float64),
                torch.empty((N,), device=DEV, dtype=torch.float64), torch.empty((N,), device=DEV, dtype=torch.int32)) for _ in range(total)]
    acc_ms = timed(lambda i: ops.rise_accumulate(logits, clean, (hw, hw), 0, grid, p1, n_masks, out=acc_out[i]), 2, args.kernel_runs)
    written = n_launch * chunk * 3 * hw * hw * 4
    a_med = statistics.median(apply_ms)
    print(json.dumps(dict(common, apply=stats(apply_ms), apply_launches=n_launch, apply_bytes_written=written,
                          apply_gb_per_s=round(written / (a_med * 1e-3) / 1e9, 1), accumulate=stats(acc_ms),
                          accumulate_mask_evaluations=n_masks * hw * hw)), flush=True)


if __name__ == "__main__":
    main()
