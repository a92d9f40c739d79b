"""Grad-CAM++ timing on the reference's current workload (multiple_sample_using_gradcam_plusplus_atualizado.py:341-399):
densenet169 + one-hot metadata + gfcam, one 224 x 224 image with 15 metadata variants, hook on image_encoder.features[-1]
(C = 1664, 7 x 7 map); and the same on resnet-50 hooked at its last conv (C = 2048).

    python scripts/gradcam_bench.py [--encoders densenet169 resnet-50] [--variants 15] [--runs 7] [--warmup 2] [--kernel-runs 20]

The parent process touches no GPU: every encoder is measured by a child process of its own under a time limit
(--step-timeout seconds), and a child that fails ends the run.  Per encoder, medians after warm-ups, from device events:
  batch     mmskin.cam.GradCAMPlusPlus.generate_batch, the whole call (one encoder pass, one head pass over the 15 rows)
  loop      the reference's loop driven through the same HIP model, per variant: a no_grad forward to pick the class, the hooked
            forward, autograd.grad at the activations, the Grad-CAM++ formula, _normalize and F.interpolate in torch ops, and
            the map's `.cpu().numpy()` -- what a user gets without generate_batch
  kernels   mmskin_gradcam_weights and mmskin_gradcam_map (both launches) alone, on the call's own tensors
Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "multimodal-model-skin-lesion-classifier_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DEV = "cuda:0"


def timed(fn, warmup, runs):
    import torch
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


def reference_loop(model, layer, image, metadata):
    """gradcam_atualizado.py:263-306 behind the mosaic script's class choice (:383-389), one variant at a time"""
    import torch
    import torch.nn.functional as F
    store = {}
    handle = layer.register_forward_hook(lambda mod, i, o: store.__setitem__("a", o))
    maps = []
    try:
        for r in range(metadata.shape[0]):
            meta = metadata[r:r + 1]
            with torch.no_grad():
                pred = int(torch.argmax(model(image, meta), dim=1).item())
            img = image.clone().requires_grad_(True)
            score = model(img, meta)[:, pred]
            acts = store["a"]
            grads = torch.autograd.grad(score, acts, retain_graph=True, create_graph=True)[0]
            g2, g3 = grads ** 2, grads ** 3
            alpha = g2 / (2 * g2 + torch.sum(acts * g3, dim=(2, 3), keepdim=True) + 1e-8)
            weights = torch.sum(alpha * F.relu(grads), dim=(2, 3), keepdim=True)
            cam = F.relu(torch.sum(weights * acts, dim=1, keepdim=True))
            cam = (cam - cam.min()) / (cam.max() - cam.min() + 1e-8)
            cam = F.interpolate(cam, size=image.shape[-2:], mode="bilinear", align_corners=False)
            maps.append(cam.squeeze().detach().cpu().numpy())
    finally:
        handle.remove()
    return maps


def measure(args, encoder):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("gradcam_bench: no GPU visible; this measurement has no CPU fallback")
    import torch.nn as nn
    from mmskin import ops
    from mmskin.cam import GradCAMPlusPlus
    from models import multimodalIntraInterModal as M

    torch.manual_seed(0)
    model = M.MultimodalModel(num_classes=6, num_heads=8, device=DEV, cnn_model_name=encoder, text_model_name="one-hot-encoder",
                              vocab_size=85, attention_mecanism="gfcam", n=2).to(DEV).eval()
    layer = model.image_encoder.features[-1] if encoder == "densenet169" else \
        [m for m in model.image_encoder.modules() if isinstance(m, nn.Conv2d)][-1]
    hw, V = args.size, args.variants
    image = torch.randn(1, 3, hw, hw, device=DEV)
    metadata = torch.randn(V, 85, device=DEV)
    cam = GradCAMPlusPlus(model, layer)
    out = {}
    try:
        batch_ms = timed(lambda i: out.__setitem__("maps", cam.generate_batch(image, metadata, None, variants_per_image=V)),
                         args.warmup, args.runs)
        acts, weights = cam.activations, cam.weights
        row_image = torch.zeros(V, dtype=torch.int32, device=DEV)
        jac, dfeat = torch.rand_like(acts), torch.rand(V, acts.shape[1], device=DEV)
        keep = []
        weights_ms = timed(lambda i: keep.append(ops.gradcam_weights(acts, jac, dfeat, row_image, ops.GRADCAM_PLUSPLUS)), 3, args.kernel_runs)
        map_ms = timed(lambda i: keep.append(ops.gradcam_map(acts, weights, row_image, (hw, hw))), 3, args.kernel_runs)
        pred = cam.pred.cpu().tolist()
    finally:
        cam.remove_hook()
    loop_ms = timed(lambda i: out.__setitem__("loop", reference_loop(model, layer, image, metadata)), 1, args.loop_runs)
    diff = float(np.abs(out["maps"].cpu().numpy() - np.stack(out["loop"])).max())
    b, l = statistics.median(batch_ms), statistics.median(loop_ms)
    print(json.dumps({"what": "gradcam++", "encoder": encoder, "fusion": "gfcam", "height": hw, "width": hw, "variants": V,
                      "channels": acts.shape[1], "map": list(acts.shape[2:]), "device": torch.cuda.get_device_name(0),
                      "backbone_dtype": model.image_encoder.compute_dtype, "batch": stats(batch_ms), "loop": stats(loop_ms),
                      "loop_over_batch": round(l / b, 2), "weights_kernel": stats(weights_ms), "map_kernels": stats(map_ms),
                      "predicted": pred, "max_abs_map_diff_vs_loop": diff}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoders", nargs="+", default=["densenet169", "resnet-50"])
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--variants", type=int, default=15)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-runs", type=int, default=20)
    ap.add_argument("--loop-runs", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return measure(args, args.child)
    for encoder in args.encoders:               # one GPU step per encoder, each a fresh process under its own time limit
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--child", encoder,
               "--size", str(args.size), "--variants", str(args.variants), "--runs", str(args.runs), "--warmup", str(args.warmup),
               "--kernel-runs", str(args.kernel_runs), "--loop-runs", str(args.loop_runs)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(f"gradcam_bench: the {encoder} step ended with status {rc}; nothing further is started")


if __name__ == "__main__":
    main()
