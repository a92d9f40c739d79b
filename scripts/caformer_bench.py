"""Train-step timing of the reference's current configuration (train_pad_20.py:510-516): MultimodalModel with
caformer_b36.sail_in22k_ft_in1k + one-hot metadata + att-intramodal+residual+cross-attention-metadados, unfrozen, Adam, bf16-operand
mode, batch 64 at 224x224.  Prints img/s, ms per step and the fraction of 2.5 PF the step's GEMM FLOPs reach.

    python scripts/caformer_bench.py [--batch 64] [--steps 10] [--warmup 3] [--size 224]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "multimodal-model-skin-lesion-classifier_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK = 2.5e15


def encoder_train_flops(size, depths=(3, 12, 18, 3), dims=(128, 256, 512, 768)):
    """3 x forward multiply-add FLOPs of the encoder's GEMMs, convolutions and attention per image (forward + two backward GEMMs)."""
    h = (size - 3) // 4 + 1
    f = 2 * h * h * 147 * dims[0]
    for i, (d, n) in enumerate(zip(depths, dims)):
        if i:
            h = (h - 1) // 2 + 1
            f += 2 * h * h * 9 * dims[i - 1] * n
        t = h * h
        if i < 2:
            per = 2 * t * (n * 2 * n * 2 + 49 * 2 * n) + 2 * t * 8 * n * n
        else:
            per = 2 * t * (4 * n * n + 8 * n * n) + 4 * t * t * n
        f += d * per
    return 3 * f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=224)
    args = ap.parse_args()
    from mmskin import ops
    from mmskin.optim import Adam
    from models import multimodalIntraInterModal as M
    dev = "cuda:0"
    ops.set_linear_dtype("bf16")
    torch.manual_seed(0)
    model = M.MultimodalModel(num_classes=6, num_heads=8, device=dev, cnn_model_name="caformer_b36.sail_in22k_ft_in1k",
                              text_model_name="one-hot-encoder", vocab_size=85, unfreeze_weights="unfrozen_weights",
                              attention_mecanism="att-intramodal+residual+cross-attention-metadados").to(dev).train()
    opt = Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    img = torch.randn(args.batch, 3, args.size, args.size, device=dev)
    meta = torch.randn(args.batch, 85, device=dev)
    lab = torch.randint(0, 6, (args.batch,), device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(model(img, meta), lab).backward()
        opt.step()

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    flops = encoder_train_flops(args.size) * args.batch
    print(json.dumps({"workload": "caformer_b36 multimodal train step", "batch": args.batch, "size": args.size,
                      "ms_per_step": round(dt * 1e3, 3), "img_per_s": round(args.batch / dt, 1),
                      "encoder_tflop_per_step": round(flops / 1e12, 2), "fraction_of_2_5_pf": round(flops / dt / PEAK, 4)}))


if __name__ == "__main__":
    main()
