"""CoaT-Lite timings: the two new kernels per stage shape of coat_lite_small at batch 64 next to their HBM floors, and the train step
of MultimodalModel with coat_lite_small.in1k + one-hot metadata + att-intramodal+residual+cross-attention-metadados (unfrozen, Adam,
bf16-operand mode, batch 64 at 224x224).

    python scripts/coat_bench.py [--batch 64] [--steps 10] [--warmup 3] [--size 224] [--hbm-tbs 4.0] [--no-step]

Floors (bytes each pass must move once, halo re-reads excluded; T = B * N * 3C * 4 = the packed qkv):
  factor_attention forward   (2/3 + 2/3 + 1/3) T      k, v (reduce) + q, v (apply) + att written
  factor_attention backward  (2/3 + 1 + 4/3 + 1) T    q, dO (dF) + q, v, dO (conv gradients) + q, k, v, dO (apply) + d(qkv) written
  conv_pos_enc_tokens forward 2 X, backward 5 X       X = B * N * C * 4: x, y / dy, dx + dy, x (dw, db)
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

DEV = "cuda:0"


def _time(fn, iters=10, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def kernel_table(batch, size, hbm_tbs):
    from mmskin import ops
    rows = []
    for i, C in enumerate((64, 128, 320, 512)):
        H = W = size // (4 << i)
        N, Ch = 1 + H * W, C // 8
        qkv = torch.randn(batch, N, 3, 8, Ch, device=DEV, requires_grad=True)
        ws = [torch.randn(n * Ch, 1, k, k, device=DEV, requires_grad=True) for k, n in ((3, 2), (5, 3), (7, 3))]
        bs = [torch.randn(n * Ch, device=DEV, requires_grad=True) for n in (2, 3, 3)]
        dO = torch.randn(batch, N, C, device=DEV)
        x = torch.randn(batch, N, C, device=DEV, requires_grad=True)
        cw = torch.randn(C, 1, 3, 3, device=DEV, requires_grad=True)
        cb = torch.randn(C, device=DEV, requires_grad=True)
        T, X = batch * N * 3 * C * 4, batch * N * C * 4

        def fwd_bwd(op, grad):
            y = op()
            t_f = _time(op)
            t_fb = _time(lambda: op().backward(grad))
            del y
            return t_f, t_fb - t_f

        fa_f, fa_b = fwd_bwd(lambda: ops.factor_attention(qkv, H, W, ws, bs), dO)
        pe_f, pe_b = fwd_bwd(lambda: ops.conv_pos_enc_tokens(x, H, W, cw, cb), dO)
        for name, t, floor in (("factor_attention fwd", fa_f, 5 / 3 * T), ("factor_attention bwd", fa_b, 4 * T),
                               ("conv_pos_enc_tokens fwd", pe_f, 2 * X), ("conv_pos_enc_tokens bwd", pe_b, 5 * X)):
            floor_us = floor / (hbm_tbs * 1e12) * 1e6
            rows.append({"stage": i + 1, "H": H, "Ch": Ch, "kernel": name, "us": round(t * 1e6, 1), "floor_us": round(floor_us, 1),
                         "x_floor": round(t * 1e6 / floor_us, 2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--hbm-tbs", type=float, default=4.0, help="achievable HBM bandwidth the floors are quoted at, TB/s")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    from mmskin import ops
    from mmskin.optim import Adam
    from models import multimodalIntraInterModal as M
    for row in kernel_table(args.batch, args.size, args.hbm_tbs):
        print(json.dumps(row))
    if args.no_step:
        return
    ops.set_linear_dtype("bf16")
    torch.manual_seed(0)
    model = M.MultimodalModel(num_classes=6, num_heads=8, device=DEV, cnn_model_name="coat_lite_small.in1k",
                              text_model_name="one-hot-encoder", vocab_size=85, unfreeze_weights="unfrozen_weights",
                              attention_mecanism="att-intramodal+residual+cross-attention-metadados").to(DEV).train()
    opt = Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    img = torch.randn(args.batch, 3, args.size, args.size, device=DEV)
    meta = torch.randn(args.batch, 85, device=DEV)
    lab = torch.randint(0, 6, (args.batch,), device=DEV)

    def step():
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(model(img, meta), lab).backward()
        opt.step()

    dt = _time(step, args.steps, args.warmup)
    print(json.dumps({"workload": "coat_lite_small multimodal train step", "batch": args.batch, "size": args.size,
                      "ms_per_step": round(dt * 1e3, 3), "img_per_s": round(args.batch / dt, 1)}))


if __name__ == "__main__":
    main()
