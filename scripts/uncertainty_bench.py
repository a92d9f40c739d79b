"""Predictive-uncertainty timing: PredictiveUncertainty.mc_dropout (32 passes) and .tta (8 views) on densenet169 + gfcam at batch 64,
against the way a user would do the same without the feature, and the three kernels of csrc/uncertainty.hip alone.

    python scripts/uncertainty_bench.py [--batch 64] [--size 224] [--passes 32] [--rows 2048 16384] [--runs 5] [--warmup 2]

Each figure is the median of repeated runs after warm-ups, from device events (inputs are already on the device):
  mc_dropout        pu.mc_dropout: one encoder pass, the fusion head on passes x batch rows, the reduce kernel
  mc_dropout_loop   without the feature: `passes` whole model(images, metadata) calls with the head's dropouts switched on by hand,
                    and the statistics (mean, std, entropies, mutual information, votes) by torch ops on the stacked logits
  tta               pu.tta with the 8 dihedral views: one views kernel, the model on 8 x batch images, the reduce kernel
  tta_loop          without the feature: 8 model calls on torch.rot90 / torch.flip views, the same torch statistics
  views             mmskin.ops.dihedral_views alone on the batch (fp32, 8 views), with its bytes read + written and the rate
  reduce            mmskin.ops.uncertainty_reduce alone on [passes, rows, 6] logits at the fold sizes of --rows
  risk_coverage     mmskin.ops.risk_coverage + risk_coverage_summary alone at those fold sizes (the ranking holds <= 16384 rows)
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


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def torch_statistics(logits):
    """the statistics of uncertainty_reduce by torch ops, fp64, on logits [T, B, C]"""
    p = torch.softmax(logits.double(), dim=-1)
    mean = p.mean(dim=0)
    ent = lambda q: -(q * torch.log(q.clamp_min(1e-300))).sum(dim=-1)
    h_mean, h_exp = ent(mean), ent(p).mean(dim=0)
    votes = torch.nn.functional.one_hot(logits.argmax(dim=-1), logits.shape[-1]).sum(dim=0)
    top2 = mean.topk(2, dim=-1).values
    return mean, p.std(dim=0, unbiased=False), votes, mean.argmax(dim=-1), torch.stack(
        [top2[:, 0], top2[:, 0] - top2[:, 1], h_mean, h_exp, (h_mean - h_exp).clamp_min(0), 1.0 - votes.max(dim=-1).values / logits.shape[0]], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--passes", type=int, default=32)
    ap.add_argument("--rows", type=int, nargs="+", default=[2048, 16384])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("uncertainty_bench: no GPU visible; this measurement has no CPU fallback")
    from mmskin import ops
    from mmskin.uncertainty import PredictiveUncertainty, mc_dropout_mode
    from models import multimodalIntraInterModal as M

    torch.manual_seed(0)
    B, hw, T = args.batch, args.size, args.passes
    model = M.MultimodalModel(num_classes=6, num_heads=8, device=DEV, cnn_model_name="densenet169", text_model_name="one-hot-encoder",
                              vocab_size=VOCAB, attention_mecanism="gfcam", n=2).to(DEV).eval()
    images = torch.randn(B, 3, hw, hw, device=DEV)
    meta = torch.randn(B, VOCAB, device=DEV)
    pu = PredictiveUncertainty(model, DEV)
    keep = [None]
    out = {"what": "predictive_uncertainty", "model": "densenet169+gfcam", "batch": B, "size": hw, "passes": T,
           "device": torch.cuda.get_device_name(0)}

    def mc(i):
        pu.reset()
        keep[0] = pu.mc_dropout(images, meta, passes=T, seed=i)

    def mc_loop(i):
        with torch.no_grad(), mc_dropout_mode(model):
            logits = torch.stack([model(images, meta).float() for _ in range(T)])
        keep[0] = torch_statistics(logits)

    def tta(i):
        pu.reset()
        keep[0] = pu.tta(images, meta, views="dihedral")

    def tta_loop(i):
        with torch.no_grad():
            views = []
            for v in range(8):
                y = torch.rot90(images, v & 3, (2, 3))
                views.append(model((torch.flip(y, (3,)) if v & 4 else y).contiguous(), meta).float())
        keep[0] = torch_statistics(torch.stack(views))

    out["mc_dropout"] = stats(timed(mc, args.warmup, args.runs))
    out["mc_dropout_loop"] = stats(timed(mc_loop, args.warmup, args.runs))
    out["mc_dropout_speedup"] = round(out["mc_dropout_loop"]["median_ms"] / out["mc_dropout"]["median_ms"], 2)
    out["tta"] = stats(timed(tta, args.warmup, args.runs))
    res = keep[0]
    out["tta_loop"] = stats(timed(tta_loop, args.warmup, args.runs))
    out["tta_speedup"] = round(out["tta_loop"]["median_ms"] / out["tta"]["median_ms"], 2)
    want = keep[0]
    out["tta_vs_loop_max_prob_diff"] = float((res.mean_prob - want[0]).abs().max())      # 256-image calls against 64-image calls
    assert out["tta_vs_loop_max_prob_diff"] <= 1e-2, "tta and the torch loop disagree"
    stack = torch.empty((8, B, 3, hw, hw), device=DEV)
    out["views"] = stats(timed(lambda i: ops.dihedral_views(images, 0xFF, out=stack), args.warmup, args.runs))
    moved = 9 * images.numel() * 4
    out["views"].update(bytes=moved, gb_per_s=round(moved / (out["views"]["median_ms"] * 1e6), 1))
    print(json.dumps(out), flush=True)

    for N in args.rows:
        g = torch.Generator().manual_seed(N)
        logits = (3.0 * torch.randn(T, N, 6, generator=g)).to(DEV)
        row = {"what": "uncertainty_kernels", "rows": N, "classes": 6, "passes": T}
        row["reduce"] = stats(timed(lambda i: keep.__setitem__(0, ops.uncertainty_reduce(logits)), args.warmup, args.runs))
        mean, _, _, pred, st = keep[0]
        row["reduce_torch"] = stats(timed(lambda i: keep.__setitem__(0, torch_statistics(logits)), args.warmup, args.runs))
        assert float((mean - keep[0][0]).abs().max()) <= 1e-12, "the reduce kernel and torch disagree"
        if N <= ops.RISK_COVERAGE_MAX_ROWS:
            labels = torch.randint(0, 6, (N,), generator=g).to(DEV)
            wrong = (pred.long() != labels).to(torch.uint8)
            score = st[:, 4].contiguous()
            row["risk_coverage"] = stats(timed(lambda i: keep.__setitem__(0, ops.risk_coverage(score, wrong)), args.warmup, args.runs))
            counts = keep[0]
            row["risk_coverage_summary"] = stats(timed(lambda i: keep.__setitem__(0, ops.risk_coverage_summary(counts, wrong)), args.warmup,
                                                       args.runs))
            row["aurc"] = float(keep[0][0])
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
