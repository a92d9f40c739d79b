"""Metadata-Shapley timing at the reference's setting (shap's permutation explainer: 10 antithetic permutations, 100 background
rows) on the PAD-UFES-20 column layout, 18 categorical + 3 numeric columns = 21 players, 40 101 head rows per explained sample:
densenet169 + gfcam (the configuration of the reference's interpretability scripts) and the headline ResNet-50 + crossattention.

    python scripts/shapley_bench.py [--configs densenet169:gfcam resnet-50:crossattention] [--batch 2] [--rows 8192]
                                    [--background 100] [--permutations 10] [--baseline-rows 256] [--runs 5] [--warmup 2]

Per configuration, each figure the median of repeated runs after warm-ups, from device events (every timed call ends with its
result on the device; the event pair brackets finished work), as time PER EXPLAINED SAMPLE:
  shapley      mmskin.shapley.MetadataShapley.explain: one image encoding per batch, the coalitions kernel, the fusion head in
               `rows` blocks, the reduce kernels
  torch_rows   what a user can do with encode_image / fuse but without the kernels: the image encoded once, the coalition rows
               mixed from the encoded explained and background rows with torch.where, model.fuse in the same blocks, soft-max
               and the background means in torch
  baseline     the straightforward loop on the public API, model(image, row) at the reference's batch 1, one forward per
               coalition row -- timed on `--baseline-rows` rows and SCALED to the sample's row count (the output says so)
  head_rows_per_s   rows of one `rows`-sized model.fuse call over its time
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
# PAD-UFES-20-like encoder: 18 categorical columns (ten booleans with "EMPTY", gender, region, ...) and 3 numerics: 88 columns,
# padded to the checkpoint's 91
CATEGORIES = [["EMPTY", "False", "True"]] * 10 + [["EMPTY", "FEMALE", "MALE"]] + [[f"REGION{i}" for i in range(14)] + ["EMPTY"]] + \
             [[f"V{i}" for i in range(5)] + ["EMPTY"]] * 5 + [["EMPTY", "False", "True"]]
N_NUM, VOCAB = 3, 91


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
    ap.add_argument("--background", type=int, default=100)
    ap.add_argument("--permutations", type=int, default=10)
    ap.add_argument("--baseline-rows", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("shapley_bench: no GPU visible; this measurement has no CPU fallback")
    from mmskin import ops
    from mmskin.preprocess import MetadataEncoder
    from mmskin.shapley import MetadataShapley
    from models import multimodalIntraInterModal as M

    enc = MetadataEncoder()
    enc.categories_ = [np.array(c, dtype=object) for c in CATEGORIES]
    enc.mean_, enc.scale_ = np.array([55.0, 9.0, 7.0]), np.array([18.0, 6.0, 5.0])
    rng = np.random.default_rng(0)
    B, G, P, hw = args.batch, args.background, args.permutations, args.size
    draw = lambda n: (torch.from_numpy(np.stack([rng.integers(0, len(c), n) for c in CATEGORIES], axis=1).astype(np.int32)).to(DEV),
                      torch.from_numpy(rng.uniform(1, 90, (n, N_NUM)).astype(np.float32)).to(DEV))
    codes, numeric = draw(B)
    bg_codes, bg_numeric = draw(G)
    n_players = len(CATEGORIES) + N_NUM
    keep = [None, None]

    for config in args.configs:
        cnn, fusion = config.split(":")
        torch.manual_seed(0)
        model = M.MultimodalModel(num_classes=6, num_heads=8, device=DEV, cnn_model_name=cnn, text_model_name="one-hot-encoder",
                                  vocab_size=VOCAB, attention_mecanism=fusion, n=2).to(DEV).eval()
        images = torch.randn(B, 3, hw, hw, device=DEV)
        ex = MetadataShapley(model, enc, DEV, bg_codes, bg_numeric, n_permutations=P, seed=0, rows_per_head_call=args.rows)
        per_sample = ex.rows_per_sample()
        step = ex.rows_per_head_call
        out = {"what": "metadata_shapley", "encoder": cnn, "fusion": fusion, "batch": B, "height": hw, "width": hw, "players": n_players,
               "background": G, "permutations": P, "rows_per_sample": per_sample, "rows_per_head_call": step,
               "device": torch.cuda.get_device_name(0), "backbone_dtype": model.image_encoder.compute_dtype,
               "linear_dtype": ops.get_linear_dtype()}

        ms = timed(lambda i: keep.__setitem__(0, ex.explain(images, codes, numeric)), args.warmup, args.runs)
        out["shapley_per_sample"] = stats(ms, per=B)
        values = keep[0].values.clone()

        # the same rows without the kernels: cells of the encoded explained row or of the encoded background row, by coalition
        K = 2 * P * (n_players - 1)
        off = np.concatenate([[0], np.cumsum([len(c) for c in CATEGORIES])])
        cell_player = np.concatenate([np.repeat(np.arange(len(CATEGORIES)), np.diff(off)), len(CATEGORIES) + np.arange(N_NUM),
                                      np.zeros(VOCAB - off[-1] - N_NUM, dtype=np.int64)])
        masks = np.zeros((K + 1, n_players), dtype=bool)                    # interior coalitions in the walk's order, then the empty one
        for p, perm in enumerate(ex.permutations):
            for side in (0, 1):
                for n in range(1, n_players):
                    masks[(p * 2 + side) * (n_players - 1) + n - 1, perm[:n] if side == 0 else perm[n_players - n:]] = True
        cell_mask = torch.from_numpy(masks[:, cell_player]).to(DEV)          # [K + 1, VOCAB]
        pad = lambda t: torch.nn.functional.pad(t, (0, VOCAB - t.shape[1]))
        x_enc, bg_enc = pad(enc.transform(codes, numeric)), pad(enc.transform(bg_codes, bg_numeric))
        blocks = max(step // G, 1)                                           # coalitions per head call

        def torch_rows(i):
            with torch.no_grad():
                feat = model.encode_image(images)
                v = []
                for b in range(B):
                    for k0 in range(0, K + 1, blocks):
                        m = cell_mask[k0:k0 + blocks]
                        rows = torch.where(m[:, None, :], x_enc[b][None, None, :], bg_enc[None, :, :]).reshape(-1, VOCAB)
                        logits = model.fuse(feat[b:b + 1].expand(rows.shape[0], -1).contiguous(), rows).float()
                        v.append(torch.softmax(logits, dim=-1).reshape(-1, G, logits.shape[-1]).double().mean(dim=1))
                keep[1] = (torch.cat(v), torch.softmax(model.fuse(feat, x_enc).float(), dim=-1))

        out["torch_rows_per_sample"] = stats(timed(torch_rows, args.warmup, args.runs), per=B)
        base_check = float((keep[1][0].reshape(B, K + 1, -1)[:, K].float() - keep[0].base).abs().max())
        out["torch_rows_base_max_abs_diff"] = base_check

        n_base = min(args.baseline_rows, per_sample)
        metas = ops.shapley_coalitions(codes[:1].contiguous(), numeric[:1].contiguous(), bg_codes, bg_numeric, off.astype(np.int32),
                                       *enc._tables(DEV)[1:], enc.nan_fill, ex.permutations, VOCAB, row0=0, row1=n_base)

        def baseline(i):
            with torch.no_grad():
                keep[1] = torch.cat([torch.softmax(model(images[:1], metas[r:r + 1]).float(), dim=-1) for r in range(n_base)])

        base_ms = timed(baseline, 1, max(args.runs // 2, 1))
        scale = per_sample / n_base
        out["baseline_per_sample"] = dict(stats([m * scale for m in base_ms]), scaled=True, timed_rows=n_base,
                                          note=f"batch-1 forwards timed on {n_base} rows, scaled to {per_sample}")
        with torch.no_grad():
            out["encode_image"] = stats(timed(lambda i: keep.__setitem__(1, model.encode_image(images)), args.warmup, args.runs))
            feats = keep[1][:1].expand(step, -1).contiguous()
            block = ops.shapley_coalitions(codes, numeric, bg_codes, bg_numeric, off.astype(np.int32), *enc._tables(DEV)[1:], enc.nan_fill,
                                           ex.permutations, VOCAB, row0=0, row1=step)
            head = timed(lambda i: keep.__setitem__(1, model.fuse(feats, block)), args.warmup, args.runs)
        out["head_call"] = stats(head)
        out["head_rows_per_s"] = round(step / (statistics.median(head) * 1e-3))
        out["speedup_vs_baseline"] = round(out["baseline_per_sample"]["median_ms"] / out["shapley_per_sample"]["median_ms"], 1)
        out["speedup_vs_torch_rows"] = round(out["torch_rows_per_sample"]["median_ms"] / out["shapley_per_sample"]["median_ms"], 2)
        out["max_abs_value"] = float(values.abs().max())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
