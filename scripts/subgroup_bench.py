"""Subgroup-audit timing on two folds: N = 460, K = 6, G = 6 (a PAD-UFES-20 validation fold by Fitzpatrick type) and N = 5000,
K = 8, G = 16 (an ISIC-2019 one), B = 2000 replicates each, beside the plain bootstrap of the same fold.

    python scripts/subgroup_bench.py [--shapes 460:6:6 5000:8:16] [--resamples 2000] [--groups-sweep 1 2 4 8 16] [--runs 5] [--warmup 2]

Per shape, each figure the median of repeated runs after warm-ups, from device events (the event pair brackets finished work on the
stream; inputs are already on the device):
  prep                  mmskin.ops.subgroup_tables: the per-class sorts by (group, score), tie groups, group and member lists
  replicates            mmskin.ops.subgroup_replicates on all B replicates with G groups: the hot path, one workgroup per replicate
  bootstrap_replicates  mmskin.ops.bootstrap_replicates on the same fold and B: what ONE ungrouped bootstrap costs
  ratio                 replicates / bootstrap_replicates: G groups should cost about one bootstrap, not G of them
  finalize, gaps        mmskin.ops.subgroup_finalize (G (7 + 4 K) sorted columns) and mmskin.ops.subgroup_gaps
  audit                 SubgroupAudit.evaluate from device tensors to the host result (the fold with one group AND the G groups:
                        two studies, their point estimates, finalize, gaps and the copies)
  bootstrap_evaluate    BootstrapMetrics.evaluate on the same fold, for the same comparison end to end
  by_groups             the replicates kernel alone with the rows dealt into G = 1, 2, 4, ... groups: does the cost grow with G?
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


def fold(N, K, G, rng):
    labels = rng.integers(0, K, N).astype(np.int64)
    raw = rng.random((N, K)) + 0.8 * np.eye(K)[labels]
    share = rng.random(G) + 0.3                                       # uneven groups, as skin types are
    groups = rng.choice(G, N, p=share / share.sum()).astype(np.int32)
    groups[rng.random(N) < 0.05] = -1                                 # some rows without the attribute
    return (raw / raw.sum(axis=1, keepdims=True)).astype(np.float32), labels, groups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["460:6:6", "5000:8:16"])
    ap.add_argument("--resamples", type=int, default=2000)
    ap.add_argument("--groups-sweep", type=int, nargs="*", default=[1, 2, 4, 8, 16])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("subgroup_bench: no GPU visible; this measurement has no CPU fallback")
    from mmskin import ops
    from mmskin.bootstrap import BootstrapMetrics
    from mmskin.subgroup import SubgroupAudit

    rng = np.random.default_rng(0)
    B, mode = args.resamples, ops.BOOTSTRAP_PLAIN
    keep = [None]
    for shape in args.shapes:
        N, K, G = (int(v) for v in shape.split(":"))
        scores, labels, groups = fold(N, K, G, rng)
        sd, yd, gd = (torch.from_numpy(a).to(DEV) for a in (scores, labels, groups))
        out = {"what": "subgroup_audit", "rows": N, "classes": K, "groups": G, "resamples": B, "device": torch.cuda.get_device_name(0)}
        out["prep"] = stats(timed(lambda i: keep.__setitem__(0, ops.subgroup_tables(sd, yd, gd, G)), args.warmup, args.runs))
        tables = keep[0]
        conf, counts = ops.subgroup_accumulators(B, G, K, DEV)
        out["replicates"] = stats(timed(lambda i: ops.subgroup_replicates(tables, i, mode, conf, counts), args.warmup, args.runs))
        plain = ops.bootstrap_tables(sd, yd)
        pconf, pcounts = ops.bootstrap_accumulators(B, K, DEV)
        out["bootstrap_replicates"] = stats(timed(lambda i: ops.bootstrap_replicates(plain, i, mode, pconf, pcounts), args.warmup, args.runs))
        out["ratio"] = round(out["replicates"]["median_ms"] / out["bootstrap_replicates"]["median_ms"], 3)
        out["finalize"] = stats(timed(lambda i: keep.__setitem__(0, ops.subgroup_finalize(conf, counts)), args.warmup, args.runs))
        metrics = keep[0][0]
        out["gaps"] = stats(timed(lambda i: keep.__setitem__(0, ops.subgroup_gaps(metrics)), args.warmup, args.runs))
        audit, bs = SubgroupAudit(B, seed=0), BootstrapMetrics(B, seed=0)
        out["audit"] = stats(timed(lambda i: keep.__setitem__(0, audit.evaluate(sd, yd, gd)), args.warmup, args.runs))
        res = keep[0]
        out["bootstrap_evaluate"] = stats(timed(lambda i: bs.evaluate(sd, yd), args.warmup, args.runs))
        out["audit_ratio"] = round(out["audit"]["median_ms"] / out["bootstrap_evaluate"]["median_ms"], 3)
        sweep = {}
        for g in args.groups_sweep:
            if g > ops.SUBGROUP_MAX_GROUPS or g * K * K > ops.SUBGROUP_MAX_CELLS:
                continue
            t = ops.subgroup_tables(sd, yd, torch.arange(N, device=DEV, dtype=torch.int32) % g, g)
            c, n = ops.subgroup_accumulators(B, g, K, DEV)
            sweep[str(g)] = stats(timed(lambda i: ops.subgroup_replicates(t, i, mode, c, n), args.warmup, args.runs))["median_ms"]
        out["by_groups"] = sweep
        out["balanced_accuracy_gap"] = [res.gap.point["balanced_accuracy"], *res.gap.interval("balanced_accuracy")]
        out["balanced_accuracy_overall"] = [res.overall.point["balanced_accuracy"], *res.overall.interval("balanced_accuracy")]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
