"""Conformal-study timing: ConformalPredictor.study with C = 6 at N = 2298 (PAD-UFES-20) and a fold ten times that size, with
R = 2000 and R = 8192 random splits.

    python scripts/conformal_bench.py [--shapes 2298:6 22980:6] [--resamples 2000 8192] [--score aps] [--mondrian] [--stratified]
                                      [--numpy-replicates 50] [--runs 5] [--warmup 2]

Per (shape, R), each figure the median of repeated runs after warm-ups, from device events (inputs are already on the device, every
run writes into buffers of its own):
  scored       the score pass and the per-fold tables (two device sorts): once per study
  replicates   mmskin_conformal_study on all R replicates: the hot path, one workgroup per replicate
  finalize     mmskin_conformal_finalize: the metric columns, the sorted columns and the summary
  study        ConformalPredictor.study from device tensors to the host report (all of the above and the copies)
  numpy        tests/conformal_oracle.study, the host restatement (one sort per split), timed by the wall clock on
               `--numpy-replicates` replicates and SCALED to R -- an extrapolation, labelled so; its integers are compared with the
               kernel's.  The parent commit has no function to compare with.
Needs a GPU: no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "multimodal-model-skin-lesion-classifier_amd"), os.path.join(ROOT, "tests")):
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


def fold(N, C, rng):
    z = rng.normal(size=(N, C)) * 2.0
    e = np.exp(z - z.max(axis=1, keepdims=True))
    probs = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    labels = (rng.random(N)[:, None] > np.cumsum(probs.astype(np.float64), axis=1)).sum(axis=1).clip(0, C - 1)
    return probs, labels.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["2298:6", "22980:6"])
    ap.add_argument("--resamples", nargs="+", type=int, default=[2000, 8192])
    ap.add_argument("--score", default="aps")
    ap.add_argument("--mondrian", action="store_true")
    ap.add_argument("--stratified", action="store_true")
    ap.add_argument("--numpy-replicates", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conformal_bench: no GPU visible; this measurement has no CPU fallback")
    import conformal_oracle as co
    from mmskin import conformal
    from mmskin._lib import call, ptr, stream
    from mmskin.ops import bootstrap_quantiles

    rng = np.random.default_rng(0)
    cp = conformal.ConformalPredictor(alpha=0.1, score=args.score, mondrian=args.mondrian)
    flags = (conformal.STRATIFIED if args.stratified else 0) | (conformal.MONDRIAN if args.mondrian else 0)
    keep = [None]
    for shape in args.shapes:
        N, C = (int(v) for v in shape.split(":"))
        probs, labels = fold(N, C, rng)
        pd, yd = torch.from_numpy(probs).to(DEV), torch.from_numpy(labels).to(DEV)
        n_cal = N // 2
        take = torch.from_numpy(conformal.cal_counts(labels, C, n_cal).astype(np.int32)).to(DEV) if args.stratified else None
        for R in args.resamples:
            out = {"what": "conformal_study", "rows": N, "classes": C, "n_cal": n_cal, "resamples": R, "score": args.score,
                   "mondrian": args.mondrian, "stratified": args.stratified, "device": torch.cuda.get_device_name(0)}
            out["scored"] = stats(timed(lambda i: keep.__setitem__(0, cp._scored(pd, yd, 0, R)), args.warmup, args.runs))
            workspace, order, members, class_start = keep[0]
            outs = [(torch.empty((R, C), dtype=torch.float64, device=DEV), torch.empty((R, 8 + 5 * C), dtype=torch.int64, device=DEV))
                    for _ in range(args.warmup + args.runs)]
            run = lambda i: call("mmskin_conformal_study", 0, N, C, R, n_cal, cp.alpha, flags, ptr(yd), ptr(order), ptr(members),
                                 ptr(class_start), ptr(take), 0, R, ptr(workspace), ptr(outs[i][0]), ptr(outs[i][1]), stream())
            out["replicates"] = stats(timed(run, args.warmup, args.runs))
            qhat, counts = outs[-1]
            summaries = [torch.empty((5, 6 + 2 * C), dtype=torch.float64, device=DEV) for _ in range(args.warmup + args.runs)]
            q_lo, q_hi = bootstrap_quantiles(0.95)
            out["finalize"] = stats(timed(lambda i: call("mmskin_conformal_finalize", ptr(counts), ptr(qhat), N, C, R, q_lo, q_hi, ptr(workspace),
                                                         ptr(summaries[i]), stream()), args.warmup, args.runs))
            out["study"] = stats(timed(lambda i: keep.__setitem__(0, cp.study(pd, yd, n_resamples=R, seed=0, stratified=args.stratified)),
                                       args.warmup, args.runs))
            rep = keep[0]
            reps = min(args.numpy_replicates, R)
            t0 = time.perf_counter()
            want_q, want_counts = co.study(probs, labels, cp.score, cp.alpha, n_cal, reps, 0, cp.randomized, cp.lam, cp.k_reg, cp.mondrian,
                                           args.stratified)
            wall = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(rep.counts[:reps], want_counts) and np.array_equal(rep.qhat[:reps], want_q), "the restatement and the kernel disagree"
            out["numpy"] = {"ms": round(wall * R / reps, 1), "scaled": True, "timed_replicates": reps,
                            "note": f"the numpy restatement timed on {reps} replicates by the wall clock, EXTRAPOLATED to {R}"}
            out["replicates_us_each"] = round(out["replicates"]["median_ms"] * 1e3 / R, 3)
            out["coverage"] = [rep.point["coverage"], rep.summary["mean"]["coverage"], rep.summary["low"]["coverage"], rep.summary["high"]["coverage"]]
            out["mean_set_size"] = [rep.point["mean_set_size"], rep.summary["mean"]["mean_set_size"]]
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
