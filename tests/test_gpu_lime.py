"""-m gpu: the metadata-LIME kernels (csrc/lime.hip) against their numpy restatement (tests/lime_oracle.py, held to sklearn by
tests/test_cpu_lime.py), and mmskin.lime.MetadataLime end to end against the restatement driven by the model's own fusion head."""
import os

import numpy as np
import pytest
import torch

import lime_oracle as lo
import sweep_oracle as so
from gpu_util import DEV
from helpers import SMALL
from mmskin import ops
from mmskin._lib import MMSkinError, call, ptr, stream
from mmskin.lime import MetadataLime
from models import multimodalIntraInterModal as M
from oracle.detinit import det_init_
from oracle.model import OracleMultimodalModel

pytestmark = pytest.mark.gpu

SENTINEL = -77.0

# (F, columns past F, N, B, seed): a partial tile, odd sizes, the cap; one and several slabs of 256 rows; one and several samples
NEIGHBOUR_CASES = [(5, 0, 64, 1, 1), (5, 3, 257, 3, 2), (21, 3, 64, 3, 3), (21, 0, 257, 1, 4), (91, 0, 5000, 1, 5), (91, 3, 257, 3, 6),
                   (128, 3, 64, 1, 7), (128, 0, 257, 3, 8)]
# Largest |z(float32 rows) - z(float64 rows)| / max(1, |z|) over NEIGHBOUR_CASES, both centres, with the restatement run in float32
# and in float64 on the same counters on the CPU (tests/test_cpu_lime.py::test_float32_rows_stay_within_the_recorded_error_of_float64
# prints the figure per case and asserts it): the float32 Box-Muller's and the float32 row's own error.  The device's logf / cosf are
# a few ulp looser than libm's, so the kernel is allowed NORMAL_KERNEL_FACTOR times it.
NORMAL_F32_ERROR = 1.4780e-06
NORMAL_KERNEL_FACTOR = 8.0

# (F, columns past F, N, B, C, K): K = 7, 15 and F; two and six classes; N below, at and far above a slab
SOLVE_CASES = [(5, 0, 64, 1, 2, 5), (21, 3, 257, 3, 6, 7), (21, 0, 64, 1, 2, 15), (91, 0, 5000, 1, 6, 15), (91, 3, 257, 3, 2, 91),
               (128, 3, 257, 3, 6, 15), (128, 0, 64, 1, 6, 7)]
SOLVE_TOL = 1e-9


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# --------------------------------------------------------------------------------------------------------- neighbourhood
@pytest.mark.parametrize("F,extra,N,B,seed", NEIGHBOUR_CASES)
def test_neighbourhood_kernel(F, extra, N, B, seed):
    mean, scale, x = lo.case_stats(F, seed)
    x, width, total = x[:B], F + extra, B * N
    xd, md, sd = dev(x), dev(mean), dev(scale)
    for around in (False, True):
        buf = torch.full((total + 2, width), SENTINEL, device=DEV)               # one guard row on either side of the output
        wbuf = torch.full((total + 2,), SENTINEL, device=DEV, dtype=torch.float64)
        rows, w = ops.lime_neighbourhood(xd, md, sd, N, seed, out_width=width, sample0=3, around_instance=around, out=buf[1:total + 1],
                                         weights=wbuf[1:total + 1])
        torch.cuda.synchronize()
        host, whost = buf.cpu().numpy(), wbuf.cpu().numpy()
        assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all() and whost[0] == SENTINEL and whost[-1] == SENTINEL
        got, gw = host[1:-1].reshape(B, N, width), whost[1:-1].reshape(B, N)
        assert np.array_equal(got[:, 0, :F].view(np.uint32), x.view(np.uint32)), "row 0 is not x bit for bit"
        assert not got[..., F:].any() and np.isfinite(got).all()
        # the draws against the float64 Box-Muller
        want = lo.standardise(lo.neighbourhood(x, mean, scale, N, seed, sample0=3, around=around, dt=np.float64), mean, scale)
        z = lo.standardise(got, mean, scale)
        err = float((np.abs(z - want) / np.maximum(1.0, np.abs(want))).max())
        print(f"F {F} N {N} B {B} around {around}: max |dz| / max(1, |z|) against float64 {err:.4e}, bound "
              f"{NORMAL_KERNEL_FACTOR * NORMAL_F32_ERROR:.4e}")
        assert err <= NORMAL_KERNEL_FACTOR * NORMAL_F32_ERROR
        # the weights from the device's own rows, fp64 and fp32
        ww = lo.kernel_weights(got, mean, scale)
        assert (gw[:, 0] == 1.0).all() and np.abs(gw / ww - 1).max() <= 1e-6
        _, w32 = ops.lime_neighbourhood(xd, md, sd, N, seed, out_width=width, sample0=3, around_instance=around, weight_dtype=torch.float32)
        assert w32.dtype == torch.float32 and np.abs(w32.cpu().numpy().reshape(B, N) / ww - 1).max() <= 1e-6
        # cut at three uneven places: each call writes its rows only, together they are the full write bit for bit
        cuts = sorted({1, total // 3 + 1, total - 5})
        edges = [0, *[c for c in cuts if 0 < c < total], total]
        buf2, wbuf2 = torch.full_like(buf, SENTINEL), torch.full_like(wbuf, SENTINEL)
        for r0, r1 in reversed(list(zip(edges[:-1], edges[1:]))):
            ops.lime_neighbourhood(xd, md, sd, N, seed, out_width=width, sample0=3, around_instance=around, row0=r0, row1=r1,
                                   out=buf2[1 + r0:1 + r1], weights=wbuf2[1 + r0:1 + r1])
            torch.cuda.synchronize()
            assert bool((buf2[:1 + r0] == SENTINEL).all()) and bool((wbuf2[:1 + r0] == SENTINEL).all())
        assert torch.equal(buf2, buf) and torch.equal(wbuf2, wbuf)
    other, _ = ops.lime_neighbourhood(xd, md, sd, N, seed, out_width=width, sample0=4)
    assert not torch.equal(other, rows)                                          # another sample offset: other draws


# --------------------------------------------------------------------------------------------------------- reduce + solve
def run_fit(rows, w, logits, x, mean, scale, B, N, C, K, output, cuts=(), abs_sum=None):
    F = mean.shape[0]
    acc = ops.lime_accumulator(B, N, F, C, DEV)
    edges = [0, *cuts, B * N]
    for r0, r1 in zip(edges[:-1], edges[1:]):
        ops.lime_reduce(rows[r0:r1], w[r0:r1], logits[r0:r1].contiguous(), mean, scale, acc, B, N, r0, output=output)
    out = ops.lime_solve(acc, x, mean, scale, N, C, K, abs_sum=abs_sum)
    return dict(zip(("coef", "feature", "intercept", "score", "local_pred", "dense"), (t.cpu().numpy() for t in out)))


@pytest.mark.parametrize("F,extra,N,B,C,K", SOLVE_CASES)
def test_reduce_and_solve_kernels(F, extra, N, B, C, K):
    seed = 100 + F + N + C
    mean, scale, x = lo.case_stats(F, seed)
    x, width, total = x[:B], F + extra, B * N
    xd, md, sd = dev(x), dev(mean), dev(scale)
    rows, w = ops.lime_neighbourhood(xd, md, sd, N, seed, out_width=width)
    rows_host = rows.cpu().numpy().reshape(B, N, width)
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 1, (total, C))
    m = min(C, F)
    logits[:, :m] += 1.5 * lo.standardise(rows_host, mean, scale).reshape(total, F)[:, :m]      # the targets depend on the features
    cuts = [c for c in sorted({1, total // 3 + 7, total - 5}) if 0 < c < total]
    for output in (lo.PROB, lo.LOGIT):
        for dtype in (torch.float32, torch.bfloat16):
            lg = torch.from_numpy(logits).float().to(DEV).to(dtype)
            want = lo.explain_batch(rows_host, lg.float().cpu().numpy().reshape(B, N, C), mean, scale, K, output)      # bf16: the rounded values
            assert want["gap"].min() > 1e-6, "the oracle's K-th and (K+1)-th |beta0 z0| tie: choose another seed"
            acc_abs = torch.zeros((F, C), dtype=torch.float64, device=DEV)
            got = run_fit(rows, w, lg, xd, md, sd, B, N, C, K, output, abs_sum=acc_abs)
            assert got["coef"].shape == (B, C, K) and got["feature"].dtype == np.int32
            assert np.array_equal(np.sort(got["feature"], -1), np.sort(want["feature"], -1)), "the selected feature sets differ"
            assert np.array_equal(got["feature"], want["feature"])
            for key in ("coef", "intercept", "local_pred", "score", "dense"):
                err = float((np.abs(got[key] - want[key]) / np.maximum(1.0, np.abs(want[key]))).max())
                print(f"F {F} N {N} B {B} C {C} K {K} output {output} {dtype}: {key} against the oracle {err:.3e}")
                assert err <= SOLVE_TOL, key
            want_abs = np.zeros((F, C))
            for b in range(B):
                want_abs += np.abs(got["dense"][b]).T
            assert np.array_equal(acc_abs.cpu().numpy(), want_abs)
            # rows reduced in uneven chunks, and a second run: bitwise equal
            for again in (run_fit(rows, w, lg, xd, md, sd, B, N, C, K, output, cuts=cuts), run_fit(rows, w, lg, xd, md, sd, B, N, C, K, output)):
                for key in got:
                    assert np.array_equal(got[key], again[key]), key
    # fp32 weights: the same fits up to the weights' rounding
    got32 = run_fit(rows, w.float(), lg, xd, md, sd, B, N, C, K, output)
    assert np.array_equal(got32["feature"], got["feature"]) and np.abs(got32["coef"] - got["coef"]).max() <= 1e-5


def test_a_duplicated_column_still_solves():
    """two identical columns make G singular: alpha = 0.01 of the selection fit is what keeps its factorisation positive"""
    F, N, B, C = 21, 257, 1, 2
    mean, scale, x = lo.case_stats(F, 9)
    mean[4], scale[4], x[:, 4] = mean[3], scale[3], x[:, 3]
    xd, md, sd = dev(x[:B]), dev(mean), dev(scale)
    rows, w = ops.lime_neighbourhood(xd, md, sd, N, 9)
    rows[:, 4] = rows[:, 3]
    z = lo.standardise(rows.cpu().numpy(), mean, scale)
    logits = torch.from_numpy(np.random.default_rng(9).normal(0, 1, (N, C)) + 2.0 * z[:, 3:5]).float().to(DEV)
    got = run_fit(rows, w, logits, xd, md, sd, B, N, C, F, lo.LOGIT)
    assert all(np.isfinite(v).all() for v in got.values())
    assert np.abs(got["dense"][..., 3] - got["dense"][..., 4]).max() <= 1e-6 * np.abs(got["dense"][..., 3]).max()
    assert np.abs(got["dense"][..., 3]).min() > 0.1 and (got["score"] > 0.5).all() and (got["score"] <= 1).all()


def test_refusals_leave_the_outputs_untouched():
    F, N, B, C, K = 21, 64, 2, 3, 7
    mean, scale, x = lo.case_stats(F, 1)
    xd, md, sd = dev(x[:B]), dev(mean), dev(scale)
    out = torch.full((B * N, F), SENTINEL, device=DEV)
    wout = torch.full((B * N,), SENTINEL, device=DEV, dtype=torch.float64)
    big = torch.zeros(129, dtype=torch.float64, device=DEV)

    def raw_neighbourhood(x=xd, mean=md, F=F, row0=0, row1=B * N, stride=F):
        call("mmskin_lime_neighbourhood", ptr(x), stride, B, ptr(mean), ptr(sd), F, N, 0, 0, 0, row0, row1, ptr(out), max(F, 21), ptr(wout), 1,
             stream())

    for kw, word in [(dict(F=129, mean=big, stride=129), "at most 128"), (dict(mean=None), "null"), (dict(x=None), "null"),
                     (dict(row0=9, row1=3), "not a range"), (dict(row1=B * N + 1), "not a range")]:
        with pytest.raises(MMSkinError, match=word):
            raw_neighbourhood(**kw)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((wout == SENTINEL).all())

    rows, w = ops.lime_neighbourhood(xd, md, sd, N, 0)
    logits = torch.zeros((B * N, C), device=DEV)
    acc = torch.full((int(ops.lime_accumulator(B, N, F, C, DEV).numel()),), SENTINEL, dtype=torch.float64, device=DEV)

    def raw_reduce(rows=rows, F=F, row0=0, row1=B * N, C=C):
        call("mmskin_lime_reduce", ptr(rows), max(F, 21), ptr(w), 1, ptr(logits), 0, 0, ptr(md), ptr(sd), B, N, F, C, row0, row1, ptr(acc),
             stream())

    for kw, word in [(dict(F=129), "at most 128"), (dict(rows=None), "null"), (dict(row0=9, row1=3), "not a range"), (dict(C=65), "classes")]:
        with pytest.raises(MMSkinError, match=word):
            raw_reduce(**kw)
    torch.cuda.synchronize()
    assert bool((acc == SENTINEL).all())

    outs = [torch.full((B, C, K), SENTINEL, dtype=torch.float64, device=DEV), torch.full((B, C, K), -77, dtype=torch.int32, device=DEV)]
    outs += [torch.full((B, C), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(3)]
    outs += [torch.full((B, C, F), SENTINEL, dtype=torch.float64, device=DEV), torch.full((F, C), SENTINEL, dtype=torch.float64, device=DEV)]
    ws = torch.empty(int(ops._lib.load().mmskin_lime_solve_workspace_bytes(B, F, C)), dtype=torch.uint8, device=DEV)
    zero_acc = ops.lime_accumulator(B, N, F, C, DEV)

    def raw_solve(F=F, K=K, x=xd, intercept=outs[2]):
        call("mmskin_lime_solve", ptr(zero_acc), ptr(x), max(F, 21), ptr(md), ptr(sd), B, N, F, C, K, ptr(outs[0]), ptr(outs[1]), ptr(intercept),
             ptr(outs[3]), ptr(outs[4]), ptr(outs[5]), ptr(outs[6]), ptr(ws), stream())

    for kw, word in [(dict(F=129), "at most 128"), (dict(K=F + 1), "num_features"), (dict(K=0), "num_features"), (dict(x=None), "null"),
                     (dict(intercept=None), "null")]:
        with pytest.raises(MMSkinError, match=word):
            raw_solve(**kw)
    # sums that are not those of a neighbourhood (nothing was reduced: sum w = 0): an error, not NaNs
    with pytest.raises(MMSkinError, match="error 4.*pivot"):
        raw_solve()
    torch.cuda.synchronize()
    assert all(bool((t == -77).all()) for t in outs)


# --------------------------------------------------------------------------------------------------------- end to end
def hip_model(mech):
    os.environ["MMSKIN_BACKBONE_DTYPE"] = "fp32"
    cpu = det_init_(OracleMultimodalModel(**dict(SMALL, attention_mecanism=mech)), salt=so.E2E_SALT).eval()
    hip = M.MultimodalModel(**dict(SMALL, attention_mecanism=mech, device=DEV))
    hip.load_state_dict(cpu.state_dict(), strict=True)
    return hip.to(DEV).eval()


def e2e_rows():
    """the sweep fixture's 8 rows, encoded (18 columns) and padded to the model's vocab_size of 20: the two constant columns get
    scale 1"""
    enc = so.e2e_encoder()
    img, cats, num = so.e2e_case()
    encoded = enc.transform(enc.codes(cats).to(DEV), torch.from_numpy(num).float().to(DEV))
    rows = torch.zeros((8, 20), device=DEV)
    rows[:, :encoded.shape[1]] = encoded
    return enc, img, rows


@pytest.mark.parametrize("output", ["prob", "logit"])
@pytest.mark.parametrize("mech", ["gfcam", "concatenation"])
def test_lime_end_to_end(mech, output):
    """two batches of 2 images, N = 257, K = 7: MetadataLime against the restatement driven by the model's own head on the device's
    own rows; the fits are fp64 and only the soft-max is fp32, taken the same way: 1e-9, as for the kernels"""
    hip = hip_model(mech)
    enc, img, rows = e2e_rows()
    N, K, B, C, F, seed = 257, 7, 2, 6, 20, 11
    calls = []
    encode = hip.encode_image
    hip.encode_image = lambda image: (calls.append(tuple(image.shape)), encode(image))[1]
    make = lambda per: MetadataLime(hip, enc, DEV, rows, num_samples=N, num_features=K, seed=seed, output=output, rows_per_head_call=per)  # noqa: E731
    ex = make(10 ** 6)
    assert ex.scale[18] == 1.0 and ex.scale[19] == 1.0 and ex.mean[19] == 0.0
    md, sd = dev(ex.mean), dev(ex.scale)
    results = []
    for k, (r0, r1) in enumerate([(0, 2), (2, 4)]):
        before = len(calls)
        res = ex.explain(img[r0:r1].to(DEV), rows[r0:r1])
        assert calls[before:] == [(B, 3, 32, 32)] and res.n_samples == r1      # the image encoder ran once
        assert tuple(res.coef.shape) == (B, C, K) and tuple(res.dense.shape) == (B, C, F) and tuple(res.score.shape) == (B, C)
        results.append(res)
        # the oracle on the device's rows (sample offset = the samples explained before) and the head's logits on them
        with torch.no_grad():
            metas, _ = ops.lime_neighbourhood(rows[r0:r1].contiguous(), md, sd, N, seed, sample0=r0)
            feat = encode(img[r0:r1].to(DEV))
            logits = hip.fuse(feat.index_select(0, torch.arange(B * N, device=DEV) // N), metas).float()
        want = lo.explain_batch(metas.cpu().numpy().reshape(B, N, F), logits.cpu().numpy().reshape(B, N, C), ex.mean, ex.scale, K,
                                lo.PROB if output == "prob" else lo.LOGIT)
        assert want["gap"].min() > 1e-6
        assert np.array_equal(res.features.cpu().numpy(), want["feature"])
        for key, got in (("coef", res.coef), ("intercept", res.intercept), ("local_pred", res.local_pred), ("score", res.score), ("dense", res.dense)):
            err = float((np.abs(got.cpu().numpy() - want[key]) / np.maximum(1.0, np.abs(want[key]))).max())
            print(f"{mech} {output} batch {k}: {key} against the oracle {err:.3e}, max |want| {np.abs(want[key]).max():.3e}")
            assert err <= SOLVE_TOL, key
        assert np.abs(want["coef"]).max() > 1e-4                               # the head reacts to the metadata: there is something to get wrong
    # |coef| accumulates over the two batches; the ranking follows it
    total = np.zeros((F, C))
    for res in results:
        for b in range(B):
            total += np.abs(res.dense[b].cpu().numpy()).T
    assert np.array_equal(ex.abs_sum.cpu().numpy(), total) and np.allclose(results[-1].mean_abs.cpu().numpy(), total / 4, rtol=1e-15, atol=0)
    importance, order = ex.global_importance()
    assert np.array_equal(order.cpu().numpy(), np.argsort(-(total / 4).mean(-1), kind="stable"))
    names = [f"f{j}" for j in range(F)]
    listed = results[0].as_list(1, 3, names)
    assert [n for n, _ in listed] == [names[j] for j in results[0].features[1, 3].tolist()] and len(listed) == K
    # head calls cut at 100 rows: bitwise the same explanation
    cut = make(100)
    for k, (r0, r1) in enumerate([(0, 2), (2, 4)]):
        res = cut.explain(img[r0:r1].to(DEV), rows[r0:r1])
        for key in ("features", "coef", "intercept", "score", "local_pred", "dense"):
            assert torch.equal(getattr(res, key), getattr(results[k], key)), key
    ex.reset()
    assert ex.n_samples == 0 and ex.abs_sum is None


def test_explain_refuses_train_mode_and_a_fusion_without_metadata():
    enc, img, rows = e2e_rows()
    hip = hip_model("gfcam")
    ex = MetadataLime(hip, enc, DEV, rows, num_samples=64)
    hip.train()
    with pytest.raises(MMSkinError, match="eval"):
        ex.explain(img[:2].to(DEV), rows[:2])
    blind = M.MultimodalModel(**dict(SMALL, attention_mecanism="no-metadata", device=DEV)).to(DEV).eval()
    with pytest.raises(ValueError, match="nothing to explain"):
        MetadataLime(blind, enc, DEV, rows, num_samples=64).explain(img[:2].to(DEV), rows[:2])
