"""-m gpu: the metadata-Shapley kernels (csrc/shapley.hip) against their numpy restatement (tests/shapley_oracle.py, held to
brute-force Shapley values and to float64 by tests/test_cpu_shapley.py), and mmskin.shapley.MetadataShapley end to end on the HIP
model against the straightforward loop on the CPU oracle model."""
import functools
import os

import numpy as np
import pytest
import torch

import shapley_oracle as sh
import sweep_oracle as so
from gpu_util import DEV
from helpers import SMALL
from mmskin import ops
from mmskin._lib import MMSkinError
from mmskin.preprocess import MetadataEncoder
from mmskin.shapley import MetadataShapley
from models import multimodalIntraInterModal as M
from oracle.detinit import det_init_
from oracle.model import OracleMultimodalModel

pytestmark = pytest.mark.gpu

SENTINEL = -77.0

# Largest |fp32 numpy restatement - float64| over shapley_oracle.REDUCE_CASES (seed 0, the inputs of the kernel test), measured on
# the CPU (tests/test_cpu_shapley.py::test_oracle_reduce_matches_float64 prints the figures per case and asserts that they stay
# at or below these): of phi, and of the two ends base = v(empty) and full = v(all).  "prob": the fp32 soft-max, phi 1.5683e-07,
# ends 1.4382e-07; "logit": only the rounding of the fp64 result to the fp32 output, at logits of up to 52 and |phi| of up to 32,
# phi 1.2666e-06, ends 4.7684e-07.  The kernel uses another exp and adds the background rows in another order, so it is allowed
# REDUCE_KERNEL_FACTOR times these -- the factor of tests/test_gpu_sweep.py, for the same reason.
REDUCE_F32_ERROR = {"prob": {"phi": 1.5683e-07, "ends": 1.4382e-07}, "logit": {"phi": 1.2666e-06, "ends": 4.7684e-07}}
REDUCE_KERNEL_FACTOR = 4.0


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# --------------------------------------------------------------------------------------------------------- coalitions
def coalition_case(n_cat, n_num, B, G, seed):
    """category counts cycle through 1 .. 7; codes include -1 (unseen at fit time) and numerics NaN, on the explained rows and on
    the background alike: B + G rows of one draw, the first B explained, the rest the background"""
    rng = np.random.default_rng(seed)
    counts = [1 + (j % 7) for j in range(n_cat)]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    n = B + G
    codes = np.stack([rng.integers(-1, c, n) for c in counts], axis=1).astype(np.int32) if n_cat else np.zeros((n, 0), dtype=np.int32)
    numeric = rng.uniform(-5, 90, (n, n_num)).astype(np.float32)
    numeric[rng.random((n, n_num)) < 0.25] = np.nan
    if n_cat:
        codes[0, 0] = codes[B, n_cat - 1] = -1
    if n_num:
        numeric[0, 0] = numeric[B, n_num - 1] = np.nan
    mean, scale = rng.uniform(-3, 50, n_num).astype(np.float32), rng.uniform(0.5, 20, n_num).astype(np.float32)
    return off, codes[:B], numeric[:B], codes[B:], numeric[B:], mean, scale


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("G", [1, 3, 33])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n_cat,n_num", [(0, 3), (1, 0), (5, 3)])        # (1, 0): M = 1, no interior coalition, only the ends
def test_coalitions_kernel_matches_the_restatement_bit_for_bit(n_cat, n_num, B, G, P):
    n = n_cat + n_num
    off, codes, numeric, bg_codes, bg_numeric, mean, scale = coalition_case(n_cat, n_num, B, G, seed=100 * B + 10 * G + n)
    rng = np.random.default_rng(B + G + P)
    perms = np.stack([rng.permutation(n) for _ in range(P)]).astype(np.int32)
    width = int(off[-1]) + n_num
    N = sh.n_rows(B, G, P, n)
    assert ops.shapley_rows(B, G, P, n) == N
    args = (dev(codes), dev(numeric), dev(bg_codes), dev(bg_numeric), off, dev(mean), dev(scale), -1.0, perms)
    for out_width in sorted({max(width - 2, 1), width, width + 5}):
        want = sh.coalition_rows(codes, numeric, bg_codes, bg_numeric, off, mean, scale, -1.0, perms, out_width)
        assert want.shape == (N, out_width)
        buf = torch.full((N + 2, out_width), SENTINEL, device=DEV)            # one guard row on either side of the output
        got = ops.shapley_coalitions(*args, out_width, out=buf[1:N + 1])
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all(), "bytes outside the rows were written"
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want), (out_width, width)
        if out_width > width:
            assert not host[1:N + 1, width:].any()
        # two ragged ranges: each writes its rows and nothing else, and together they are the whole walk
        cut = N // 3 + 1
        if cut < N:
            buf = torch.full((N + 2, out_width), SENTINEL, device=DEV)
            ops.shapley_coalitions(*args, out_width, row0=cut, row1=N, out=buf[1 + cut:N + 1])
            torch.cuda.synchronize()
            assert bool((buf[:1 + cut] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())
            ops.shapley_coalitions(*args, out_width, row0=0, row1=cut, out=buf[1:1 + cut])
            torch.cuda.synchronize()
            assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())
            assert np.array_equal(buf[1:N + 1].cpu().numpy(), want)


def test_end_rows_equal_metadata_encode_bit_for_bit():
    """the all-explained row of a sample is metadata_encode of x, every row of its empty coalition that of b_g"""
    rng = np.random.default_rng(0)
    n, B, G, P = 70, 5, 4, 2
    cats = np.stack([rng.choice(["True", "False", "EMPTY"], n), rng.choice(["ARM", "FACE", "BACK", "CHEST", "EMPTY"], n),
                     rng.choice(["FEMALE", "MALE"], n)], axis=1)
    num = np.stack([rng.integers(6, 95, n).astype(float), rng.uniform(1, 40, n), rng.uniform(1, 30, n)], axis=1)
    num[rng.random((n, 3)) < 0.15] = np.nan
    enc = MetadataEncoder().fit(cats[:50], num[:50])
    cats[60, 1] = "SCALP"                                                       # unseen at fit time, on the explained side
    cats[66, 1] = "SCALP"                                                       # ... and in the background
    codes, numeric = enc.codes(cats).to(DEV), torch.from_numpy(num).float().to(DEV)
    x, bg = slice(60, 60 + B), slice(66, 66 + G)
    want_x, want_bg = enc.transform(codes[x], numeric[x]), enc.transform(codes[bg], numeric[bg])
    off, mean, scale = enc._tables(DEV)
    perms = MetadataShapley.draw_permutations(6, P, seed=1)
    got = ops.shapley_coalitions(codes[x].contiguous(), numeric[x].contiguous(), codes[bg].contiguous(), numeric[bg].contiguous(),
                                 off.cpu().numpy(), mean, scale, enc.nan_fill, perms, enc.width)
    K = 2 * P * 5
    assert torch.equal(got[B * (K + 1) * G:], want_x)
    walk = got[:B * (K + 1) * G].reshape(B, K + 1, G, enc.width)
    assert all(torch.equal(walk[b, K], want_bg) for b in range(B))
    assert not torch.equal(walk[0, 0], want_bg) and not torch.equal(walk[0, 0], want_x[:1].expand(G, -1))


# --------------------------------------------------------------------------------------------------------- reduce
def run_reduce(logits, perms, B, G, output, cuts=(), abs_sum=None):
    """the walk's logits through ops.shapley_reduce, in the row ranges that `cuts` splits [0, N) into"""
    P, n = perms.shape
    C = logits.shape[1]
    v = torch.full((B, 2 * P * (n - 1) + 2, C), float("nan"), dtype=torch.float64, device=DEV)
    edges = [0, *cuts, logits.shape[0]]
    out = None
    for r0, r1 in zip(edges[:-1], edges[1:]):
        out = ops.shapley_reduce(logits[r0:r1].contiguous(), v, perms, G, r0, output=output, finish=r1 == logits.shape[0], abs_sum=abs_sum)
    torch.cuda.synchronize()
    phi, base, full = out
    assert not bool(torch.isnan(v).any()), "an entry of v was not written"
    return dict(phi=phi.cpu().numpy(), base=base.cpu().numpy(), full=full.cpu().numpy(), v=v.cpu().numpy())


@pytest.mark.parametrize("B,G,P,n,C", sh.REDUCE_CASES)
def test_reduce_kernels_match_the_restatement(B, G, P, n, C):
    logits, perms = sh.reduce_case(B, G, P, n, C)
    N = logits.shape[0]
    K = 2 * P * (n - 1)
    for output, mode in (("prob", sh.PROB), ("logit", sh.LOGIT)):
        for dtype in (torch.float32, torch.bfloat16):
            lg = torch.from_numpy(logits).to(DEV).to(dtype)
            want64 = sh.reduce(lg.float().cpu().numpy(), B, G, perms, mode, dt=np.float64)       # bf16: the rounded values
            acc = torch.zeros((n, C), dtype=torch.float64, device=DEV)
            got = run_reduce(lg, perms, B, G, mode, abs_sum=acc)
            err = sh.reduce_errors(got, want64)
            print(f"B {B} G {G} P {P} M {n} C {C} {output} {dtype}: kernel against float64: {err}")
            bound = REDUCE_KERNEL_FACTOR * REDUCE_F32_ERROR[output]["phi"]
            assert got["phi"].dtype == np.float32 and got["phi"].shape == (B, n, C)
            assert err["phi"] <= bound and err["ends"] <= REDUCE_KERNEL_FACTOR * REDUCE_F32_ERROR[output]["ends"]
            assert err["efficiency"] <= bound * n
            assert np.abs(got["v"] - want64["v"]).max() <= REDUCE_KERNEL_FACTOR * REDUCE_F32_ERROR[output]["ends"]
            # |phi| summed over the batch in fp64, b = 0 .. B - 1
            want_acc = np.zeros((n, C))
            for b in range(B):
                want_acc += np.abs(got["phi"][b].astype(np.float64))
            assert np.array_equal(acc.cpu().numpy(), want_acc)
            # the same inputs again, whole and in ragged ranges cut at whole coalitions: bitwise equal; the sums add up
            cuts = sorted({G * max(1, (B * (K + 1)) // 3), B * (K + 1) * G})
            cuts = [c for c in cuts if 0 < c < N]
            again = run_reduce(lg, perms, B, G, mode, cuts=cuts, abs_sum=acc)
            for key in ("phi", "base", "full", "v"):
                assert np.array_equal(got[key], again[key]), key
            for b in range(B):
                want_acc += np.abs(got["phi"][b].astype(np.float64))
            assert np.array_equal(acc.cpu().numpy(), want_acc)


def test_bad_arguments_return_a_status_and_launch_nothing():
    off, codes, numeric, bg_codes, bg_numeric, mean, scale = coalition_case(2, 1, 4, 3, seed=1)
    out = torch.full((sh.n_rows(4, 3, 2, 3), 6), SENTINEL, device=DEV)
    args = (dev(codes), dev(numeric), dev(bg_codes), dev(bg_numeric), off, dev(mean), dev(scale), -1.0)
    for perms, word in [([[0, 1, 2], [0, 2, 2]], "row 1 of the table is not a permutation"), ([[0, 1, 3], [0, 1, 2]], "not a permutation")]:
        with pytest.raises(MMSkinError, match=word):
            ops.shapley_coalitions(*args, np.array(perms, dtype=np.int32), 6, out=out)
    with pytest.raises(MMSkinError, match="extent"):
        ops.shapley_coalitions(dev(codes), dev(numeric), dev(bg_codes[:0]), dev(bg_numeric[:0]), off, dev(mean), dev(scale), -1.0,
                               np.array([[0, 1, 2]], dtype=np.int32), 6, row1=4, out=out[:4])
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    good = np.array([[2, 0, 1]], dtype=np.int32)
    for C in (1, 65):
        v = torch.full((2, 6, C), SENTINEL, dtype=torch.float64, device=DEV)
        with pytest.raises(MMSkinError, match="error 3"):                   # MMSKIN_ERR_UNSUPPORTED, nothing launched
            ops.shapley_reduce(torch.zeros((sh.n_rows(2, 3, 1, 3), C), device=DEV), v, good, 3, 0, finish=True)
        torch.cuda.synchronize()
        assert bool((v == SENTINEL).all())
    v = torch.full((2, 6, 6), SENTINEL, dtype=torch.float64, device=DEV)
    for perms, rows, row0, word in [(np.array([[2, 0, 0]], dtype=np.int32), sh.n_rows(2, 3, 1, 3), 0, "not a permutation"),
                                    (good, 4, 0, "split a coalition"), (good, 6, 2, "split a coalition")]:
        with pytest.raises(MMSkinError, match=word):
            ops.shapley_reduce(torch.zeros((rows, 6), device=DEV), v, perms, 3, row0, finish=True)
    torch.cuda.synchronize()
    assert bool((v == SENTINEL).all())


# --------------------------------------------------------------------------------------------------------- end to end
def oracle_model(mech):
    return det_init_(OracleMultimodalModel(**dict(SMALL, attention_mecanism=mech)), salt=so.E2E_SALT).eval()


def hip_model(mech):
    os.environ["MMSKIN_BACKBONE_DTYPE"] = "fp32"
    hip = M.MultimodalModel(**dict(SMALL, attention_mecanism=mech, device=DEV))
    hip.load_state_dict(oracle_model(mech).state_dict(), strict=True)
    return hip.to(DEV).eval()


def e2e_inputs():
    enc = so.e2e_encoder()
    img, cats, num = so.e2e_case()
    codes, numeric = enc.codes(cats), torch.from_numpy(num).float()
    rows = sh.E2E_BACKGROUND_ROWS
    return enc, img, codes, numeric, codes[rows].contiguous(), numeric[rows].contiguous()


@functools.lru_cache(maxsize=None)
def e2e_oracle_logits(mech):
    """the CPU oracle's logits of every (sample, coalition) of the 8 rows: computed once per fusion, shared by both outputs"""
    cpu = oracle_model(mech)
    enc, img, codes, numeric, bg_codes, bg_numeric = e2e_inputs()
    off = np.concatenate([[0], np.cumsum([len(c) for c in enc.categories_])])
    return sh.oracle_loop(cpu, img, codes.numpy(), numeric.numpy(), bg_codes.numpy(), bg_numeric.numpy(), off, enc.mean_, enc.scale_,
                          enc.nan_fill, sh.e2e_permutations(8), 20)


@pytest.mark.parametrize("output", ["prob", "logit"])
@pytest.mark.parametrize("mech", so.E2E_MECHS)
def test_shapley_end_to_end(mech, output):
    """8 images as a batch of 5 and one of 3, G = 3 background rows of the fixture, P = 2, several ragged head calls.  values, base
    and full against the loop on the CPU oracle model: every phi is a mean of differences of two means of `out`, and each
    probability (logit) is held to the sweep test's bound, 0.5 x (x 1) the project's fp32 logits tolerance at the largest logit."""
    hip = hip_model(mech)
    enc, img, codes, numeric, bg_codes, bg_numeric = e2e_inputs()
    want = sh.oracle_values(e2e_oracle_logits(mech), sh.e2e_permutations(8), sh.PROB if output == "prob" else sh.LOGIT)
    tol = so.LOGIT_ATOL + so.LOGIT_RTOL * want["logit_max"]
    bound = 2 * 0.5 * tol + 1e-6 if output == "prob" else 2 * tol
    calls = []
    encode = hip.encode_image
    hip.encode_image = lambda image: (calls.append(tuple(image.shape)), encode(image))[1]
    ex = MetadataShapley(hip, enc, DEV, bg_codes, bg_numeric, n_permutations=sh.E2E_P, seed=sh.E2E_SEED, output=output,
                         rows_per_head_call=100)                           # 99 rows a call: 440 and 264 rows, five and three calls
    assert np.array_equal(ex.permutations, sh.e2e_permutations(8)) and ex.rows_per_head_call == 99 and ex.rows_per_sample() == 88
    results = []
    for r0, r1 in so.E2E_BATCHES:
        before = len(calls)
        res = ex.explain(img[r0:r1].to(DEV), codes[r0:r1], numeric[r0:r1])
        assert calls[before:] == [(r1 - r0, 3, 32, 32)]                    # the image encoder ran once
        assert tuple(res.values.shape) == (r1 - r0, 8, 6) and tuple(res.base.shape) == tuple(res.full.shape) == (r1 - r0, 6)
        assert res.n_samples == r1
        results.append((res.values.clone(), res.base.clone(), res.full.clone()))
    values, base, full = (torch.cat(t).double().cpu().numpy() for t in zip(*results))
    err = {k: float(np.abs(g - want[k]).max()) for k, g in (("phi", values), ("base", base), ("full", full))}
    print(f"{mech} {output}: max |GPU - oracle loop| {err}, bound {bound:.3e}, max |phi| {np.abs(want['phi']).max():.3e}, "
          f"max |logit| {want['logit_max']:.3e}")
    assert np.abs(want["phi"]).max() > 5 * bound                           # the heads react to the metadata: there is something to get wrong
    assert err["phi"] <= bound and err["base"] <= bound and err["full"] <= bound
    assert np.abs(values.sum(axis=1) - (full - base)).max() <= REDUCE_KERNEL_FACTOR * REDUCE_F32_ERROR[output]["phi"] * 8     # efficiency
    mean_abs = res.mean_abs.cpu().numpy()
    assert np.allclose(mean_abs, np.abs(values).mean(axis=0), rtol=1e-12, atol=0)
    importance, order = ex.global_importance()
    assert np.allclose(importance.cpu().numpy(), mean_abs.mean(-1), rtol=1e-12, atol=0)
    assert np.array_equal(order.cpu().numpy(), np.argsort(-mean_abs.mean(-1), kind="stable"))
    # the same seed again: bitwise equal
    again = MetadataShapley(hip, enc, DEV, bg_codes, bg_numeric, n_permutations=sh.E2E_P, seed=sh.E2E_SEED, output=output, rows_per_head_call=100)
    r0, r1 = so.E2E_BATCHES[1]
    res2 = again.explain(img[r0:r1].to(DEV), codes[r0:r1], numeric[r0:r1])
    for a, b in zip((res2.values, res2.base, res2.full), results[1]):
        assert torch.equal(a, b)


def test_explain_refuses_train_mode_and_a_fusion_without_metadata():
    enc, img, codes, numeric, bg_codes, bg_numeric = e2e_inputs()
    hip = hip_model("gfcam")
    ex = MetadataShapley(hip, enc, DEV, bg_codes, bg_numeric, n_permutations=1)
    hip.train()
    with pytest.raises(MMSkinError, match="eval"):
        ex.explain(img[:2].to(DEV), codes[:2], numeric[:2])
    blind = M.MultimodalModel(**dict(SMALL, attention_mecanism="no-metadata", device=DEV)).to(DEV).eval()
    with pytest.raises(ValueError, match="nothing to explain"):
        MetadataShapley(blind, enc, DEV, bg_codes, bg_numeric, n_permutations=1).explain(img[:2].to(DEV), codes[:2], numeric[:2])
