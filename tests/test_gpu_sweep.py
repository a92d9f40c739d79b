"""-m gpu: the metadata-sweep kernels (csrc/sweep.hip) against their numpy restatement (tests/sweep_oracle.py, held to sklearn
and to float64 formulas by tests/test_cpu_sweep.py), and mmskin.sweep.MetadataSweep end to end on the HIP model against plain
forwards of the same model and against the reference's loop on the CPU oracle."""
import os

import numpy as np
import pytest
import torch

import sweep_oracle as so
from gpu_util import DEV
from helpers import SMALL
from mmskin import ops
from mmskin._lib import MMSkinError
from mmskin.preprocess import MetadataEncoder
from mmskin.sweep import MetadataSweep
from models import multimodalIntraInterModal as M
from oracle.detinit import det_init_
from oracle.model import OracleMultimodalModel

pytestmark = pytest.mark.gpu

SENTINEL = -77.0

# Largest |fp32 numpy restatement - float64| of the continuous outputs over sweep_oracle.REDUCE_SHAPES (seed 0, the inputs of
# the kernel test), measured on the CPU: probs 3.0003e-07, entropy 7.2807e-07, KL 4.9967e-06, JS 1.6013e-07, confidence change
# 2.3803e-07 (tests/test_cpu_sweep.py::test_oracle_reduce_matches_float64 prints the figures per case and asserts that they
# stay at or below these).  The kernel sums in another order and uses another exp / log, so it is allowed
# REDUCE_KERNEL_FACTOR times these.
REDUCE_F32_ERROR = {"probs": 3.0003e-07, "entropy": 7.2807e-07, "kl": 4.9967e-06, "js": 1.6013e-07, "dconf": 2.3803e-07}
REDUCE_KERNEL_FACTOR = 4.0


# --------------------------------------------------------------------------------------------------------- variants
def encoder_case(n_cat, n_num, B, seed):
    """category counts cycle through 1 .. 7; codes include -1 (unseen at fit time); numerics include NaN"""
    rng = np.random.default_rng(seed)
    counts = [1 + (j % 7) for j in range(n_cat)]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    codes = np.stack([rng.integers(-1, c, B) for c in counts], axis=1).astype(np.int32) if n_cat else np.zeros((B, 0), dtype=np.int32)
    numeric = rng.uniform(-5, 90, (B, n_num)).astype(np.float32)
    numeric[rng.random((B, n_num)) < 0.25] = np.nan
    mean, scale = rng.uniform(-3, 50, n_num).astype(np.float32), rng.uniform(0.5, 20, n_num).astype(np.float32)
    missing = np.array([rng.integers(-1, c) for c in counts], dtype=np.int32)
    return counts, off, codes, numeric, mean, scale, missing


def variant_table(V, counts, n_num, rng):
    """the baseline, then every op in turn on columns and codes drawn at random (-1 included)"""
    n_cat = len(counts)
    recs = [so.record()]
    for v in range(1, V):
        cat = n_cat and (not n_num or v % 2)
        if cat:
            col = int(rng.integers(0, n_cat))
            a, b = (int(x) for x in rng.integers(-1, counts[col], 2))
            recs.append(so.record(so.CAT_TOGGLE if v % 4 == 1 else so.CAT_SET, col, a, b))
        else:
            recs.append(so.record(so.NUM_ADD if v % 4 == 0 else so.NUM_SET, n_cat + int(rng.integers(0, n_num)), value=float(rng.uniform(-9, 80))))
    return so.table(recs)


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("V", [1, 16])
@pytest.mark.parametrize("n_cat,n_num", [(0, 3), (1, 0), (21, 3)])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_variants_kernel_matches_the_restatement_bit_for_bit(B, n_cat, n_num, V, with_mask):
    rng = np.random.default_rng(B * 100 + n_cat * 10 + V + with_mask)
    counts, off, codes, numeric, mean, scale, missing = encoder_case(n_cat, n_num, B, seed=B + n_cat)
    width = int(off[-1]) + n_num
    tab = variant_table(V, counts, n_num, rng)
    mask = (rng.random((V, B, n_cat + n_num)) < 0.3).astype(np.uint8) if with_mask else None
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    for out_width in sorted({max(width - 2, 1), width, width + 5}):
        want = so.variants(codes, numeric, off, mean, scale, -1.0, tab, out_width, mask=mask, missing_code=missing)
        buf = torch.full((V + 2, B, out_width), SENTINEL, device=DEV)         # one guard block on either side of the output
        got = ops.metadata_variants(dev(codes), dev(numeric), off, dev(mean), dev(scale), -1.0, tab, out_width, mask=dev(mask),
                                    missing_code=dev(missing), out=buf[1:V + 1])
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all(), "bytes outside the V blocks were written"
        assert not (host[1:V + 1] == SENTINEL).any(), "an element was not written"
        assert got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), want), (out_width, width)
        if out_width > width:
            assert not host[1:V + 1, :, width:].any()


def test_unmutated_variant_equals_metadata_encode_bit_for_bit():
    rng = np.random.default_rng(0)
    n = 67
    cats = np.stack([rng.choice(["True", "False", "EMPTY"], n), rng.choice(["ARM", "FACE", "BACK", "CHEST", "EMPTY"], n),
                     rng.choice(["FEMALE", "MALE"], n)], axis=1)
    num = np.stack([rng.integers(6, 95, n).astype(float), rng.uniform(1, 40, n), rng.uniform(1, 30, n)], axis=1)
    num[rng.random((n, 3)) < 0.15] = np.nan
    enc = MetadataEncoder().fit(cats[:50], num[:50])
    codes, numeric = enc.codes(cats).to(DEV), torch.from_numpy(num).float().to(DEV)
    want = enc.transform(codes, numeric)
    off, mean, scale = enc._tables(DEV)
    tab = so.table([so.record(), so.record(so.NUM_ADD, 3, value=5.0), so.record()])
    got = ops.metadata_variants(codes, numeric, off.cpu().numpy(), mean, scale, enc.nan_fill, tab, enc.width)
    assert torch.equal(got[0], want) and torch.equal(got[2], want) and not torch.equal(got[1], want)


def test_variants_bad_table_returns_a_status_without_launching():
    counts, off, codes, numeric, mean, scale, missing = encoder_case(2, 1, 4, seed=1)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    out = torch.full((1, 4, 4), SENTINEL, device=DEV)
    for rec, word in [(so.record(so.CAT_SET, 3, 0), "outside the 3 columns"), (so.record(so.CAT_SET, 2, 0), "categorical op on numeric"),
                      (so.record(so.NUM_SET, 0, value=1.0), "numeric op on categorical"), (so.record(so.CAT_SET, 1, 2), "outside the 2 categories")]:
        with pytest.raises(MMSkinError, match=word):
            ops.metadata_variants(dev(codes), dev(numeric), off, dev(mean), dev(scale), -1.0, so.table([rec]), 4, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# --------------------------------------------------------------------------------------------------------- reduce
def run_reduce(logits, base, labels, counters=None):
    V, B, C = logits.shape
    if counters is None:
        counters = (torch.zeros(V, dtype=torch.int32, device=DEV), torch.zeros((V, C, C), dtype=torch.int32, device=DEV),
                    torch.zeros((V, C, C), dtype=torch.int32, device=DEV) if labels is not None else None)
    probs, pred, margin, stats = ops.sweep_reduce(torch.from_numpy(logits).to(DEV), torch.from_numpy(base).to(DEV), counters[0], counters[1],
                                                  confusion=counters[2], labels=None if labels is None else torch.from_numpy(labels).to(DEV))
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return dict(probs=host(probs), pred=host(pred), margin=host(margin), stats=host(stats), flips=host(counters[0]),
                transitions=host(counters[1]), confusion=host(counters[2])), counters


@pytest.mark.parametrize("V,B,C", so.REDUCE_SHAPES)
def test_reduce_kernel_matches_the_restatement(V, B, C):
    """planted in every case (sweep_oracle.reduce_case): exact ties between the two largest logits, variant 0 and one more row
    equal to their baseline, a label out of range"""
    logits, base, labels = so.reduce_case(V, B, C)
    want = so.reduce(logits, base, labels)
    want64 = so.reduce(logits, base, labels, dt=np.float64)
    got, counters = run_reduce(logits, base, labels)
    for key in ("pred", "flips", "transitions", "confusion"):
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["margin"], want["margin"])
    assert not got["stats"][0, :, 1:].any() and got["flips"][0] == 0                   # variant 0 is the baseline: zero KL, JS, change
    if V > 1:
        assert got["margin"][1, 0] == 0 and got["pred"][1, 0] == want["pred"][1, 0]     # the tie: the first index wins
        assert not got["stats"][-1, B - 1, 1:].any()
    err = so.continuous_errors(got, want64)
    print(f"V {V} B {B} C {C}: kernel against float64: {err}")
    for name, e in err.items():
        assert e <= REDUCE_KERNEL_FACTOR * REDUCE_F32_ERROR[name], (name, e)
    # a second call into the same counters: the sum; and without labels the confusion matrix is not touched
    logits2, base2, labels2 = so.reduce_case(V, B, C, seed=1)
    want2 = so.reduce(logits2, base2, labels2)
    got2, _ = run_reduce(logits2, base2, labels2, counters)
    for key in ("flips", "transitions", "confusion"):
        assert np.array_equal(got2[key], want[key] + want2[key]), key
    got3, _ = run_reduce(logits, base, None)
    assert got3["confusion"] is None and np.array_equal(got3["transitions"], want["transitions"]) and np.array_equal(got3["pred"], want["pred"])


def test_reduce_bf16_logits_and_unsupported_class_counts():
    logits, base, _ = so.reduce_case(3, 65, 7)
    lb = torch.from_numpy(logits).to(DEV).bfloat16()
    flips, trans = torch.zeros(3, dtype=torch.int32, device=DEV), torch.zeros((3, 7, 7), dtype=torch.int32, device=DEV)
    probs, pred, margin, stats = ops.sweep_reduce(lb, torch.from_numpy(base).to(DEV), flips, trans)
    want = so.reduce(lb.float().cpu().numpy(), base)
    assert np.array_equal(pred.cpu().numpy(), want["pred"]) and np.array_equal(trans.cpu().numpy(), want["transitions"])
    assert np.array_equal(margin.cpu().numpy(), want["margin"])
    for C in (65, 1):
        sentinel = torch.full((2, 4), -7, dtype=torch.int32, device=DEV)
        with pytest.raises(MMSkinError, match="error 3"):                   # MMSKIN_ERR_UNSUPPORTED, nothing launched
            ops.sweep_reduce(torch.zeros((2, 4, C), device=DEV), torch.zeros((4, C), device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV),
                             torch.zeros((2, C, C), dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        assert bool((sentinel == -7).all())


# --------------------------------------------------------------------------------------------------------- end to end
def model_pair(mech):
    os.environ["MMSKIN_BACKBONE_DTYPE"] = "fp32"
    kw = dict(SMALL, attention_mecanism=mech)
    cpu = det_init_(OracleMultimodalModel(**kw), salt=so.E2E_SALT).eval()
    hip = M.MultimodalModel(**dict(kw, device=DEV))
    hip.load_state_dict(cpu.state_dict(), strict=True)
    return cpu, hip.to(DEV).eval()


@pytest.mark.parametrize("mech", so.E2E_MECHS)
def test_sweep_end_to_end(mech):
    """A flip sweep of 16 mutations and a missing sweep of 3 rates, each as a batch of 5 and a batch of 3 into the same counters.
    (a) logits / probs against one plain forward of the same HIP model per variant, within the project's fp32 logits tolerance
    (the V x B-row head call may take another GEMM route than a B-row one); (b) pred, flips, transitions against the reference's
    loop on the CPU oracle, pairs whose oracle top-2 margin is below twice that tolerance excluded (at most 10 %,
    tests/test_cpu_sweep.py guarantees it for these inputs; a row whose baseline is excluded leaves the transitions for all
    v); (c) the image encoder runs once per run."""
    cpu, hip = model_pair(mech)
    enc = so.e2e_encoder()
    img, cats, num = so.e2e_case()
    codes, numeric = enc.codes(cats), torch.from_numpy(num).float()
    labels = torch.arange(8) % 6
    off = np.concatenate([[0], np.cumsum([len(c) for c in enc.categories_])])
    calls = []
    encode = hip.encode_image
    hip.encode_image = lambda image: (calls.append(tuple(image.shape)), encode(image))[1]
    sw = MetadataSweep(hip, enc, DEV, rows_per_head_call=32)               # 85 and 51 rows: three and two ragged head calls
    flip_tab = sw.flip_variants(so.E2E_FLIPS, so.E2E_CAT_NAMES, so.E2E_NUM_NAMES)
    miss_tab, miss_mask = sw.missing_variants(so.E2E_RATES, 8, so.E2E_NUM_NAMES, so.E2E_CAT_NAMES, so.E2E_SEEDS)
    for name, tab, mask in [("flip", flip_tab, None), ("missing", miss_tab, miss_mask)]:
        V = len(tab)
        metas = so.variants(codes.numpy(), num, off, enc.mean_, enc.scale_, enc.nan_fill, tab, 20, mask=mask, missing_code=sw._missing_codes())
        oracle = so.oracle_loop(cpu, img, metas)
        want = so.reduce(oracle, oracle[0])
        clear = want["margin"] >= so.margin_threshold(oracle)                                   # [V, 8]
        assert (~clear).mean() <= 0.10
        sw.reset()
        pred = []
        for r0, r1 in so.E2E_BATCHES:
            before = len(calls)
            res = sw.run(img[r0:r1].to(DEV), codes[r0:r1], numeric[r0:r1], tab, mask=None if mask is None else mask[:, r0:r1],
                         labels=labels[r0:r1])
            assert calls[before:] == [(r1 - r0, 3, 32, 32)]                                                                   # (c)
            with torch.no_grad():
                plain = torch.stack([hip(img[r0:r1].to(DEV), torch.from_numpy(metas[v, r0:r1]).to(DEV)) for v in range(V)]).float()
            err = (res.logits.float() - plain).abs()
            print(f"{mech} {name} rows {r0}:{r1}: max |sweep - plain forward| {float(err.max()):.3e}, max |logit| {float(plain.abs().max()):.3e}")
            assert bool((err <= so.LOGIT_ATOL + so.LOGIT_RTOL * plain.abs()).all())                                          # (a)
            assert torch.allclose(res.probs, torch.softmax(plain, dim=-1), rtol=0, atol=0.5 * float((so.LOGIT_ATOL + so.LOGIT_RTOL * plain.abs()).max()) + 1e-6)
            assert tuple(res.pred.shape) == (V, r1 - r0) and tuple(res.stats.shape) == (V, r1 - r0, 4)
            pred.append(res.pred.cpu().numpy())
        pred = np.concatenate(pred, axis=1)
        assert np.array_equal(pred[clear], want["pred"][clear])                                                               # (b)
        assert res.n_samples == 8 and int(res.transitions.sum()) == V * 8 and int(res.confusion.sum()) == V * 8
        rows = clear[0]                                                     # rows whose baseline prediction is beyond doubt
        flips, trans = res.flips.cpu().numpy(), res.transitions.cpu().numpy()
        for v in range(V):
            keep = rows & clear[v]
            if keep.all():                                                  # nothing excluded: the accumulated counters, exactly
                assert flips[v] == want["flips"][v] and np.array_equal(trans[v], want["transitions"][v]), v
            t = np.zeros((6, 6), dtype=np.int32)                            # the counters rebuilt from the kernel's own predictions ...
            np.add.at(t, (pred[0], pred[v]), 1)
            assert np.array_equal(trans[v], t) and flips[v] == (pred[v] != pred[0]).sum()
            w = np.zeros((6, 6), dtype=np.int32)                            # ... and, on the rows that are kept, the oracle's
            np.add.at(w, (want["pred"][0][keep], want["pred"][v][keep]), 1)
            k = np.zeros((6, 6), dtype=np.int32)
            np.add.at(k, (pred[0][keep], pred[v][keep]), 1)
            assert np.array_equal(k, w), v
        conf = np.zeros((6, 6), dtype=np.int32)
        np.add.at(conf, (labels.numpy(), pred[1]), 1)
        assert np.array_equal(res.confusion[1].cpu().numpy(), conf)
        assert torch.allclose(res.flip_rate, res.flips.double() / 8)
