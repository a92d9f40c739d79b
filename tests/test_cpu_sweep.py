"""The metadata sweep without a GPU: tests/sweep_oracle.py (the numpy restatement the kernels are held to by
tests/test_gpu_sweep.py) against sklearn / pandas on mutated raw rows and against float64 formulas; the host logic of
mmskin.sweep (record packing, the library's table validation, the missing-metadata draw, the errors of `run` that fire before any
GPU call); and the condition under which the end-to-end GPU test is meaningful."""
import ctypes

import numpy as np
import pytest
import torch

import sweep_oracle as so
from helpers import SMALL
from mmskin import _lib, ops
from mmskin._lib import MMSkinError
from mmskin.preprocess import MetadataEncoder
from mmskin.sweep import MetadataSweep
from models import multimodalIntraInterModal as M
from oracle.detinit import det_init_
from oracle.model import OracleMultimodalModel

# Largest |fp32 restatement - float64 formulas| over sweep_oracle.REDUCE_SHAPES, measured on the CPU (this test prints the
# figures); tests/test_gpu_sweep.py allows the kernel four times these
from test_gpu_sweep import REDUCE_F32_ERROR  # noqa: E402


# ------------------------------------------------------------------------------------------- variants against sklearn
CAT_NAMES = ["itch", "gender", "region", "bleed"]
NUM_NAMES = ["age", "diameter_1", "diameter_2"]


def raw_rows(n, rng):
    cats = np.stack([rng.choice(["True", "False", "EMPTY"], n), rng.choice(["FEMALE", "MALE", "EMPTY"], n),
                     rng.choice(["ARM", "FACE", "BACK", "FOREARM", "EMPTY"], n), rng.choice(["True", "False"], n)], axis=1).astype(object)
    num = np.stack([rng.integers(6, 95, n).astype(float), rng.uniform(1, 40, n), rng.uniform(1, 30, n)], axis=1)
    num[rng.random((n, 3)) < 0.2] = np.nan
    return cats, num


def mutate_like_the_reference(cats, num, name, rule):
    """flip_rate.py:164-183 on raw rows: a toggle is `a if x != a else b` written the reference's way round"""
    import pandas as pd
    df = pd.DataFrame(cats, columns=CAT_NAMES)
    for j, n in enumerate(NUM_NAMES):
        df[n] = num[:, j]
    if rule[0] == "toggle":
        df[name] = [rule[2] if x == rule[1] else rule[1] for x in df[name]]
    elif rule[0] == "set":
        df[name] = rule[1]
    elif rule[0] == "add":
        df[name] = [float(x) + rule[1] for x in df[name]]              # float('nan') + 5 stays NaN
    return df


def encode_like_the_reference(df, ohe, scaler, target):
    """inference_all_folds.py:95-112"""
    import pandas as pd
    catd = ohe.transform(df[CAT_NAMES].astype(str).to_numpy())
    numd = scaler.transform(df[NUM_NAMES].apply(pd.to_numeric, errors="coerce").fillna(-1).to_numpy())
    processed = np.hstack([catd, numd])
    if processed.shape[1] < target:
        processed = np.hstack([processed, np.zeros((processed.shape[0], target - processed.shape[1]))])
    return processed[:, :target]


@pytest.fixture(scope="module")
def fitted():
    from sklearn.preprocessing import OneHotEncoder, StandardScaler
    rng = np.random.default_rng(3)
    cats, num = raw_rows(120, rng)
    fit_rows = cats[:80].copy()                                    # "bleed" never shows "EMPTY" at fit time
    ohe = OneHotEncoder(sparse_output=False, handle_unknown="ignore").fit(fit_rows)
    scaler = StandardScaler().fit(np.where(np.isnan(num[:80]), -1.0, num[:80]))
    return cats, num, ohe, scaler, MetadataEncoder.from_sklearn(ohe, scaler)


RULES = [("itch", ("toggle", "True", "False")),                   # the boolean `not`: rows holding "EMPTY" (neither a nor b) go to a
         ("gender", ("toggle", "FEMALE", "MALE")),                 # the reference's gender swap
         ("region", ("toggle", "FACE", "FOREARM")),                # "FACE" if x != "FACE" else "FOREARM"
         ("region", ("set", "SCALP")),                             # a value unseen at fit time: an all-zero block
         ("age", ("set", 80.0)), ("diameter_1", ("add", 5.0)),     # NaN + 5 stays NaN, then fillna(-1)
         ("diameter_2", ("add", -2.5))]


@pytest.mark.parametrize("out_width", [16, 10, 21])             # the encoder's width (13 + 3), truncation, padding
def test_oracle_variants_match_sklearn_on_mutated_rows(fitted, out_width):
    cats, num, ohe, scaler, enc = fitted
    assert enc.width == 16 and np.isnan(num[:, 1]).any() and (cats[:, 0] == "EMPTY").any()
    sw = MetadataSweep(None, enc, "cpu", out_width=out_width)
    tab = sw.flip_variants(RULES, CAT_NAMES, NUM_NAMES)
    assert len(tab) == 1 + len(RULES) and tab["op"][0] == ops.META_NONE and tab["a"][4] == -1      # "SCALP" is unseen
    off = np.concatenate([[0], np.cumsum([len(c) for c in enc.categories_])])
    got = so.variants(enc.codes(cats).numpy(), num, off, enc.mean_, enc.scale_, enc.nan_fill, tab, out_width)
    for v, (name, rule) in enumerate([(None, ("none",))] + RULES):
        want = encode_like_the_reference(mutate_like_the_reference(cats, num, name, rule), ohe, scaler, out_width)
        oh = min(enc.onehot_width, out_width)
        assert np.array_equal(got[v][:, :oh], want[:, :oh]), (v, name)                            # one-hot block: exact
        assert np.allclose(got[v][:, oh:], want[:, oh:], rtol=1e-5, atol=1e-5), (v, name)         # as the metadata-encode test
    assert not got[:, :, 16:].any()


def test_oracle_variants_match_sklearn_on_blanked_rows(fitted):
    """simulate_missing_metadata (inference_all_folds.py:116-140): NaN for a numeric, "EMPTY" for a categorical -- a column whose
    "EMPTY" was unseen at fit time ("bleed") then encodes as an all-zero block"""
    cats, num, ohe, scaler, enc = fitted
    sw = MetadataSweep(None, enc, "cpu", out_width=18)
    rates, seeds = [0.0, 0.3, 0.9], [5, 305, 905]
    tab, mask = sw.missing_variants(rates, len(cats), NUM_NAMES, CAT_NAMES, seeds)
    missing = sw._missing_codes()
    assert missing[3] == -1 and (missing[:3] >= 0).all() and not mask[0].any() and not mask[1].any() and mask[3].mean() > 0.8
    off = np.concatenate([[0], np.cumsum([len(c) for c in enc.categories_])])
    got = so.variants(enc.codes(cats).numpy(), num, off, enc.mean_, enc.scale_, enc.nan_fill, tab, 18, mask=mask, missing_code=missing)
    for i, (rate, seed) in enumerate(zip(rates, seeds), start=1):
        df = mutate_like_the_reference(cats, num, None, ("none",))
        keep = np.random.default_rng(seed).random((len(df), 7)) < (1 - rate)                      # the reference's draw, its order
        for j, col in enumerate(NUM_NAMES + CAT_NAMES):
            df[col] = df[col].astype(object)
            df.loc[~keep[:, j], col] = np.nan if col in NUM_NAMES else "EMPTY"
        want = encode_like_the_reference(df, ohe, scaler, 18)
        assert np.array_equal(got[i][:, :13], want[:, :13]), rate
        assert np.allclose(got[i][:, 13:], want[:, 13:], rtol=1e-5, atol=1e-5), rate
    # the mask is the reference's draw rearranged from [numeric | categorical] to [categorical | numeric]
    keep = np.random.default_rng(905).random((len(cats), 7)) < (1 - 0.9)
    assert np.array_equal(mask[3].astype(bool), ~np.concatenate([keep[:, 3:], keep[:, :3]], axis=1))


# ------------------------------------------------------------------------------------------- reduce against float64
@pytest.mark.parametrize("V,B,C", so.REDUCE_SHAPES)
def test_oracle_reduce_matches_float64(V, B, C):
    """integer outputs and the margin exactly, the continuous ones within the recorded error of fp32 arithmetic"""
    logits, base, labels = so.reduce_case(V, B, C)
    got, want = so.reduce(logits, base, labels), so.reduce(logits, base, labels, dt=np.float64)
    for key in ("pred", "flips", "transitions", "confusion"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["margin"], want["margin"].astype(np.float32))
    assert got["transitions"].sum() == V * B and got["confusion"].sum() == V * (B - (B > 2))      # one label out of range
    assert got["flips"][0] == 0 and not got["stats"][0, :, 1:].any()                               # variant 0 is the baseline
    if V > 1:
        assert got["pred"][1, 0] == min(np.flatnonzero(logits[1, 0] == logits[1, 0].max())) and got["margin"][1, 0] == 0     # tie
        assert not got["stats"][-1, B - 1, 1:].any()                                               # a row equal to its baseline
    err = so.continuous_errors(got, want)
    print(f"V {V} B {B} C {C}: fp32 restatement against float64: {err}")
    for name, e in err.items():
        assert e <= REDUCE_F32_ERROR[name], (name, e)


@pytest.mark.parametrize("V,B,C", so.ROWWISE_SHAPES)
def test_vectorised_float64_equals_the_reference_formulas_row_by_row(V, B, C):
    logits, base, labels = so.reduce_case(V, B, C)
    got, want = so.reduce(logits, base, labels, dt=np.float64), so.reduce64(logits, base, labels)
    for key in ("pred", "flips", "transitions", "confusion"):
        assert np.array_equal(got[key], want[key]), key
    for key in ("probs", "margin", "stats"):
        assert np.allclose(got[key], want[key], rtol=0, atol=1e-12), key


# ------------------------------------------------------------------------------------------- host logic
def _call_variants(tab, n_cat=2, n_num=1, off=(0, 3, 5), V=None, batch=4, out_width=6):
    """the library's entry point with host memory in every pointer: only calls that fail validation (nothing may be launched)"""
    lib = _lib.load()
    off = np.asarray(off, dtype=np.int32)
    buf = np.zeros(4096, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)
    rc = lib.mmskin_metadata_variants(p, n_cat, p, ctypes.c_void_p(off.ctypes.data), int(off[-1]), p, n_num, p, p, -1.0,
                                      ctypes.c_void_p(tab.ctypes.data), p, len(tab) if V is None else V, None, None, p, batch, out_width, None)
    return rc, lib.mmskin_last_error() or b""


def test_library_rejects_bad_tables_before_any_launch():
    r = so.record
    for tab, kw, word in [(so.table([r()]), dict(V=0), b"extent"), (so.table([r()]), dict(batch=0), b"extent"),
                          (so.table([r()]), dict(out_width=0), b"extent"), (so.table([r()]), dict(n_cat=0, n_num=0, off=(0,)), b"shape"),
                          (so.table([r(), r(so.CAT_SET, 3, 0)]), {}, b"outside the 3 columns"),
                          (so.table([r(so.NUM_SET, -1)]), {}, b"outside the 3 columns"),
                          (so.table([r(so.CAT_TOGGLE, 2, 0, 1)]), {}, b"categorical op on numeric column"),
                          (so.table([r(so.NUM_ADD, 1, value=2.0)]), {}, b"numeric op on categorical column"),
                          (so.table([r(so.CAT_SET, 1, 2)]), {}, b"outside the 2 categories"),
                          (so.table([r(so.CAT_TOGGLE, 0, 1, 3)]), {}, b"outside the 3 categories"),
                          (so.table([r(so.CAT_SET, 0, -2)]), {}, b"outside the 3 categories"), (so.table([r(9, 0)]), {}, b"unknown op")]:
        rc, msg = _call_variants(tab, **kw)
        assert rc == 1 and word in msg, (kw, msg)
    assert so.VARIANT_DTYPE == ops.META_VARIANT_DTYPE and ops.META_VARIANT_DTYPE.itemsize == 32
    assert [ops.META_VARIANT_DTYPE.fields[k][1] for k in ("op", "column", "a", "b", "value", "reserved")] == [0, 4, 8, 12, 16, 20]
    lib = _lib.load()
    p = ctypes.c_void_p(np.zeros(64, dtype=np.float32).ctypes.data)
    for C in (1, 65):
        assert lib.mmskin_sweep_reduce(p, 0, p, None, 1, 1, C, None, p, p, p, p, p, None, None) == 3           # MMSKIN_ERR_UNSUPPORTED
    assert lib.mmskin_sweep_reduce(p, 0, p, None, 0, 1, 6, None, p, p, p, p, p, None, None) == 1


def test_flip_variants_packs_names_and_strings_into_records(fitted):
    enc = fitted[4]
    sw = MetadataSweep(None, enc, "cpu")
    tab = sw.flip_variants({"itch": ("toggle", "True", "False"), "age": ("set", 80.0), "diameter_1": ("add", 5.0), "region": ("set", "FACE")},
                           CAT_NAMES, NUM_NAMES)
    itch, region = list(enc.categories_[0]), list(enc.categories_[2])
    want = so.table([so.record(), so.record(so.CAT_TOGGLE, 0, itch.index("True"), itch.index("False")), so.record(so.NUM_SET, 4, value=80.0),
                     so.record(so.NUM_ADD, 5, value=5.0), so.record(so.CAT_SET, 2, region.index("FACE"))])
    assert tab.tobytes() == want.tobytes()
    for spec, word in [({"colour": ("set", "RED")}, "not a column"), ({"age": ("toggle", 1, 2)}, "numeric"), ({"itch": ("add", 1.0)}, "categorical")]:
        with pytest.raises(ValueError, match=word):
            sw.flip_variants(spec, CAT_NAMES, NUM_NAMES)
    with pytest.raises(ValueError, match="names"):
        sw.flip_variants({}, CAT_NAMES[:2], NUM_NAMES)
    with pytest.raises(ValueError, match="seeds"):
        sw.missing_variants([0.1, 0.2], 4, NUM_NAMES, CAT_NAMES, [1])


def test_run_raises_before_any_gpu_call():
    enc = so.e2e_encoder()
    img, cats, num = so.e2e_case()
    codes, numeric = enc.codes(cats), torch.from_numpy(num).float()

    def sweep(**kw):
        out_width = kw.pop("out_width", None)
        model = M.MultimodalModel(**dict(SMALL, **{"attention_mecanism": "gfcam", **kw})).eval()
        sw = MetadataSweep(model, enc, "cpu", out_width=out_width)
        return sw, sw.flip_variants(so.E2E_FLIPS, so.E2E_CAT_NAMES, so.E2E_NUM_NAMES)

    sw, tab = sweep()
    sw.model.train()
    with pytest.raises(MMSkinError, match="eval"):
        sw.run(img, codes, numeric, tab)
    for kw, word in [(dict(attention_mecanism="no-metadata", n=1), "nothing to sweep"), (dict(attention_mecanism="no-metadata-without-mlp"), "nothing to sweep"),
                     (dict(out_width=18), "vocab_size")]:
        sw, tab = sweep(**kw)
        with pytest.raises(ValueError, match=word):
            sw.run(img, codes, numeric, tab)
    sw, tab = sweep()
    sw.model.text_model_name = "tab-transformer"
    with pytest.raises(ValueError, match="one-hot"):
        sw.run(img, codes, numeric, tab)
    sw, tab = sweep()
    for args, kw, word in [((img, codes[:5], numeric, tab), {}, "codes"), ((img, codes, numeric[:, :2], tab), {}, "numeric"),
                           ((img, codes, numeric, tab), dict(mask=np.zeros((17, 8, 7), dtype=np.uint8)), "mask"),
                           ((img, codes, numeric, tab), dict(labels=torch.zeros(7, dtype=torch.int64)), "labels"),
                           ((img, codes, numeric, tab[1:]), {}, "baseline"), ((img, codes, numeric, np.zeros(3)), {}, "table")]:
        with pytest.raises(ValueError, match=word):
            sw.run(*args, **kw)
    with pytest.raises(MMSkinError, match="no CPU fallback"):      # everything checks out: the first kernel call refuses the CPU
        sw.run(img, codes, numeric, tab)


# ------------------------------------------------------------------------------------------- the end-to-end condition
def e2e_oracle(mech):
    """the CPU oracle's logits [V, 8, C] of the flip sweep and of the missing sweep"""
    enc = so.e2e_encoder()
    img, cats, num = so.e2e_case()
    sw = MetadataSweep(None, enc, "cpu", out_width=20)
    off = np.concatenate([[0], np.cumsum([len(c) for c in enc.categories_])])
    model = det_init_(OracleMultimodalModel(**dict(SMALL, attention_mecanism=mech)), salt=so.E2E_SALT).eval()
    flip_tab = sw.flip_variants(so.E2E_FLIPS, so.E2E_CAT_NAMES, so.E2E_NUM_NAMES)
    miss_tab, mask = sw.missing_variants(so.E2E_RATES, 8, so.E2E_NUM_NAMES, so.E2E_CAT_NAMES, so.E2E_SEEDS)
    codes = enc.codes(cats).numpy()
    enc_args = (codes, num, off, enc.mean_, enc.scale_, enc.nan_fill)
    flip = so.oracle_loop(model, img, so.variants(*enc_args, flip_tab, 20))
    miss = so.oracle_loop(model, img, so.variants(*enc_args, miss_tab, 20, mask=mask, missing_code=sw._missing_codes()))
    return flip, miss


@pytest.mark.parametrize("mech", so.E2E_MECHS)
def test_end_to_end_inputs_flip_predictions_and_keep_clear_margins(mech):
    """What makes tests/test_gpu_sweep.py's end-to-end comparison mean something, checked on the oracle alone: at most 10 % of
    the (variant, row) pairs are too close to call, and at least half of the non-baseline variants flip some but not all rows."""
    for name, logits in zip(("flip", "missing"), e2e_oracle(mech)):
        res = so.reduce(logits, logits[0])
        close = res["margin"] < so.margin_threshold(logits)
        flips = res["flips"][1:]
        print(f"{mech} {name}: {close.mean():.3f} of the pairs below the margin threshold, flips per variant {flips.tolist()}")
        assert close.mean() <= 0.10
        assert ((flips > 0) & (flips < logits.shape[1])).sum() * 2 >= len(flips)
