"""Metadata Shapley values without a GPU: tests/shapley_oracle.py (the numpy restatement the kernels are held to by
tests/test_gpu_shapley.py) against brute-force exact Shapley values and against float64; and the host logic of mmskin.shapley
(the permutation draw, the row count, the rounding of the head-call size, the library's validation, the errors of `explain` that
fire before any GPU call)."""
import ctypes

import numpy as np
import pytest
import torch

import shapley_oracle as sh
import sweep_oracle as so
from helpers import SMALL
from mmskin import _lib, ops
from mmskin._lib import MMSkinError
from mmskin.shapley import MetadataShapley
from models import multimodalIntraInterModal as M

# Largest |fp32 restatement - float64| over shapley_oracle.REDUCE_CASES, measured on the CPU (test_oracle_reduce_matches_float64
# prints the figures); tests/test_gpu_shapley.py allows the kernels four times these
from test_gpu_shapley import REDUCE_F32_ERROR, REDUCE_KERNEL_FACTOR  # noqa: E402


# ------------------------------------------------------------------------------------------- the estimator
@pytest.mark.parametrize("P", [1, 3])
def test_walk_is_exact_for_pairwise_value_functions(P):
    """constant + linear + pairwise terms only: the antithetic walk gives the exact Shapley values already at P = 1"""
    n = 5
    v_fn = sh.polynomial_value(n, order=2, seed=3)
    rng = np.random.default_rng(P)
    perms = np.stack([rng.permutation(n) for _ in range(P)])
    got, want = sh.values(v_fn, n, perms), sh.exact(v_fn, n)
    assert got.shape == (n, 3) and np.abs(want).min() > 1e-3
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("P", [1, 3])
def test_efficiency_holds_where_the_values_are_not_exact(P):
    n = 5
    v_fn = sh.polynomial_value(n, order=3, seed=4)
    rng = np.random.default_rng(10 + P)
    perms = np.stack([rng.permutation(n) for _ in range(P)])
    got, want = sh.values(v_fn, n, perms), sh.exact(v_fn, n)
    assert np.abs(got - want).max() > 1e-3                                        # third-order terms: a sampled estimate
    ends = v_fn(np.ones(n, dtype=bool)) - v_fn(np.zeros(n, dtype=bool))
    assert np.abs(got.sum(axis=0) - ends).max() <= 1e-12 and np.abs(want.sum(axis=0) - ends).max() <= 1e-12


def test_table_walk_equals_the_walk_on_a_value_function():
    """phi_from_v on the v table in row order (walk_masks) is `values` on the function that table was read from"""
    n, P = 6, 3
    v_fn = sh.polynomial_value(n, order=3, seed=5, n_out=4)
    perms = np.stack([np.random.default_rng(1).permutation(n) for _ in range(P)])
    masks = sh.walk_masks(perms)
    assert masks.shape == (2 * P * (n - 1) + 2, n) and not masks[-2].any() and masks[-1].all()
    assert [int(m.sum()) for m in masks[:2 * (n - 1)]] == list(range(1, n)) * 2
    v = np.stack([v_fn(m) for m in masks])[None]
    assert np.abs(sh.phi_from_v(v, perms)[0] - sh.values(v_fn, n, perms)).max() <= 1e-12
    assert sh.walk_masks(np.zeros((2, 1), dtype=int)).tolist() == [[False], [True]]          # M = 1: the two ends only


# ------------------------------------------------------------------------------------------- reduce against float64
@pytest.mark.parametrize("output", ["prob", "logit"])
@pytest.mark.parametrize("B,G,P,n,C", sh.REDUCE_CASES)
def test_oracle_reduce_matches_float64(B, G, P, n, C, output):
    logits, perms = sh.reduce_case(B, G, P, n, C)
    mode = sh.PROB if output == "prob" else sh.LOGIT
    got, want = sh.reduce(logits, B, G, perms, mode), sh.reduce(logits, B, G, perms, mode, dt=np.float64)
    assert got["phi"].dtype == np.float32 and got["phi"].shape == (B, n, C) and got["base"].shape == (B, C)
    err = sh.reduce_errors(got, want)
    print(f"B {B} G {G} P {P} M {n} C {C} {output}: fp32 restatement against float64: {err}")
    assert err["phi"] <= REDUCE_F32_ERROR[output]["phi"] and err["ends"] <= REDUCE_F32_ERROR[output]["ends"]
    assert err["efficiency"] <= REDUCE_KERNEL_FACTOR * REDUCE_F32_ERROR[output]["phi"] * n       # the GPU test's efficiency bound
    assert np.abs(want["phi"].sum(axis=1) - (want["full"] - want["base"])).max() <= 1e-12 * max(1.0, np.abs(logits).max())


# ------------------------------------------------------------------------------------------- host logic
def test_permutations_row_count_and_head_call_rounding():
    enc = so.e2e_encoder()
    bg_codes, bg_num = np.zeros((7, 5), dtype=np.int32), np.zeros((7, 3), dtype=np.float32)
    a = MetadataShapley(None, enc, "cpu", bg_codes, bg_num, n_permutations=4, seed=9, rows_per_head_call=100)
    b = MetadataShapley(None, enc, "cpu", bg_codes, bg_num, n_permutations=4, seed=9)
    c = MetadataShapley(None, enc, "cpu", bg_codes, bg_num, n_permutations=4, seed=10, rows_per_head_call=3)
    assert a.permutations.dtype == np.int32 and a.permutations.shape == (4, 8) and a.n_players == 8 and a.n_background == 7
    assert np.array_equal(a.permutations, b.permutations) and not np.array_equal(a.permutations, c.permutations)
    assert all(sorted(row) == list(range(8)) for row in a.permutations.tolist())
    rng = np.random.default_rng(9)
    assert np.array_equal(a.permutations, np.stack([rng.permutation(8) for _ in range(4)]))
    assert a.rows_per_sample() == 1 + 7 + 4 * 2 * 7 * 7 == sh.n_rows(1, 7, 4, 8)
    assert ops.shapley_rows(5, 7, 4, 8) == 5 * a.rows_per_sample() == len(sh.row_plan(5, 7, 4, 8))
    assert a.rows_per_head_call == 98 and c.rows_per_head_call == 7 and b.rows_per_head_call == 8192 // 7 * 7
    assert a.column_names(so.E2E_CAT_NAMES, so.E2E_NUM_NAMES) == so.E2E_CAT_NAMES + so.E2E_NUM_NAMES
    with pytest.raises(ValueError, match="names"):
        a.column_names(so.E2E_CAT_NAMES[:2], so.E2E_NUM_NAMES)
    with pytest.raises(ValueError, match="nothing has been explained"):
        a.global_importance()
    for kw, word in [(dict(n_permutations=0), "n_permutations"), (dict(output="odds"), "output"), (dict(rows_per_head_call=0), "rows_per_head_call")]:
        with pytest.raises(ValueError, match=word):
            MetadataShapley(None, enc, "cpu", bg_codes, bg_num, **kw)
    for codes, num in [(bg_codes[:0], bg_num[:0]), (bg_codes[:, :4], bg_num), (bg_codes, bg_num[:5])]:
        with pytest.raises(ValueError, match="background"):
            MetadataShapley(None, enc, "cpu", codes, num)
    with pytest.raises(ValueError, match="shapley_rows"):
        ops.shapley_rows(1, 0, 1, 3)


def _host_calls():
    """the library's entry points with host memory in every pointer: only calls that fail validation (nothing may be launched)"""
    lib = _lib.load()
    buf = np.zeros(4096, dtype=np.float32)
    p = ctypes.c_void_p(buf.ctypes.data)
    off = np.array([0, 3, 5], dtype=np.int32)

    def coalitions(perms, batch=2, G=3, n_cat=2, n_num=1, row0=0, row1=4, out_width=6):
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        rc = lib.mmskin_shapley_coalitions(p, p, batch, p, p, G, n_cat, p, ctypes.c_void_p(off.ctypes.data), int(off[n_cat]), n_num, p, p,
                                           -1.0, ctypes.c_void_p(perms.ctypes.data), p, len(perms), row0, row1, p, out_width, None)
        return rc, lib.mmskin_last_error() or b""

    def reduce(perms, batch=2, G=3, C=6, row0=0, row1=3, finish=1, output=0, dtype=0):
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        rc = lib.mmskin_shapley_reduce(p, dtype, output, batch, G, len(perms), perms.shape[1], C, row0, row1, p, finish,
                                       ctypes.c_void_p(perms.ctypes.data), p, p, p, p, None, None)
        return rc, lib.mmskin_last_error() or b""
    return coalitions, reduce


def test_library_rejects_bad_arguments_before_any_launch():
    coalitions, reduce = _host_calls()
    good = [[2, 0, 1], [0, 1, 2]]
    total = sh.n_rows(2, 3, 2, 3)                                                 # 2 x (1 + 3 + 2 * 2 * 2 * 3) = 56
    for perms, kw, word in [([[2, 0, 1], [0, 1, 1]], {}, b"row 1 of the table is not a permutation"), ([[0, 1, 3]], {}, b"not a permutation"),
                            ([[0, -1, 2]], {}, b"not a permutation"), (good, dict(G=0), b"extent"), (good, dict(batch=0), b"extent"),
                            (good, dict(n_cat=0, n_num=0), b"shape"), (good, dict(out_width=0), b"out_width"),
                            (good, dict(row0=4, row1=4), b"not a range"), (good, dict(row1=total + 1), b"not a range"),
                            (good, dict(row0=-1), b"not a range")]:
        rc, msg = coalitions(perms, **kw)
        assert rc == 1 and word in msg, (kw, msg)
    for C in (1, 65):
        assert reduce(good, C=C)[0] == 3                                          # MMSKIN_ERR_UNSUPPORTED
    for perms, kw, word in [([[2, 0, 1], [0, 0, 2]], {}, b"not a permutation"), (good, dict(G=0), b"extent"), (np.zeros((0, 3)), {}, b"extent"),
                            (good, dict(row0=1, row1=3), b"split a coalition"), (good, dict(row1=4), b"split a coalition"),
                            (good, dict(row1=total + 1), b"not a range"), (good, dict(dtype=2), b"dtype"), (good, dict(output=2), b"output")]:
        rc, msg = reduce(perms, **kw)
        assert rc == 1 and word in msg, (kw, msg)
    assert _lib.load().mmskin_shapley_rows(2, 3, 2, 3) == total and _lib.load().mmskin_shapley_rows(2, 3, 0, 3) == -1


def test_explain_raises_before_any_gpu_call():
    enc = so.e2e_encoder()
    img, cats, num = so.e2e_case()
    codes, numeric = enc.codes(cats), torch.from_numpy(num).float()
    rows = sh.E2E_BACKGROUND_ROWS

    def explainer(**kw):
        out_width = kw.pop("out_width", None)
        model = M.MultimodalModel(**dict(SMALL, **{"attention_mecanism": "gfcam", **kw})).eval()
        return MetadataShapley(model, enc, "cpu", codes[rows], numeric[rows], n_permutations=2, out_width=out_width)

    ex = explainer()
    ex.model.train()
    with pytest.raises(MMSkinError, match="eval"):
        ex.explain(img, codes, numeric)
    for kw, word in [(dict(attention_mecanism="no-metadata", n=1), "nothing to explain"), (dict(attention_mecanism="no-metadata-without-mlp"), "nothing to explain"),
                     (dict(out_width=18), "vocab_size")]:
        with pytest.raises(ValueError, match=word):
            explainer(**kw).explain(img, codes, numeric)
    ex = explainer()
    ex.model.text_model_name = "tab-transformer"
    with pytest.raises(ValueError, match="one-hot"):
        ex.explain(img, codes, numeric)
    ex = explainer()
    for args, word in [((img, codes[:5], numeric), "codes"), ((img, codes, numeric[:, :2]), "numeric")]:
        with pytest.raises(ValueError, match=word):
            ex.explain(*args)
    with pytest.raises(MMSkinError, match="no CPU fallback"):      # everything checks out: the first kernel call refuses the CPU
        ex.explain(img, codes, numeric)
    assert ex.n_samples == 0
