"""Metadata LIME without a GPU: tests/lime_oracle.py (the numpy restatement the kernels are held to by tests/test_gpu_lime.py)
against outside knowledge -- sklearn's Ridge and StandardScaler, a literal transcription of lime's selection, a linear model whose
coefficients are known, the moments of a normal --, and the host logic of mmskin.lime (the refusals, the signatures)."""
import ctypes

import numpy as np
import pytest
import torch
from sklearn.linear_model import Ridge
from sklearn.preprocessing import StandardScaler

import lime_oracle as lo
from helpers import SMALL
from mmskin import _lib, ops
from mmskin._lib import MMSkinError
from mmskin.lime import LimeResult, MetadataLime
from models import multimodalIntraInterModal as M

# the neighbourhood cases of tests/test_gpu_lime.py and the largest |z(float32 rows) - z(float64 rows)| / max(1, |z|) over them
from test_gpu_lime import NEIGHBOUR_CASES, NORMAL_F32_ERROR  # noqa: E402


def problem(N=2000, F=91, seed=0, C=3):
    rng = np.random.default_rng(seed)
    mean, scale, x = lo.case_stats(F, seed)
    rows = lo.neighbourhood(x[:1], mean, scale, N, seed)
    z, w = lo.standardise(rows, mean, scale)[0], lo.kernel_weights(rows, mean, scale)[0]
    y = lo.softmax32(rng.normal(0, 1, (N, C)) + z[:, :C] * rng.normal(0, 1, C)).astype(np.float64)
    return z, y, w


# ------------------------------------------------------------------------------------------- the ridge against sklearn
@pytest.mark.parametrize("alpha", [0.01, 1.0])
def test_ridge_equals_sklearn_with_sample_weights(alpha):
    z, y, w = problem()
    assert 0 < w[1:].min() and w[1:].max() < 1 and w[0] == 1.0
    for keep in (None, np.array([0, 3, 4, 17, 40, 88, 90])):
        zs = z if keep is None else z[:, keep]
        for c in range(y.shape[1]):
            beta, icpt, score = lo.ridge_fit(z, y[:, c], w, alpha, keep)
            ref = Ridge(alpha=alpha, fit_intercept=True).fit(zs, y[:, c], sample_weight=w)
            err = max(np.abs(beta - ref.coef_).max(), abs(icpt - ref.intercept_), abs(score - ref.score(zs, y[:, c], sample_weight=w)))
            print(f"alpha {alpha} class {c}: closed form against sklearn {err:.3e}")
            assert err <= 1e-10


def test_selection_equals_the_literal_transcription():
    """lime_base.feature_selection 'highest_weights': sorted(zip(range(F), coef * data[0]), key=|.|, reverse=True)[:K]"""
    z, y, w = problem(seed=1)
    z[0, 5] = z[0, 9] = 0.0                                                       # ties at zero: the lower index first
    for c in range(y.shape[1]):
        clf = Ridge(alpha=0.01, fit_intercept=True).fit(z, y[:, c], sample_weight=w)
        weighted = clf.coef_ * z[0]
        ranked = sorted(zip(range(z.shape[1]), weighted), key=lambda t: np.abs(t[1]), reverse=True)     # python's sort is stable
        for K in (7, 15, 90, 91):
            keep, gap = lo.select(lo.ridge_fit(z, y[:, c], w, 0.01)[0], z[0], K)
            assert keep.tolist() == sorted(j for j, _ in ranked[:K]) and gap >= 0
    keep, _ = lo.select(np.array([1.0, -1.0, 0.5, 1.0]), np.ones(4), 2)
    assert keep.tolist() == [0, 1]


def test_explain_is_the_two_ridges_in_sequence():
    z, y, w = problem(N=500, F=21, seed=2)
    got = lo.explain(z, y, w, 7)
    for c in range(y.shape[1]):
        first = Ridge(alpha=0.01).fit(z, y[:, c], sample_weight=w)
        keep = np.sort(np.argsort(-np.abs(first.coef_ * z[0]), kind="stable")[:7])
        ref = Ridge(alpha=1.0).fit(z[:, keep], y[:, c], sample_weight=w)
        order = np.argsort(-np.abs(ref.coef_), kind="stable")
        assert got["feature"][c].tolist() == keep[order].tolist()
        assert np.abs(got["coef"][c] - ref.coef_[order]).max() <= 1e-10 and abs(got["intercept"][c] - ref.intercept_) <= 1e-10
        assert abs(got["local_pred"][c] - ref.predict(z[:1, keep])[0]) <= 1e-10
        assert abs(got["score"][c] - ref.score(z[:, keep], y[:, c], sample_weight=w)) <= 1e-10
        assert np.array_equal(np.flatnonzero(got["dense"][c]), keep)


def test_scaler_equals_standardscaler_with_a_constant_column():
    rng = np.random.default_rng(3)
    rows = rng.normal(2, 3, (40, 6))
    rows[:, 2] = 1.0
    ref = StandardScaler().fit(rows)
    for fit in (lo.fit_scaler, MetadataLime.fit_scaler):
        mean, scale = fit(rows)
        assert np.abs(mean - ref.mean_).max() <= 1e-14 and np.abs(scale - ref.scale_).max() <= 1e-14 and scale[2] == 1.0


def test_a_linear_model_is_recovered():
    """y = a + z b exactly, every feature kept, alpha -> 0: the coefficients are b, the intercept a, the score 1"""
    z, _, w = problem(N=400, F=21, seed=4)
    rng = np.random.default_rng(4)
    b, a = rng.normal(0, 1, (21, 2)), np.array([0.3, -1.2])
    got = lo.explain(z, a + z @ b, w, 21, alpha_select=1e-12, alpha_fit=1e-12)
    for c in range(2):
        assert np.abs(got["dense"][c] - b[:, c]).max() <= 1e-9 and abs(got["intercept"][c] - a[c]) <= 1e-9
        assert abs(got["score"][c] - 1) <= 1e-12 and abs(got["local_pred"][c] - (a[c] + z[0] @ b[:, c])) <= 1e-9
        assert np.array_equal(got["feature"][c], np.argsort(-np.abs(b[:, c]), kind="stable"))


# ------------------------------------------------------------------------------------------- the generator
def test_generator_moments():
    s, f = np.meshgrid(np.arange(10000), np.arange(100), indexing="ij")
    for seed, sample, dt in [(0, 0, np.float64), (0, 0, np.float32), (12345, 7, np.float64)]:
        n = lo.normals(seed, sample, s, f, dt).astype(np.float64)
        assert n.size == 10 ** 6 and np.isfinite(n).all()
        print(f"seed {seed} sample {sample} {dt.__name__}: mean {n.mean():+.3e} var {n.var():.5f} max |n| {np.abs(n).max():.3f}")
        assert abs(n.mean()) < 5e-3 and abs(n.var() - 1) < 1e-2
        assert abs((n ** 3).mean()) < 2e-2 and abs((n ** 4).mean() - 3) < 5e-2
    a, b = lo.normals(0, 0, s[:100], f[:100]), lo.normals(0, 1, s[:100], f[:100])
    assert abs(np.corrcoef(a.ravel(), b.ravel())[0, 1]) < 5e-2                    # another sample: another stream
    assert np.array_equal(a, lo.normals(0, 0, s[:100], f[:100]))
    u1, u2 = lo.uniforms(9, 3, s, f)
    assert 0 < u1.min() and u1.max() < 1 and 0 < u2.min() and u2.max() < 1
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1)           # exact in float32


def test_float32_rows_stay_within_the_recorded_error_of_float64():
    """the constant the GPU test scales its bound from: the float32 formula's own error, on the GPU test's counters"""
    worst = 0.0
    for F, extra, N, B, seed in NEIGHBOUR_CASES:
        mean, scale, x = lo.case_stats(F, seed)
        for around in (False, True):
            z32 = lo.standardise(lo.neighbourhood(x[:B], mean, scale, N, seed, around=around), mean, scale)
            z64 = lo.standardise(lo.neighbourhood(x[:B], mean, scale, N, seed, around=around, dt=np.float64), mean, scale)
            err = float((np.abs(z32 - z64) / np.maximum(1.0, np.abs(z64))).max())
            print(f"F {F} N {N} B {B} around {around}: float32 rows against float64 {err:.4e}")
            worst = max(worst, err)
    assert worst <= NORMAL_F32_ERROR and worst >= 0.5 * NORMAL_F32_ERROR          # the recorded figure is the measured one


# ------------------------------------------------------------------------------------------- host logic
def test_signatures_and_symbols_exist():
    names = ["mmskin_lime_accumulator_doubles", "mmskin_lime_solve_workspace_bytes", "mmskin_lime_neighbourhood", "mmskin_lime_reduce",
             "mmskin_lime_solve"]
    lib = _lib.load()
    for n in names:
        assert n in _lib._SIGNATURES and n in _lib.declared_symbols() and hasattr(lib, n)
    assert lib.mmskin_lime_accumulator_doubles(2, 5000, 91, 6) == 2 * 20 * (92 * 98 + 6)
    assert lib.mmskin_lime_accumulator_doubles(1, 256, 5, 2) == 6 * 8 + 2 and lib.mmskin_lime_accumulator_doubles(1, 257, 5, 2) == 2 * 50
    assert lib.mmskin_lime_accumulator_doubles(1, 64, 129, 2) == -1 and lib.mmskin_lime_solve_workspace_bytes(1, 129, 2) == -1
    assert lib.mmskin_lime_solve_workspace_bytes(2, 91, 6) >= 2 * (92 * 98 + 6) * 8 + 12 * 4


def test_library_rejects_bad_arguments_before_any_launch():
    """host memory in every pointer: only calls that fail validation (nothing may be launched)"""
    lib = _lib.load()
    buf = np.zeros(4096, dtype=np.float64)
    p = ctypes.c_void_p(buf.ctypes.data)

    def neighbourhood(batch=2, F=5, N=64, row0=0, row1=128, out_width=5, x_stride=5, w_dtype=1, sample0=0, out=p):
        rc = lib.mmskin_lime_neighbourhood(p, x_stride, batch, p, p, F, N, 0, sample0, 0, row0, row1, out, out_width, p, w_dtype, None)
        return rc, lib.mmskin_last_error() or b""

    def reduce(batch=2, F=5, N=64, C=3, row0=0, row1=128, width=5, w_dtype=1, dtype=0, output=0, acc=p):
        rc = lib.mmskin_lime_reduce(p, width, p, w_dtype, p, dtype, output, p, p, batch, N, F, C, row0, row1, acc, None)
        return rc, lib.mmskin_last_error() or b""

    def solve(batch=2, F=5, N=64, C=3, K=5, x_stride=5, coef=p):
        rc = lib.mmskin_lime_solve(p, p, x_stride, p, p, batch, N, F, C, K, coef, p, p, p, p, None, None, p, None)
        return rc, lib.mmskin_last_error() or b""

    for fn, cases in [(neighbourhood, [(dict(F=129, out_width=129, x_stride=129), b"at most 128"), (dict(batch=0), b"extent"), (dict(N=0), b"extent"),
                                       (dict(row0=5, row1=4), b"not a range"), (dict(row1=129), b"not a range"), (dict(row0=-1), b"not a range"),
                                       (dict(out_width=4), b"out_width"), (dict(x_stride=4), b"x_stride"), (dict(w_dtype=2), b"weight dtype"),
                                       (dict(sample0=2 ** 24 - 1), b"2^24"), (dict(out=None), b"null")]),
                      (reduce, [(dict(F=129, width=129), b"at most 128"), (dict(C=65), b"classes"), (dict(C=0), b"classes"),
                                (dict(row0=5, row1=4), b"not a range"), (dict(row1=129), b"not a range"), (dict(width=4), b"width"),
                                (dict(w_dtype=3), b"weight dtype"), (dict(dtype=2), b"logits dtype"), (dict(output=2), b"output"),
                                (dict(acc=None), b"null")]),
                      (solve, [(dict(F=129, x_stride=129, K=15), b"at most 128"), (dict(K=6), b"num_features"), (dict(K=0), b"num_features"),
                               (dict(C=0), b"classes"), (dict(x_stride=3), b"x_stride"), (dict(coef=None), b"null")])]:
        for kw, word in cases:
            rc, msg = fn(**kw)
            assert rc == 1 and word in msg, (fn.__name__, kw, msg)


def stub_model(**kw):
    return M.MultimodalModel(**dict(SMALL, **{"attention_mecanism": "gfcam", **kw})).eval()


def test_metadata_lime_refusals():
    rng = np.random.default_rng(5)
    train = rng.normal(0, 1, (30, 20))
    images, rows = torch.zeros((2, 3, 32, 32)), torch.zeros((2, 20))
    for kw, word in [(dict(num_features=6), "forward_selection"), (dict(num_features=1), "forward_selection"), (dict(output="odds"), "output"),
                     (dict(num_samples=1), "num_samples"), (dict(rows_per_head_call=0), "rows_per_head_call")]:
        with pytest.raises(ValueError, match=word):
            MetadataLime(None, None, "cpu", train, **kw)
    with pytest.raises(ValueError, match="at most 128"):
        MetadataLime(None, None, "cpu", rng.normal(0, 1, (4, 129)))
    with pytest.raises(ValueError, match="training_rows"):
        MetadataLime(None, None, "cpu", np.zeros((0, 20)))
    ex = MetadataLime(stub_model(), None, "cpu", train, num_samples=64, num_features=40)
    assert ex.num_features == 20 and ex.kernel_width == 0.75 * np.sqrt(20) and ex.mean.dtype == np.float64      # num_features >= F keeps all
    with pytest.raises(ValueError, match="nothing has been explained"):
        ex.global_importance()
    ex.model.train()
    with pytest.raises(MMSkinError, match="eval"):
        ex.explain(images, rows)
    for kw, word in [(dict(attention_mecanism="no-metadata", n=1), "nothing to explain"), (dict(attention_mecanism="no-metadata-without-mlp"), "nothing to explain"),
                     (dict(vocab_size=18), "vocab_size")]:
        with pytest.raises(ValueError, match=word):
            MetadataLime(stub_model(**kw), None, "cpu", train, num_samples=64).explain(images, rows)
    ex = MetadataLime(stub_model(), None, "cpu", train, num_samples=64)
    ex.model.text_model_name = "tab-transformer"
    with pytest.raises(ValueError, match="one-hot"):
        ex.explain(images, rows)
    ex = MetadataLime(stub_model(), None, "cpu", train, num_samples=64)
    with pytest.raises(ValueError, match="encoded rows"):
        ex.explain(images, rows[:, :19])
    with pytest.raises(MMSkinError, match="no CPU fallback"):      # everything checks out: the first kernel call refuses the CPU
        ex.explain(images, rows)
    assert ex.n_samples == 0
    with pytest.raises(ValueError, match="lime_accumulator"):
        ops.lime_accumulator(1, 64, 129, 2, "cpu")


def test_result_lists_names_in_the_order_of_the_coefficients():
    res = LimeResult(torch.tensor([[[2, 0]]], dtype=torch.int32), torch.tensor([[[-0.5, 0.25]]], dtype=torch.float64), None, None, None,
                     torch.zeros((1, 1, 3), dtype=torch.float64), torch.ones((3, 1), dtype=torch.float64), 4)
    assert res.as_list(0, 0, ["a", "b", "c"]) == [("c", -0.5), ("a", 0.25)] and res.as_list(0, 0) == [("2", -0.5), ("0", 0.25)]
    assert float(res.mean_abs[0, 0]) == 0.25
    with pytest.raises(ValueError, match="names"):
        res.as_list(0, 0, ["a"])
