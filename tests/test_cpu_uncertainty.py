"""Predictive uncertainty without a GPU: the refusals of the three entry points of csrc/uncertainty.hip (they launch nothing), the
dropout stream and the Monte-Carlo dropout switch, and tests/uncertainty_oracle.py (the numpy restatement the kernels are held to
by tests/test_gpu_uncertainty_ops.py and tests/test_gpu_uncertainty.py) against closed forms."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import uncertainty_oracle as uo
from helpers import SMALL
from mmskin import _autograd, _lib, ops
from mmskin._autograd import _dropout_state, dropout_stream
from mmskin._lib import MMSkinError
from mmskin.uncertainty import PredictiveUncertainty, RiskCoverage, mc_dropout_mode

NAMES = ("mmskin_dihedral_views", "mmskin_uncertainty_reduce", "mmskin_risk_coverage", "mmskin_risk_coverage_summary")


# ------------------------------------------------------------------------------------------------------- the C entry points
def test_symbols_are_declared_bound_and_built():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for name in NAMES:
        assert name in _lib._SIGNATURES and name in declared and hasattr(lib, name), name
    import mmskin
    assert mmskin.PredictiveUncertainty is PredictiveUncertainty and "PredictiveUncertainty" in mmskin.__all__
    assert ops.UNCERTAINTY_STATS == uo.STATS and ops.RISK_COVERAGE_SUMMARY == uo.SUMMARY
    assert ops.view_ids(ops.VIEWS_FLIPS) == [0, 2, 4, 6] and ops.view_ids(ops.VIEWS_DIHEDRAL) == list(range(8))


def test_c_entry_points_refuse_without_a_device():
    lib = _lib.load()
    one, two = ctypes.c_void_p(64), ctypes.c_void_p(4096)                            # never dereferenced: the checks come first

    def refused(rc, code, word):
        assert rc == code
        assert word in lib.mmskin_last_error().decode(), (word, lib.mmskin_last_error().decode())

    ARG, UNSUPPORTED = 1, 3
    views = lib.mmskin_dihedral_views
    refused(views(one, two, 2, 3, 8, 8, 4, 0, None), ARG, "view_mask")                # an empty mask
    refused(views(one, two, 2, 3, 8, 8, 4, 0x100, None), ARG, "view_mask")
    for mask in (0x02, 0x08, 0x20, 0x80, 0xFF):
        refused(views(one, two, 2, 3, 7, 9, 4, mask, None), ARG, "H == W")            # a quarter turn of a non-square plane
    for eb in (0, 3, 8):
        refused(views(one, two, 2, 3, 8, 8, eb, 1, None), ARG, "elem_bytes")
    for shape in ((0, 3, 8, 8), (2, 0, 8, 8), (2, 3, 0, 8), (2, 3, 8, -1)):
        refused(views(one, two, *shape, 4, 1, None), ARG, "extent")
    refused(views(one, one, 2, 3, 8, 8, 4, 1, None), ARG, "src == dst")
    refused(views(None, two, 2, 3, 8, 8, 4, 1, None), ARG, "null")
    refused(views(one, None, 2, 3, 8, 8, 4, 1, None), ARG, "null")

    red = lib.mmskin_uncertainty_reduce
    out = [one] * 5
    for T in (0, ops.UNCERTAINTY_MAX_PASSES + 1):
        refused(red(one, 60, 6, T, 10, 6, *out, None), UNSUPPORTED, "MMSKIN_UNCERTAINTY_MAX_PASSES")
    for C in (1, 65):
        refused(red(one, 10 * C, C, 4, 10, C, *out, None), UNSUPPORTED, "MMSKIN_UNCERTAINTY_MAX_CLASSES")
    for N in (0, (1 << 24) + 1):
        refused(red(one, 60, 6, 4, N, 6, *out, None), ARG, "N =")
    refused(red(one, 60, 5, 4, 10, 6, *out, None), ARG, "row_stride")
    refused(red(one, -1, 6, 4, 10, 6, *out, None), ARG, "pass_stride")
    for k in range(5):
        refused(red(one, 60, 6, 4, 10, 6, *[None if j == k else one for j in range(5)], None), ARG, "null")
    refused(red(None, 60, 6, 4, 10, 6, *out, None), ARG, "null")

    for N in (0, ops.BOOTSTRAP_MAX_ROWS + 1):
        refused(lib.mmskin_risk_coverage(one, one, N, one, None), UNSUPPORTED, "MMSKIN_BOOTSTRAP_MAX_ROWS")
        refused(lib.mmskin_risk_coverage_summary(one, one, N, one, None), UNSUPPORTED, "MMSKIN_BOOTSTRAP_MAX_ROWS")
    refused(lib.mmskin_risk_coverage(None, one, 5, one, None), ARG, "null")
    refused(lib.mmskin_risk_coverage(one, None, 5, one, None), ARG, "null")
    refused(lib.mmskin_risk_coverage(one, one, 5, None, None), ARG, "null")
    refused(lib.mmskin_risk_coverage_summary(None, one, 5, one, None), ARG, "null")
    refused(lib.mmskin_risk_coverage_summary(one, one, 5, None, None), ARG, "null")


def test_python_limits_and_arguments_need_no_device():
    for kw, word in ((dict(T=0), "MAX_PASSES"), (dict(T=4097), "MAX_PASSES"), (dict(C=1), "MAX_CLASSES"), (dict(C=65), "MAX_CLASSES"),
                     (dict(N=0), "MAX_ROWS")):
        with pytest.raises(MMSkinError, match=word):
            ops.uncertainty_check_limits("t", **kw)
    ops.uncertainty_check_limits("t", T=4096, C=64, N=1 << 24)
    with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_ROWS"):
        ops.risk_coverage_check_limits("t", ops.BOOTSTRAP_MAX_ROWS + 1)
    with pytest.raises(MMSkinError, match="HIP device"):
        ops.uncertainty_reduce(torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="rows_per_head_call"):
        PredictiveUncertainty(None, "cpu", rows_per_head_call=0)
    with pytest.raises(ValueError, match="images_per_model_call"):
        PredictiveUncertainty(None, "cpu", images_per_model_call=0)
    pu = PredictiveUncertainty(nn.Linear(2, 2).eval(), "cpu")
    with pytest.raises(TypeError, match="encode_image"):
        pu.mc_dropout(torch.zeros(2, 3, 8, 8), torch.zeros(2, 2))
    with pytest.raises(ValueError, match="views"):
        pu.tta(torch.zeros(2, 3, 8, 8), torch.zeros(2, 2), views="rotations")
    with pytest.raises(ValueError, match="view ids"):
        pu.tta(torch.zeros(2, 3, 8, 8), torch.zeros(2, 2), views=[0, 8])
    with pytest.raises(ValueError, match="fp32"):
        pu.from_logits(torch.zeros(2, 3, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="labels"):
        pu.from_logits(torch.zeros(2, 3, 4), labels=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="no rows"):
        pu.risk_coverage()
    with pytest.raises(ValueError, match="score must be one of"):
        pu.score("entropy")
    with pytest.raises(ValueError, match="no rows"):
        pu.save("nowhere")


# ------------------------------------------------------------------------------------------------------- the dropout stream
def test_dropout_stream_hands_out_its_own_seed_and_offsets():
    torch.manual_seed(1234)
    _dropout_state(0.5, 7)                                                            # the global counter is somewhere past 0
    before = _autograd._dropout_counter[0]
    assert before >= 7
    with dropout_stream(99):
        assert _dropout_state(0.5, 10) == (99, 0)
        assert _dropout_state(0.0, 1000) == (0, 0)                                    # p = 0 draws nothing, as outside
        assert _dropout_state(0.3, 5) == (99, 10)
        with dropout_stream(-1):                                                      # nested: the innermost, seeds as 64 unsigned bits
            assert _dropout_state(0.1, 4) == (0xFFFFFFFFFFFFFFFF, 0)
        assert _dropout_state(0.5, 1) == (99, 15)
    assert _autograd._dropout_counter[0] == before and not _autograd._dropout_streams
    assert _dropout_state(0.5, 3) == (1234, before)                                   # outside: as before
    assert _autograd._dropout_counter[0] == before + 3
    with pytest.raises(RuntimeError, match="boom"):
        with dropout_stream(5):
            _dropout_state(0.5, 11)
            raise RuntimeError("boom")
    assert _autograd._dropout_counter[0] == before + 3 and not _autograd._dropout_streams
    with dropout_stream(99):                                                          # a new stream starts at 0 again
        assert _dropout_state(0.5, 10) == (99, 0)


# ------------------------------------------------------------------------------------------------------- mc_dropout_mode
def small_model(mech="metablock"):
    from models import multimodalIntraInterModal as M
    return M.MultimodalModel(**dict(SMALL, attention_mecanism=mech)).eval()


def test_mc_dropout_mode_flips_exactly_the_dropouts_outside_the_encoder():
    model = small_model()
    model.image_encoder.add_module("probe_dropout", nn.Dropout(0.2))                  # a dropout INSIDE the encoder: must stay off
    model.eval()
    inside = {id(m) for m in model.image_encoder.modules()}
    drops = [m for m in model.modules() if isinstance(m, nn.Dropout) and id(m) not in inside]
    assert len(drops) >= 4                                                            # the two heads' Dropout(0.5) and Dropout(0.3) at least
    assert {0.5, 0.3} <= {m.p for m in drops}
    flags = lambda: {name: m.training for name, m in model.named_modules()}
    before = flags()
    assert not any(before.values())
    with mc_dropout_mode(model) as switched:
        assert {id(m) for m in switched} == {id(m) for m in drops}
        now = flags()
        on = {name for name, f in now.items() if f}
        assert on == {name for name, m in model.named_modules() if any(m is d for d in drops)}
        assert not model.training and not model.image_encoder.probe_dropout.training
    assert flags() == before
    drops[0].training = True                                                          # a flag that was on before stays on after
    with pytest.raises(RuntimeError, match="boom"):
        with mc_dropout_mode(model):
            assert all(m.training for m in drops)
            raise RuntimeError("boom")
    assert drops[0].training and not any(m.training for m in drops[1:]) and not model.training


def test_mc_dropout_refuses_a_model_in_train_mode_before_touching_it():
    model = small_model().train()
    pu = PredictiveUncertainty(model, "cpu")
    with pytest.raises(MMSkinError, match="eval mode"):
        pu.mc_dropout(torch.zeros(2, 3, 32, 32), torch.zeros(2, 20), passes=2)
    with pytest.raises(MMSkinError, match="eval mode"):
        pu.tta(torch.zeros(2, 3, 32, 32), torch.zeros(2, 20))
    assert pu.n_samples == 0 and model.training


# ------------------------------------------------------------------------------------------------------- the oracle, closed forms
def test_views_are_the_eight_symmetries_of_the_square():
    x = np.arange(2 * 3 * 4 * 4).reshape(2, 3, 4, 4)
    got = uo.views(x, 0xFF)
    assert got.shape == (8, 2, 3, 4, 4) and len({g.tobytes() for g in got}) == 8
    assert np.array_equal(got[0], x) and np.array_equal(got[7], x.swapaxes(-1, -2)) and np.array_equal(got[4], x[..., ::-1])
    assert np.array_equal(got[6], x[..., ::-1, :]) and np.array_equal(got[2], x[..., ::-1, ::-1])
    i, j = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")                     # the index table of mmskin.h
    assert np.array_equal(got[1], x[..., j, 3 - i]) and np.array_equal(got[3], x[..., 3 - j, i]) and np.array_equal(got[5], x[..., 3 - j, 3 - i])
    for v in range(8):
        t = torch.rot90(torch.from_numpy(x), v & 3, (2, 3))
        assert np.array_equal(got[v], (torch.flip(t, (3,)) if v & 4 else t).numpy())
    y = np.arange(2 * 7 * 9).reshape(2, 1, 7, 9)
    assert uo.views(y, 0x55).shape == (4, 2, 1, 7, 9)


@pytest.mark.parametrize("C", [2, 6, 64])
def test_reduce_closed_forms(C):
    T = 5
    r = uo.reduce(np.full((T, 3, C), 1.75, dtype=np.float32))                         # equal logits
    assert np.abs(r["stats"][:, 2] - np.log(C)).max() <= 1e-15 * np.log(C) * 4 and np.abs(r["stats"][:, 3] - np.log(C)).max() <= 1e-14
    assert (r["stats"][:, 4] <= 1e-14).all() and (r["stats"][:, 5] == 0).all() and (r["pred"] == 0).all()
    assert (r["votes"][:, 0] == T).all() and not r["votes"][:, 1:].any() and np.abs(r["stats"][:, 0] - 1.0 / C).max() <= 1e-16
    assert (r["stats"][:, 1] == 0).all() and (r["prob_std"] <= 1e-16).all() and (r["stats"][:, 6] <= 1e-16).all()   # 5 p / 5 may round
    z = np.full((2, 1, C), -1e4, dtype=np.float32)                                    # two passes, one-hot on different classes
    z[0, 0, C - 1], z[1, 0, 0] = 1e4, 1e4
    r = uo.reduce(z)
    s = r["stats"][0]
    assert abs(s[2] - np.log(2)) <= 1e-15 and s[3] == 0 and abs(s[4] - np.log(2)) <= 1e-15 and s[5] == 0.5 and s[0] == 0.5
    assert s[1] == 0                                                                  # the two classes share the top: margin 0
    assert r["pred"][0] == 0 and r["votes"][0, 0] == 1 and r["votes"][0, C - 1] == 1 and s[6] == 0.5
    assert r["mean_prob"][0, 0] == 0.5 and r["prob_std"][0, C - 1] == 0.5


def test_reduce_flags_a_non_finite_row_and_only_that_row():
    z = uo.reduce_case(5, 65, 7)
    r = uo.reduce(z)
    assert r["pred"][4] == -1 and np.isnan(r["stats"][4]).all() and np.isnan(r["mean_prob"][4]).all() and not r["votes"][4].any()
    rest = np.arange(65) != 4
    assert np.isfinite(r["stats"][rest]).all() and (r["pred"][rest] >= 0).all() and (r["votes"][rest].sum(axis=1) == 5).all()
    assert r["pred"][3] == 7 // 2 and r["votes"][3, 7 // 2] == 5 and r["stats"][3, 1] == 0     # the planted tie: the first index
    assert np.abs(r["mean_prob"][rest].sum(axis=1) - 1).max() <= 1e-14
    p = np.exp(z[:, rest].astype(np.float64) - z[:, rest].max(axis=2, keepdims=True))
    p /= p.sum(axis=2, keepdims=True)
    assert uo.close(r["mean_prob"][rest], p.mean(axis=0)) and uo.close(r["prob_std"][rest], p.std(axis=0))
    one = uo.reduce(z[:, 10:21])                                                      # a row does not depend on its neighbours
    for k in one:
        assert np.array_equal(one[k], r[k][10:21], equal_nan=True), k


def test_risk_coverage_closed_forms():
    N = 40
    wrong = np.zeros(N, dtype=np.uint8)
    wrong[-7:] = 1
    s = np.arange(N, dtype=np.float64)                                                # a perfect ranking: the errors are the least sure
    c = uo.risk_counts(s, wrong)
    assert c[:, 0].tolist() == list(range(N)) and (c[:, 1] == 1).all()
    m = uo.risk_summary(c, wrong)
    assert m[0] == m[1] and m[2] == 0 and m[3] == 1.0 and m[4] == 7 / N and m[5:].tolist() == [N, 7, N]
    assert abs(m[1] - sum((k - 33) / k for k in range(34, 41)) / N) <= 1e-16
    m = uo.risk_summary(uo.risk_counts(-s, wrong), wrong)                             # the worst ranking
    assert m[3] == 0.0 and abs(m[0] - (sum(1.0 for k in range(1, 8)) + sum(7 / k for k in range(8, 41))) / N) <= 1e-15
    tied = np.full(N, 0.5)                                                            # all tied: e(k) = k E / N, so AURC = the error rate
    c = uo.risk_counts(tied, wrong)
    assert (c == [0, N, 0, 7]).all()
    m = uo.risk_summary(c, wrong)
    assert abs(m[0] - 7 / N) <= 1e-15 and m[3] == 0.5 and m[7] == 1
    for w, rate in ((np.zeros(N, dtype=np.uint8), 0.0), (np.ones(N, dtype=np.uint8), 1.0)):
        m = uo.risk_summary(uo.risk_counts(s, w), w)
        assert m[0] == rate and m[1] == rate and m[2] == 0 and np.isnan(m[3]) and m[4] == rate
    cov, risk = uo.risk_curve(uo.risk_counts(s, wrong))
    assert cov[-1] == 1.0 and risk[-1] == 7 / N and (risk[:33] == 0).all() and len(cov) == N


@pytest.mark.parametrize("N", [1, 2, 65, 257])
def test_risk_counts_equal_the_quadratic_definition_and_sklearn_auc(N):
    for scores in uo.RISK_SCORES:
        s, w = uo.risk_case(N, scores, "drawn")
        c = uo.risk_counts(s, w)
        lt, eq = s[None, :] < s[:, None], s[None, :] == s[:, None]
        want = np.stack([lt.sum(1), eq.sum(1), (lt & (w[None, :] != 0)).sum(1), (eq & (w[None, :] != 0)).sum(1)], axis=1)
        assert np.array_equal(c, want)
        m = uo.risk_summary(c, w)
        # AURC as the mean over many random orders of the ties is the formula's expectation; one exact check: the tie-free case
        if scores == "distinct":
            order = np.argsort(s, kind="stable")
            e = np.cumsum(w[order] != 0)
            assert abs(m[0] - float((e / np.arange(1, N + 1)).sum()) / N) <= 1e-14
        if 0 < w.sum() < N:
            metrics = pytest.importorskip("sklearn.metrics")
            assert abs(m[3] - metrics.roc_auc_score(w, s)) <= 1e-12


def test_risk_coverage_object_reads_the_curve_on_the_host():
    s, w = uo.risk_case(65, "eighths", "drawn")
    c = uo.risk_counts(s, w)
    rc = RiskCoverage("variation_ratio", torch.from_numpy(c), torch.from_numpy(uo.risk_summary(c, w)))
    cov, risk = rc.curve()
    want_cov, want_risk = uo.risk_curve(c)
    assert np.array_equal(cov.numpy(), want_cov) and np.array_equal(risk.numpy(), want_risk)
    assert rc.n == 65 and rc.n_wrong == int(w.sum()) and rc.n_distinct == len(want_cov) and rc.aurc == uo.risk_summary(c, w)[0]
    assert rc.risk_at_coverage(1.0) == want_risk[-1] and rc.risk_at_coverage(1e-9) == want_risk[0]
    k = len(want_cov) // 2
    assert rc.risk_at_coverage(want_cov[k]) == want_risk[k] and rc.risk_at_coverage(want_cov[k] + 1e-9) == want_risk[k + 1]
    assert rc.coverage_at_risk(1.0) == 1.0 and rc.coverage_at_risk(-1.0) == 0.0
    assert rc.coverage_at_risk(want_risk[k]) >= want_cov[k]
    with pytest.raises(ValueError, match="coverage"):
        rc.risk_at_coverage(0.0)
