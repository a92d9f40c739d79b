"""Permutation importance of the metadata without a GPU: tests/permutation_oracle.py (the numpy restatement the kernels are held
to by tests/test_gpu_permutation.py) against outside knowledge -- sklearn's permutation_importance and roc_auc_score --, three
deliberate corruptions of it that these comparisons must reject, and the host logic of mmskin.permutation and of the C entry
points (the refusals need no device)."""
import ctypes
import os

import numpy as np
import pytest
import torch
from sklearn.base import BaseEstimator
from sklearn.inspection import _permutation_importance as skpi
from sklearn.inspection import permutation_importance
from sklearn.metrics import roc_auc_score

import permutation_oracle as po
from helpers import SMALL
from mmskin import _lib
from mmskin._lib import MMSkinError
from mmskin.permutation import MetadataPermutationImportance
from models import multimodalIntraInterModal as M

S, W, K, R = 97, 9, 4, 5


class FixedMLP(BaseEstimator):
    """sklearn estimator whose predict_proba is a fixed numpy MLP over the encoded columns; column IGNORED gets zero weights"""
    IGNORED = 4

    def __init__(self):
        rng = np.random.default_rng(5)
        self.w1, self.w2 = rng.normal(0, 1.5, (W, 16)), rng.normal(0, 1.5, (16, K))
        self.w1[self.IGNORED] = 0.0
        self.classes_ = np.arange(K)

    def fit(self, X, y):
        return self

    def logits(self, X):
        return (np.tanh(np.asarray(X, dtype=np.float64) @ self.w1) @ self.w2).astype(np.float32)

    def predict_proba(self, X):
        return po.softmax32(self.logits(X)).astype(np.float64)

    def predict(self, X):
        return self.logits(X).argmax(axis=1)


def fold():
    rng = np.random.default_rng(11)
    x = rng.normal(0, 1, (S, W)).astype(np.float32)
    x[:, 2] = rng.integers(0, 2, S)                                        # a binary column: its shuffles produce tied scores
    labels = FixedMLP().predict(x)
    flip = rng.random(S) < 0.3
    labels[flip] = rng.integers(0, K, int(flip.sum()))
    return x, labels.astype(np.int64)


def oracle_study(x, labels, perm, group, **knobs):
    est = FixedMLP()
    row_knobs = {k: knobs.pop(k) for k in ("shift_group",) if k in knobs}
    Rn, G, Sn = perm.shape
    cube = est.logits(po.rows(x, group, perm, **row_knobs)).reshape(Rn, G, Sn, K)
    return po.study(est.logits(x), cube, labels, **knobs)


class TableRandomState:
    """stands in for the RandomState that sklearn builds per column: shuffle() leaves in the index array whatever brings the
    column, which sklearn shuffles cumulatively, to x[table[r, column]]"""

    def __init__(self, table, column):
        self.table, self.column, self.repeat = table, column, 0
        self.current = np.arange(table.shape[2])

    def randint(self, *a, **k):
        return 0

    def shuffle(self, idx):
        want = self.table[self.repeat, self.column]
        where = np.empty_like(self.current)
        where[self.current] = np.arange(len(self.current))                 # where[v] = the position that now holds sample v's value
        idx[:] = where[want]
        self.current, self.repeat = want.copy(), self.repeat + 1


def sklearn_importances(x, labels, perm, scoring, monkeypatch):
    made = []

    def fake_check_random_state(seed):
        made.append(TableRandomState(perm, len(made) - 1))                 # the first one is permutation_importance's own
        return made[-1]

    monkeypatch.setattr(skpi, "check_random_state", fake_check_random_state)
    out = permutation_importance(FixedMLP(), x.astype(np.float64), labels, scoring=scoring, n_repeats=perm.shape[0], n_jobs=1)
    assert len(made) == 1 + x.shape[1] and all(rs.repeat == perm.shape[0] for rs in made[1:])
    return out


# ------------------------------------------------------------------------------------------- against sklearn
def test_importances_equal_sklearn_with_the_same_table(monkeypatch):
    x, labels = fold()
    perm = po.indices(3, R, W, S)
    group = np.arange(W)
    got = oracle_study(x, labels, perm, group)
    for k, scoring in ((0, "accuracy"), (1, "balanced_accuracy")):
        ref = sklearn_importances(x, labels, perm, scoring, monkeypatch)
        err = max(np.abs(got["importances"][k] - ref.importances).max(), np.abs(got["mean"][k] - ref.importances_mean).max(),
                  np.abs(got["std"][k] - ref.importances_std).max())
        print(f"{scoring}: oracle against sklearn {err:.3e}, largest importance {np.abs(ref.importances).max():.3e}")
        assert np.abs(ref.importances).max() > 0.05 and err <= 1e-12
    # a group the network ignores: shuffling it changes no logit, the importance is exactly 0 in every metric and repeat
    assert not got["importances"][:, FixedMLP.IGNORED].any() and not got["std"][:, FixedMLP.IGNORED].any()
    assert np.abs(got["importances"][:, :FixedMLP.IGNORED]).max() > 0


def test_auc_equals_sklearn_macro_ovr_with_ties():
    rng = np.random.default_rng(2)
    labels = rng.integers(0, K, S)
    probs = po.softmax32(rng.normal(0, 1, (S, K))).astype(np.float64)
    probs[S // 2:] = probs[:S - S // 2]                                    # every score occurs twice, under independent labels
    assert len(np.unique(probs[:, 0])) <= S // 2 + 1
    confusion, counts = po.cell_counts(np.log(probs).astype(np.float32), labels, probs=probs)
    got = po.metrics(confusion, counts)[2]
    want = roc_auc_score(labels, probs / probs.sum(axis=1, keepdims=True), multi_class="ovr", average="macro")
    print(f"macro one-vs-rest AUC: oracle {got:.15f}, sklearn {want:.15f}")
    assert abs(got - want) <= 1e-12
    # a class absent from the fold: NaN for that class, the mean over the others (the rule of evaluate.auc_from_counts)
    labels3 = np.where(labels == K - 1, 0, labels)
    confusion, counts = po.cell_counts(np.log(probs).astype(np.float32), labels3, probs=probs)
    auc = po.per_class_auc(counts)
    assert np.isnan(auc[K - 1]) and not np.isnan(auc[:K - 1]).any()
    per_class = [roc_auc_score(labels3 == c, probs[:, c]) for c in range(K - 1)]
    assert abs(po.metrics(confusion, counts)[2] - np.mean(per_class)) <= 1e-12
    counts[3 * K] = 1                                                      # a NaN probability: no AUC
    assert np.isnan(po.metrics(confusion, counts)[2])


# ------------------------------------------------------------------------------------------- the generator
def test_permutations_are_permutations_differ_and_ignore_chunking():
    for Sn in (1, 2, 63, 64, 65, 257, 1000):
        perm = po.indices(7, 3, 4, Sn)
        assert perm.dtype == np.int32 and np.array_equal(np.sort(perm, axis=-1), np.broadcast_to(np.arange(Sn), perm.shape))
        for chunk in (1, 7, 64, Sn + 3):
            assert np.array_equal(po.indices(7, 3, 4, Sn, chunk=chunk), perm)
        if Sn >= 63:
            flat = perm.reshape(-1, Sn)
            assert len({row.tobytes() for row in flat}) == len(flat)       # every (r, g) its own shuffle
            assert not np.array_equal(po.indices(8, 3, 4, Sn), perm)
            assert (flat != np.arange(Sn)).mean() > 0.9
    assert po.indices(0, 2, 2, 1).tolist() == [[[0], [0]], [[0], [0]]]
    # the finaliser itself: splitmix64's first output for state 0 (Vigna's reference implementation)
    assert int(po.mix64(np.uint64(0))) == 0xE220A8397B1DCDAF


# ------------------------------------------------------------------------------------------- corruptions are caught
def test_three_corruptions_of_the_oracle_are_rejected(monkeypatch):
    x, labels = fold()
    perm = po.indices(3, R, W, S)
    group = np.arange(W)
    ref = sklearn_importances(x, labels, perm, "balanced_accuracy", monkeypatch)
    good = oracle_study(x, labels, perm, group)
    assert np.abs(good["importances"][1] - ref.importances).max() <= 1e-12
    wrong_group = oracle_study(x, labels, perm, group, shift_group=1)
    assert np.abs(wrong_group["importances"][1] - ref.importances).max() > 1e-3
    ddof1 = oracle_study(x, labels, perm, group, ddof=1)
    assert np.abs(ddof1["std"][1] - ref.importances_std).max() > 1e-4 and np.abs(good["std"][1] - ref.importances_std).max() <= 1e-12
    rng = np.random.default_rng(4)
    y3 = rng.integers(0, K - 1, S)                                         # class K - 1 absent
    logits = rng.normal(0, 1, (S, K)).astype(np.float32)
    probs = po.softmax32(logits).astype(np.float64)
    want = np.mean([roc_auc_score(y3 == c, probs[:, c]) for c in range(K - 1)])
    confusion, counts = po.cell_counts(logits, y3)
    assert abs(po.metrics(confusion, counts)[2] - want) <= 1e-12
    assert abs(po.metrics(confusion, counts, count_absent=True)[2] - want) > 0.05


# ------------------------------------------------------------------------------------------- host logic
def test_groups_from_the_encoder_the_map_and_the_dict():
    import sweep_oracle as so
    enc = so.e2e_encoder()                                                 # blocks 3 3 2 4 3 + 3 numerics = 18 of 20 columns
    gmap, names = MetadataPermutationImportance.resolve_groups(20, enc, None)
    assert gmap.tolist() == [0] * 3 + [1] * 3 + [2] * 2 + [3] * 4 + [4] * 3 + [5, 6, 7] + [-1, -1]
    assert names == ["cat0", "cat1", "cat2", "cat3", "cat4", "num0", "num1", "num2"]
    gmap, names = MetadataPermutationImportance.resolve_groups(5, None, None)
    assert gmap.tolist() == [0, 1, 2, 3, 4] and names[4] == "col4"
    gmap, names = MetadataPermutationImportance.resolve_groups(5, None, {"a": [3, 0], "b": [1]})
    assert gmap.tolist() == [0, 1, -1, 0, -1] and names == ["a", "b"]
    gmap, names = MetadataPermutationImportance.resolve_groups(3, None, [1, -1, 0], group_names=["x", "y"])
    assert gmap.dtype == np.int32 and names == ["x", "y"]
    for bad in ([0, 2, 2], [0, 1], [-2, 0, 1], {"a": [0], "b": [0]}, {"a": [5]}):
        with pytest.raises(ValueError):
            MetadataPermutationImportance.resolve_groups(3, None, bad)
    with pytest.raises(ValueError, match="vocab_size"):
        MetadataPermutationImportance.resolve_groups(10, enc, None)


def test_fit_refuses_train_mode_text_encoders_and_blind_fusions():
    img, meta, lab = torch.zeros(3, 3, 32, 32), torch.zeros(3, 20), torch.zeros(3, dtype=torch.int64)
    model = M.MultimodalModel(**dict(SMALL, attention_mecanism="concatenation"))
    with pytest.raises(MMSkinError, match="eval"):
        MetadataPermutationImportance(model.train()).fit(img, meta, lab)
    model.eval()
    with pytest.raises(ValueError, match="encoded rows"):
        MetadataPermutationImportance(model).fit(img, meta[:, :19], lab)
    with pytest.raises(ValueError, match="integer labels"):
        MetadataPermutationImportance(model).fit(img, meta, lab.float())
    model.text_model_name = "bert-base-uncased"
    with pytest.raises(ValueError, match="one-hot"):
        MetadataPermutationImportance(model).fit(img, meta, lab)
    blind = M.MultimodalModel(**dict(SMALL, attention_mecanism="no-metadata")).eval()
    with pytest.raises(ValueError, match="nothing to explain"):
        MetadataPermutationImportance(blind).fit(img, meta, lab)
    with pytest.raises(ValueError, match="n_repeats"):
        MetadataPermutationImportance(model, n_repeats=0)


def test_entry_points_refuse_bad_arguments_without_a_device():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmmskin_hip.so is not built")
    lib = _lib.load()
    buf = (ctypes.c_int64 * 64)()                                          # never touched: every call fails its checks first
    p = ctypes.cast(buf, ctypes.c_void_p)

    def refused(rc, word, code=1):
        assert rc == code and word in lib.mmskin_last_error().decode(), (rc, lib.mmskin_last_error())

    limit = 4096
    refused(lib.mmskin_permutation_indices(0, 1, 1, limit + 1, p, None), f"at most {limit}")
    refused(lib.mmskin_permutation_indices(0, 0, 1, 5, p, None), "extent")
    refused(lib.mmskin_permutation_indices(0, 1, 1, 5, None, None), "null")
    refused(lib.mmskin_permuted_rows(p, 4, p, p, 2, 3, 5, 4, 0, 31, p, None), "not a range")
    refused(lib.mmskin_permuted_rows(p, 3, p, p, 2, 3, 5, 4, 0, 30, p, None), "stride")
    refused(lib.mmskin_permutation_scores(p, p, 2, 3, 5, 6, 0, 7, p, p, None), "split a cell")
    refused(lib.mmskin_permutation_scores(p, p, 2, 3, 5, 6, 3, 10, p, p, None), "split a cell")
    refused(lib.mmskin_permutation_scores(p, p, 2, 3, 5, 65, 0, 10, p, p, None), "classes", code=3)
    refused(lib.mmskin_permutation_scores(p, p, 2, 3, limit + 1, 6, 0, limit + 1, p, p, None), f"at most {limit}")
    refused(lib.mmskin_permutation_finalize(p, p, None, 2, 3, 6, p, p, p, p, None), "null")
    assert not any(buf)
