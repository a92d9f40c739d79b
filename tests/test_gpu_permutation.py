"""-m gpu: the permutation-importance kernels (csrc/permute.hip) against their numpy restatement (tests/permutation_oracle.py, held
to sklearn by tests/test_cpu_permutation.py), and mmskin.permutation.MetadataPermutationImportance end to end on the HIP model
against the restatement run on the same model's logits, taken row by row through the encode-once route."""
import functools
import os

import numpy as np
import pytest
import torch

import permutation_oracle as po
import sweep_oracle as so
from gpu_util import DEV
from helpers import SMALL
from mmskin import ops
from mmskin._lib import MMSkinError
from mmskin.permutation import MetadataPermutationImportance
from models import multimodalIntraInterModal as M
from oracle.detinit import det_init_, det_inputs
from oracle.model import OracleMultimodalModel

pytestmark = pytest.mark.gpu

SENTINEL = -77.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# --------------------------------------------------------------------------------------------------------- indices
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("G", [1, 7])
def test_indices_kernel_equals_the_restatement(G, R):
    for S in (1, 2, 63, 64, 65, 257):
        got = ops.permutation_indices(12345, R, G, S, DEV).cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, po.indices(12345, R, G, S)), S
        if S == 1:
            assert not got.any()                                           # the identity
    again = ops.permutation_indices(12345, R, G, 257, DEV).cpu().numpy()
    assert np.array_equal(again, got)
    assert not np.array_equal(ops.permutation_indices(12346, R, G, 257, DEV).cpu().numpy(), got)


def test_indices_kernel_at_the_limit_and_one_above():
    S = ops.PERMUTATION_MAX_SAMPLES
    assert S == po.MAX_SAMPLES
    got = ops.permutation_indices(1, 1, 2, S, DEV).cpu().numpy()
    assert np.array_equal(got, po.indices(1, 1, 2, S))
    with pytest.raises(MMSkinError, match=f"at most {S}"):
        ops.permutation_indices(1, 1, 2, S + 1, DEV)


# --------------------------------------------------------------------------------------------------------- rows
@pytest.mark.parametrize("width,blocks", [(20, [3, 3, 2, 4, 3, 5]), (21, [3, 3, 2, 4, 3, 5, 1]), (85, [7] * 11 + [3])])
def test_rows_kernel_is_bit_equal_and_ignores_the_cuts(width, blocks):
    """20: the 16-byte path; 21: the element path; 85: PAD-20's width (element path, 5 columns in no group)"""
    R, S = 2, 37
    G = len(blocks)
    x, group = po.onehot_case(S, blocks, seed=width, pad_to=width)
    x[:, sum(blocks):] = np.random.default_rng(width).normal(0, 1, (S, width - sum(blocks)))      # ungrouped columns stay the sample's own
    perm = po.indices(5, R, G, S)
    want = po.rows(x, group, perm)
    N = R * G * S
    buf = torch.full((N + 2, width), SENTINEL, device=DEV)                 # one guard row on either side of the output
    got = ops.permuted_rows(dev(x), dev(group), dev(perm), out=buf[1:N + 1])
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all(), "bytes outside the rows were written"
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(want, np.tile(x, (R * G, 1)))                # something was shuffled
    # ranges cut at odd offsets: each writes its rows and nothing else, and together they are the whole study
    buf = torch.full((N + 2, width), SENTINEL, device=DEV)
    edges = [0, 1, S + 3, 5 * S - 1, N]
    for r0, r1 in reversed(list(zip(edges[:-1], edges[1:]))):
        ops.permuted_rows(dev(x), dev(group), dev(perm), row0=r0, row1=r1, out=buf[1 + r0:1 + r1])
        torch.cuda.synchronize()
        assert bool((buf[:1 + r0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())
    assert np.array_equal(buf[1:N + 1].cpu().numpy().view(np.uint32), want.view(np.uint32))
    # a strided x (rows of a wider buffer) gives the same bytes
    wide = torch.zeros((S, width + 4), device=DEV)
    wide[:, :width] = dev(x)
    assert torch.equal(ops.permuted_rows(wide[:, :width], dev(group), dev(perm)), got)


# --------------------------------------------------------------------------------------------------------- scores, finalize
@pytest.mark.parametrize("K", [2, 6])
@pytest.mark.parametrize("S", [5, 65, 300])
def test_scores_and_finalize_kernels(S, K):
    """tied scores, two equal top logits, the last class absent and a label outside [0, K) in every cell (po.scores_case);
    S = 300 takes two tiles of staged rows at K = 6 ... 64 and more than one row per thread"""
    R, G = 3, 2
    logits, labels = po.scores_case(R, G, S, K, seed=10 * S + K)
    cube = logits.reshape(R, G, S, K)
    want_conf = np.zeros((R, G, K, K), dtype=np.int32)
    want_counts = np.zeros((R, G, 3 * K + 1), dtype=np.int64)
    cells = np.zeros((R, G, 3))
    for r in range(R):
        for g in range(G):
            want_conf[r, g], want_counts[r, g] = po.cell_counts(cube[r, g], labels)
            cells[r, g] = po.metrics(want_conf[r, g], want_counts[r, g])
    ranked = K > 2                          # two classes with one absent: no class has both kinds of row, the AUC is NaN
    assert (want_counts[..., K - 1] == 0).all() and bool(want_counts[..., 2 * K:3 * K].any()) == ranked
    baseline = np.array([0.75, 0.5, 0.625])
    want = po.finalize(cells, baseline)

    def run(cuts):
        confusion, counts = ops.permutation_accumulators(R, G, K, DEV)
        confusion.fill_(-5), counts.fill_(-5)
        edges = [0, *cuts, R * G * S]
        for r0, r1 in zip(edges[:-1], edges[1:]):
            ops.permutation_scores(dev(logits[r0:r1]), dev(labels), confusion, counts, r0)
        out = ops.permutation_finalize(confusion, counts, dev(baseline))
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (confusion, counts, *out)]

    confusion, counts, metrics, importances, mean, std = run([])
    assert np.array_equal(confusion, want_conf) and np.array_equal(counts, want_counts)
    err = {k: float(np.nanmax(np.abs(g - want[k]))) for k, g in (("metrics", metrics), ("importances", importances), ("mean", mean), ("std", std))}
    print(f"S {S} K {K}: kernels against the fp64 restatement {err}")
    for k, g in (("metrics", metrics), ("importances", importances), ("mean", mean), ("std", std)):
        assert np.array_equal(np.isnan(g), np.isnan(want[k])) and err[k] <= 1e-12, k
    assert not np.isnan(metrics[:2]).any() and bool(np.isnan(metrics[2]).any()) == (not ranked)
    for again in (run([]), run([S, 4 * S])):                               # bitwise repeatable, whatever the cuts at whole cells
        for a, b in zip(again, (confusion, counts, metrics, importances, mean, std)):
            assert a.tobytes() == b.tobytes()                               # bytes: the AUC of a two-class cell is NaN


def test_a_cut_inside_a_cell_returns_the_status_and_launches_nothing():
    R, G, S, K = 2, 2, 9, 6
    logits, labels = po.scores_case(R, G, S, K, seed=1)
    confusion, counts = ops.permutation_accumulators(R, G, K, DEV)
    confusion.fill_(-5), counts.fill_(-5)
    for r0, n in ((0, S + 1), (1, S), (S, 2 * S - 1)):
        with pytest.raises(MMSkinError, match="split a cell"):
            ops.permutation_scores(dev(logits[:n]), dev(labels), confusion, counts, r0)
    with pytest.raises(MMSkinError, match="not a range"):
        ops.permutation_scores(dev(logits[:2 * S]), dev(labels), confusion, counts, 3 * S)
    torch.cuda.synchronize()
    assert bool((confusion == -5).all()) and bool((counts == -5).all())


# --------------------------------------------------------------------------------------------------------- end to end
E2E_MECHS = ["concatenation", "crossattention", "gfcam", "metablock"]
E2E_S, E2E_R, E2E_SEED = 65, 2, 3
E2E_BLOCKS = [3, 3, 2, 4, 3, 5]                                            # 20 one-hot columns, six groups


def oracle_model(mech):
    return det_init_(OracleMultimodalModel(**dict(SMALL, attention_mecanism=mech)), salt=so.E2E_SALT).eval()


def hip_model(mech):
    os.environ["MMSKIN_BACKBONE_DTYPE"] = "fp32"
    hip = M.MultimodalModel(**dict(SMALL, attention_mecanism=mech, device=DEV))
    hip.load_state_dict(oracle_model(mech).state_dict(), strict=True)
    return hip.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def e2e_fold():
    img = det_inputs(E2E_S, 32, 20, 6)[0]
    x, group = po.onehot_case(E2E_S, E2E_BLOCKS, seed=9)
    perm = po.indices(E2E_SEED, E2E_R, len(E2E_BLOCKS), E2E_S)
    return img, x, group, perm, po.rows(x, group, perm)


@functools.lru_cache(maxsize=None)
def e2e_cpu(mech):
    """The torch loop on the CPU oracle model, one batch-1 forward per row of the fold and of the study, in fp32 and in fp64, the
    labels (the fp64 model's own predictions, three in ten replaced, class 5 absent) and the two studies.  Computed once per fusion."""
    img, x, group, perm, rows = e2e_fold()
    out = {}
    for name, dtype in (("fp32", torch.float32), ("fp64", torch.float64)):
        model = oracle_model(mech).to(dtype)
        with torch.no_grad():
            loop = lambda metas: torch.cat([model(img[n % E2E_S:n % E2E_S + 1].to(dtype), torch.from_numpy(metas[n:n + 1]).to(dtype))
                                            for n in range(len(metas))]).numpy()
            out[name] = (loop(x), loop(rows))
    rng = np.random.default_rng(1)
    labels = out["fp64"][0].argmax(axis=1)
    labels = np.where(rng.random(E2E_S) < 0.3, rng.integers(0, 5, E2E_S), labels)
    labels[labels == 5] = 0
    studies = {name: po.study(base.astype(np.float32), cube.astype(np.float32).reshape(E2E_R, -1, E2E_S, 6), labels)
               for name, (base, cube) in out.items()}
    return labels.astype(np.int64), studies


def study_distance(a, b):
    return max(float(np.abs(a[k] - b[k]).max()) for k in ("importances", "mean", "std", "baseline"))


@pytest.mark.parametrize("mech", E2E_MECHS)
def test_permutation_importance_end_to_end(mech):
    """custom-cnn on 32 x 32 images, S = 65, C = 6, 20 one-hot columns in six groups, R = 2.  .fit against the restatement run on
    the HIP model's own logits, taken one row at a time through encode_image / fuse.  The bound is four times the distance between
    the torch fp32 loop and the fp64 loop on the CPU oracle model on these inputs (printed; DESIGN.md section 20 records it)."""
    labels, studies = e2e_cpu(mech)
    measured = study_distance(studies["fp32"], studies["fp64"])
    bound = 4.0 * measured
    img, x, group, perm, rows = e2e_fold()
    hip = hip_model(mech)
    with torch.no_grad():
        feat = hip.encode_image(img.to(DEV))
        loop = lambda metas: torch.cat([hip.fuse(feat[n % E2E_S:n % E2E_S + 1], dev(metas[n:n + 1])) for n in range(len(metas))]).float().cpu().numpy()
        want = po.study(loop(x), loop(rows).reshape(E2E_R, -1, E2E_S, 6), labels)
    calls = []
    encode = hip.encode_image
    hip.encode_image = lambda image: (calls.append(tuple(image.shape)), encode(image))[1]
    results = {}
    for per_call in (E2E_S, 3 * E2E_S, E2E_R * len(E2E_BLOCKS) * E2E_S, 100):
        pi = MetadataPermutationImportance(hip, groups=group, n_repeats=E2E_R, seed=E2E_SEED, rows_per_call=per_call)
        before = len(calls)
        results[per_call] = pi.fit(img.to(DEV), x, labels)
        assert calls[before:] == [(E2E_S, 3, 32, 32)]                      # the image encoder ran once
    res = results[E2E_S]
    got = dict(importances=np.stack([res.importances[m] for m in po.METRICS]), mean=np.stack([res.importances_mean[m] for m in po.METRICS]),
               std=np.stack([res.importances_std[m] for m in po.METRICS]), baseline=np.array([res.baseline[m] for m in po.METRICS]))
    err = study_distance(got, want)
    print(f"{mech}: |fit - restatement on the HIP model's row-by-row logits| {err:.3e}; torch fp32 loop against the fp64 loop (measured) "
          f"{measured:.3e}, bound {bound:.3e}; baseline {res.baseline}; largest |importance| {np.abs(want['importances']).max():.3e}")
    assert res.importances["auc"].shape == (len(E2E_BLOCKS), E2E_R) and res.group_names == [f"group{g}" for g in range(len(E2E_BLOCKS))]
    assert np.abs(want["importances"]).max() > 0.01                        # the head reacts to the metadata: there is something to get wrong
    assert err <= bound
    # rows_per_call of S, 3 S, the whole cube and 100 (rounded down to S): bitwise equal; the same seed again: bitwise equal
    again = MetadataPermutationImportance(hip, groups=group, n_repeats=E2E_R, seed=E2E_SEED, rows_per_call=E2E_S).fit(img.to(DEV), x, labels)
    for other in (*results.values(), again):
        for m in po.METRICS:
            assert np.array_equal(other.importances[m], res.importances[m]) and np.array_equal(other.importances_std[m], res.importances_std[m])
            assert np.array_equal(other.metrics[m], res.metrics[m]) and other.baseline[m] == res.baseline[m]
    # images in batches of 32: each encoded once
    before = len(calls)
    MetadataPermutationImportance(hip, groups=group, n_repeats=1, seed=E2E_SEED, image_batch_size=32).fit(img.to(DEV), x, labels)
    assert calls[before:] == [(32, 3, 32, 32), (32, 3, 32, 32), (1, 3, 32, 32)]


def test_fit_refuses_train_mode_on_the_device():
    img, x, group, perm, rows = e2e_fold()
    hip = hip_model("gfcam")
    hip.train()
    with pytest.raises(MMSkinError, match="eval"):
        MetadataPermutationImportance(hip, groups=group, n_repeats=1).fit(img.to(DEV), x, np.zeros(E2E_S, dtype=np.int64))
