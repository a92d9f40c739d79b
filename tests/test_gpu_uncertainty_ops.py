"""-m gpu: the three kernels of csrc/uncertainty.hip against tests/uncertainty_oracle.py (held to closed forms by
tests/test_cpu_uncertainty.py): the views bit for bit against torch.rot90 / torch.flip, the reduction exactly in its integers and
within uncertainty_oracle.TOL in fp64, the risk-coverage counts exactly and their summary within the same tolerance."""
import numpy as np
import pytest
import torch

import uncertainty_oracle as uo
from gpu_util import DEV
from mmskin import evaluate, ops
from mmskin._lib import MMSkinError

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------------------------------------------- views
def torch_views(x, mask):
    out = []
    for v in ops.view_ids(mask):
        y = torch.rot90(x, v & 3, (2, 3))
        out.append(torch.flip(y, (3,)) if v & 4 else y)
    return torch.stack(out)


def drawn_images(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    return torch.randn(shape, generator=g).to(dtype)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.bfloat16, torch.float32], ids=["1B", "2B", "4B"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 5), (1, 3, 33, 33), (2, 3, 64, 64), (1, 3, 65, 65)])
def test_views_equal_torch_bit_for_bit(shape, dtype):
    x = drawn_images(shape, dtype, seed=sum(shape)).to(DEV)
    for mask in (0xFF, 0xA5, 0x08):
        V = len(ops.view_ids(mask))
        guard = torch.full((V + 2, *shape), 7, dtype=dtype, device=DEV)          # one guard slab on either side of the output
        got = ops.dihedral_views(x, mask, out=guard[1:V + 1])
        torch.cuda.synchronize()
        assert got.dtype == dtype and torch.equal(got, torch_views(x, mask)), hex(mask)
        assert bool((guard[0] == 7).all()) and bool((guard[-1] == 7).all()), "bytes outside the V slabs were written"
    assert np.array_equal(ops.dihedral_views(x, 0xFF).float().cpu().numpy(), uo.views(x.float().cpu().numpy(), 0xFF))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.bfloat16, torch.float32], ids=["1B", "2B", "4B"])
def test_flips_of_a_non_square_batch_and_the_refusals(dtype):
    x = drawn_images((1, 2, 7, 9), dtype, seed=3).to(DEV)
    for mask in (ops.VIEWS_FLIPS, 0x44, 0x01):
        assert torch.equal(ops.dihedral_views(x, mask), torch_views(x, mask)), hex(mask)
    wide = drawn_images((2, 1, 3, 70), dtype, seed=4).to(DEV)                     # more than one tile along W only
    assert torch.equal(ops.dihedral_views(wide, ops.VIEWS_FLIPS), torch_views(wide, ops.VIEWS_FLIPS))
    out = torch.full((8, 1, 2, 7, 9), 7, dtype=dtype, device=DEV)
    for mask, word in ((0xFF, "H == W"), (0x02, "H == W"), (0, "view_mask")):
        with pytest.raises(MMSkinError, match=word):
            ops.dihedral_views(x, mask, out=out[:len(ops.view_ids(mask))])
    torch.cuda.synchronize()
    assert bool((out == 7).all())


# --------------------------------------------------------------------------------------------------------------- reduce
def run_reduce(logits):
    got = ops.uncertainty_reduce(logits)
    torch.cuda.synchronize()
    return dict(zip(("mean_prob", "prob_std", "votes", "pred", "stats"), (t.cpu().numpy() for t in got)))


def check_reduce(got, want, what):
    assert got["pred"].dtype == np.int32 and np.array_equal(got["pred"], want["pred"]), what
    assert got["votes"].dtype == np.int32 and np.array_equal(got["votes"], want["votes"]), what
    assert np.array_equal(got["stats"][:, 5], want["stats"][:, 5], equal_nan=True), what          # the variation ratio: exact
    for key in ("mean_prob", "prob_std", "stats"):
        assert np.array_equal(np.isnan(got[key]), np.isnan(want[key])), (what, key)
        print(f"{what} {key}: max |got - want| / max(|want|, 1) = {uo.worst(got[key], want[key]):.3e}")
    for key in ("mean_prob", "prob_std", "stats"):
        assert uo.close(got[key], want[key]), (what, key, uo.worst(got[key], want[key]))


@pytest.mark.parametrize("T,N,C", uo.REDUCE_SHAPES)
def test_reduce_kernel_matches_the_restatement(T, N, C):
    """planted in every case (uncertainty_oracle.reduce_case): rows of +-80 and of 1e4, an all-equal row, a row with two exactly
    equal maxima, a row with an inf"""
    z = uo.reduce_case(T, N, C)
    want = uo.reduce(z)
    dev = torch.from_numpy(z).to(DEV)
    got = run_reduce(dev)
    check_reduce(got, want, f"T {T} N {N} C {C}")
    if N > 4:
        assert got["pred"][4] == -1 and np.isnan(got["stats"][4]).all() and got["pred"][3] == C // 2
    again = run_reduce(dev)                                                        # a second call equals the first
    for key in got:
        assert np.array_equal(got[key], again[key], equal_nan=True), key
    # a strided view: the passes 2 N C apart and the rows 2 C apart inside a block of sentinels
    block = torch.full((T, 2, N, 2, C), float("nan"), device=DEV)
    block[:, 0, :, 0] = dev
    view = block[:, 0, :, 0]
    assert view.stride() == (4 * N * C, 2 * C, 1)
    strided = run_reduce(view)
    for key in got:
        assert np.array_equal(got[key], strided[key], equal_nan=True), key


def test_reduce_rows_do_not_depend_on_their_neighbours():
    z = torch.from_numpy(uo.reduce_case(33, 64, 6)).to(DEV)
    full = run_reduce(z)
    part = run_reduce(z[:, 10:21])                                                 # rows 10 .. 20 alone, read in place
    for key in full:
        assert np.array_equal(part[key], full[key][10:21], equal_nan=True), key
    assert np.isfinite(part["stats"]).all()


def test_reduce_refusals_launch_nothing():
    for shape, word in (((2, 4, 65), "MAX_CLASSES"), ((2, 4, 1), "MAX_CLASSES"), ((4097, 1, 2), "MAX_PASSES")):
        with pytest.raises(MMSkinError, match=word):
            ops.uncertainty_reduce(torch.zeros(shape, device=DEV))
    with pytest.raises(ValueError, match="contiguous"):
        ops.uncertainty_reduce(torch.zeros((2, 4, 12), device=DEV)[:, :, ::2])


# --------------------------------------------------------------------------------------------------------------- risk-coverage
@pytest.mark.parametrize("N", uo.RISK_SIZES)
def test_risk_coverage_kernels_match_the_restatement(N):
    for scores in uo.RISK_SCORES:
        for wrong in uo.RISK_WRONG:
            s, w = uo.risk_case(N, scores, wrong)
            want_counts = uo.risk_counts(s, w)
            want = uo.risk_summary(want_counts, w)
            ds, dw = torch.from_numpy(s).to(DEV), torch.from_numpy(w).to(DEV)
            counts = ops.risk_coverage(ds, dw)
            summary = ops.risk_coverage_summary(counts, dw)
            torch.cuda.synchronize()
            what = f"N {N} {scores} {wrong}"
            assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), want_counts), what
            got = summary.cpu().numpy()
            print(f"{what}: aurc {got[0]:.6f} optimal {got[1]:.6f} auroc {got[3]:.6f}, worst error {uo.worst(got, want):.3e}")
            assert uo.close(got, want), (what, got, want)
            assert np.isnan(got[3]) == (w.sum() in (0, N)) and np.array_equal(got[5:], want[5:])
            again = ops.risk_coverage_summary(counts, dw)                        # a second call: the same bits (a NaN is no == NaN)
            assert torch.equal(ops.risk_coverage(ds, dw), counts) and torch.equal(again.view(torch.int64), summary.view(torch.int64))
            if scores == "eighths" and wrong == "drawn":
                # the same AUROC from the fold evaluation's kernel: class 1 of the two-column probabilities [1 - s, s], the wrong flag
                # as the label (k / 8 is exact in fp32)
                probs = torch.stack([1.0 - ds, ds], dim=1).float().contiguous()
                auc = evaluate.per_class_auc(evaluate.ovr_auc_counts(probs, dw.long()))[1]
                assert np.array_equal(auc, got[3], equal_nan=True), (what, auc, got[3])


def test_risk_coverage_refusals_launch_nothing():
    big = ops.BOOTSTRAP_MAX_ROWS + 1
    with pytest.raises(MMSkinError, match="BOOTSTRAP_MAX_ROWS"):
        ops.risk_coverage(torch.zeros(big, dtype=torch.float64, device=DEV), torch.zeros(big, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="score"):
        ops.risk_coverage(torch.zeros(5, device=DEV), torch.zeros(5, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="wrong"):
        ops.risk_coverage(torch.zeros(5, dtype=torch.float64, device=DEV), torch.zeros(5, dtype=torch.int32, device=DEV))
