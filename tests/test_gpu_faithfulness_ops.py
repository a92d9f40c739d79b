"""-m gpu: the faithfulness kernels (csrc/faithfulness.hip) against their numpy restatement (tests/faithfulness_oracle.py, held
to independent forms of the definitions by tests/test_cpu_faithfulness.py): rank, blur, mean and perturb bit for bit, curves
within 1e-12 (fp64 exp implementations differ in the last few ulps and every output lies in [0, 1])."""
import numpy as np
import pytest
import torch

import faithfulness_oracle as fo
from gpu_util import DEV
from mmskin import ops

pytestmark = pytest.mark.gpu

SENTINEL = -77.0


def equal_bits(got, want):
    """same values element for element (a -0.0 equals 0.0: no bit pattern is compared for zero)"""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def saliency_maps(N, H, W):
    """name -> [N, H, W] fp32: random; all equal; a ReLU'd map with >= 80 % zeros; one with +-0.0, +-inf and a few NaNs"""
    rng = np.random.default_rng(H * 1000 + W * 10 + N)
    relu = np.maximum(rng.standard_normal((N, H, W)) - 1.3, 0).astype(np.float32)          # P(z > 1.3) = 10 %
    assert H * W < 1000 or (relu == 0).mean() >= 0.8
    special = rng.standard_normal((N, H * W)).astype(np.float32)
    values = [0.0, -0.0, np.inf, -np.inf, np.nan, np.nan, 0.0, -0.0, np.inf, np.nan, 2.5, 2.5]
    for n in range(N):
        for i, v in zip(rng.permutation(H * W), values):
            special[n, i] = v
    return {"random": rng.standard_normal((N, H, W)).astype(np.float32), "equal": np.full((N, H, W), 0.5, np.float32), "relu": relu,
            "special": special.reshape(N, H, W)}


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 3), (37, 29), (64, 64)])
def test_rank_matches_the_restatement(H, W, N):
    """37x29 is no multiple of 4 and more than one workgroup; 64x64 spans two LDS tiles of keys"""
    for name, s in saliency_maps(N, H, W).items():
        buf = torch.full((N + 2, H, W), -7, device=DEV, dtype=torch.int32)         # one guard row on either side of the output
        sd = torch.from_numpy(s).to(DEV)
        first = ops.faith_rank(sd, out=buf[1:1 + N]).cpu().numpy()
        second = ops.faith_rank(sd).cpu().numpy()
        host = buf.cpu().numpy()
        assert (host[0] == -7).all() and (host[-1] == -7).all(), "ranks outside the N rows were written"
        assert equal_bits(first, fo.rank(s)), name
        assert np.array_equal(first, second), name                                 # a function of the input alone


@pytest.mark.parametrize("ksize", [3, 11])
@pytest.mark.parametrize("H,W", [(12, 12), (37, 29)])
def test_blur_and_mean_match_the_restatement(H, W, ksize):
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H + ksize))
    taps = ops.gaussian_taps(ksize, 5.0)
    assert np.array_equal(taps, fo.gaussian_taps(ksize, 5.0))
    buf = torch.full((4, 3, H, W), SENTINEL, device=DEV)
    got = ops.faith_blur(x.to(DEV), taps, out=buf[1:3]).cpu().numpy()
    assert equal_bits(got, fo.blur(x.numpy(), taps))
    host = buf.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all()
    buf.fill_(SENTINEL)
    got = ops.faith_mean(x.to(DEV), out=buf[1:3]).cpu().numpy()
    assert equal_bits(got, fo.mean_fill(x.numpy()))
    host = buf.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all()


def test_blur_widest_kernel_and_a_narrow_image():
    """ksize 31 (the cap; the halo is 15 of the 32-wide tile) and an image only 3 high with ksize 5 (the padding reflects
    across most of the axis)"""
    for ksize, H, W in [(31, 37, 70), (5, 3, 40)]:
        x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(ksize))
        taps = ops.gaussian_taps(ksize, 5.0)
        assert equal_bits(ops.faith_blur(x.to(DEV), taps).cpu().numpy(), fo.blur(x.numpy(), taps))


@pytest.mark.parametrize("H,W", [(5, 3), (37, 29), (12, 12), (64, 64)])
def test_perturb_matches_the_restatement(H, W):
    """all three modes, k in {0, 1, S}, S in {1, 7, H * W} (the entry points cap S at 1024: 37x29 and 64x64 take 1024 for the
    third), a ragged chunk with guard rows, and a row table with out-of-range entries (clamped: the nearest image, step and
    mode).  5x3 and 37x29 take the dword path, 12x12 and 64x64 the 16-byte one."""
    N, HW = 3, H * W
    rng = np.random.default_rng(HW)
    img = rng.standard_normal((N, 3, H, W)).astype(np.float32)
    base = rng.standard_normal((N, 3, H, W)).astype(np.float32)
    sal = (rng.standard_normal((N, H, W)) * 0.8).astype(np.float32)                 # values below 0 and above 1: the clamp is live
    sal[0, 0, 0] = np.nan
    ranks = fo.rank(sal)
    dev = [torch.from_numpy(a).to(DEV) for a in (img, base, ranks, sal)]
    for S in (1, 7, min(HW, ops.FAITH_MAX_STEPS)):
        table = [(n % N, k, mode) for n, k in enumerate((0, 1, S)) for mode in (fo.DELETION, fo.INSERTION, fo.EXPLANATION)]
        table += [(-1, 1, fo.DELETION), (N, S + 5, fo.INSERTION), (1, -3, fo.DELETION), (2, 1, 9), (7, 1, -2)]
        rows = np.asarray(table, dtype=np.int32)
        n, n_pad = len(rows), len(rows) + 3
        buf = torch.full((n_pad + 2, 3, H, W), SENTINEL, device=DEV)
        got = ops.faith_perturb(*dev, torch.from_numpy(rows).to(DEV), S, n, n_pad, out=buf[1:1 + n_pad]).cpu().numpy()
        host = buf.cpu().numpy()
        assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all(), "bytes outside the n_pad rows were written"
        want = fo.perturb(img, base, ranks, sal, rows, S, n, n_pad)
        assert equal_bits(got, want), S
        assert not host[1 + n:1 + n_pad].any()                                      # padded rows are exactly zero
        assert equal_bits(got[0], img[0]) and equal_bits(got[1], base[0])           # deletion / insertion at k = 0
        assert equal_bits(got[6], base[2]) and equal_bits(got[7], img[2])           # ... at k = S
    fresh = ops.faith_perturb(*dev, torch.from_numpy(rows).to(DEV), S, n, n_pad).cpu().numpy()
    assert equal_bits(fresh, want)                                                  # a fresh output buffer takes the same path


@pytest.mark.parametrize("H,W", [(7, 9), (32, 33), (36, 36)])
def test_perturb_tile_shared_with_rise_apply(H, W):
    """The pixel tile and the blend that faith_perturb shares with rise_apply (csrc/perturb_tile.h), at the shapes of
    test_gpu_rise_ops.test_apply_tile_matches_the_restatement_bit_for_bit.  The test above already holds both paths, a NaN
    saliency and the zero padding to the restatement; new here: a 16-byte path whose second tile is mostly empty (32x33: 1056
    pixels) or partly filled (36x36: 1296), a dword path of less than one tile whose pixel count is odd (7x9), an image that is
    its own baseline (every mode must return it exactly) and a NaN pixel in an image.  Two images, n = 3 rows, n_pad = 5."""
    N, S, n, n_pad = 2, 4, 3, 5
    rng = np.random.default_rng(H * W)
    img = rng.standard_normal((N, 3, H, W)).astype(np.float32)
    base = rng.standard_normal((N, 3, H, W)).astype(np.float32)
    base[1] = img[1]
    img[0, 1, H // 2, W // 3] = np.nan
    sal = (rng.standard_normal((N, H, W)) * 0.8).astype(np.float32)
    ranks = fo.rank(sal)
    rows = np.asarray([(0, 2, fo.DELETION), (0, 0, fo.EXPLANATION), (1, 0, fo.EXPLANATION), (1, 2, fo.INSERTION), (1, 2, fo.DELETION)],
                      dtype=np.int32)                                                 # the last two are past n: never built
    dev = [torch.from_numpy(a).to(DEV) for a in (img, base, ranks, sal, rows)]
    buf = torch.full((n_pad + 2, 3, H, W), SENTINEL, device=DEV)
    got = ops.faith_perturb(*dev, S, n, n_pad, out=buf[1:1 + n_pad]).cpu().numpy()
    host = buf.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all(), "bytes outside the n_pad rows were written"
    want = fo.perturb(img, base, ranks, sal, rows, S, n, n_pad)
    print(f"{H}x{W}: {int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())} of {got.size} values differ")
    assert equal_bits(got, want)
    assert not host[1 + n:1 + n_pad].any()                                          # padded rows are exactly zero
    assert np.array_equal(got[2], img[1])                                           # baseline == image: the blend returns it
    for mode in (fo.DELETION, fo.INSERTION):                                        # ... and so does the select
        rows[2, 1:] = (2, mode)
        assert np.array_equal(ops.faith_perturb(*dev[:4], torch.from_numpy(rows).to(DEV), S, n, n_pad).cpu().numpy()[2], img[1])
    assert np.isnan(got[1, 1, H // 2, W // 3]) and int(np.isnan(got[1]).sum()) == 1   # the blend keeps the NaN pixel, and only it


def first_largest(row):
    """the arg-max rule of csrc/target_prob.h: the first largest logit, where a NaN is never larger"""
    t, best = 0, row[0]
    for c in range(1, len(row)):
        if row[c] > best or (best != best and row[c] == row[c]):
            t, best = c, row[c]
    return t


@pytest.mark.parametrize("K", [1, 2, 7])
def test_target_and_clean_probability_are_the_ones_rise_uses(K):
    """faith_curves and rise_accumulate take the class and the clean probability from the same two device functions
    (csrc/target_prob.h): on the same clean logits both must return the same target and bitwise the same probability.  Rows: a
    tie for the maximum between the first and the last class, a NaN first logit, an all-NaN row, +inf and -inf, an ordinary
    row.  Faithfulness gets S = 1 with every row of an image equal to its clean row; RISE one mask on an 8x8 image with the
    masked logits equal to the clean ones.  target None and a given target out of range on both sides (clamped)."""
    import rise_oracle as ro
    N, S = 5, 1
    clean = (np.random.default_rng(K).standard_normal((N, K)) * 3).astype(np.float32)
    clean[0, 0] = clean[0, -1] = np.abs(clean[0]).max() + 1
    clean[1, 0] = np.nan
    clean[2, :] = np.nan
    clean[3, 0], clean[3, -1] = np.inf, -np.inf
    cd = torch.from_numpy(clean).to(DEV)
    rows = torch.from_numpy(np.repeat(clean, 2 * S + 3, axis=0)).to(DEV)
    for target in (None, [-3, K, K + 5, 0, 100]):
        td = None if target is None else torch.tensor(target, dtype=torch.int32, device=DEV)
        curves, _, _, used_f = ops.faith_curves(rows, S, N, td)
        _, _, clean_prob, used_r = ops.rise_accumulate(cd, cd, (8, 8), 9, 2, 0.5, 1, td)
        used = used_f.cpu().numpy()
        assert np.array_equal(used, used_r.cpu().numpy())
        assert used.tolist() == ([first_largest(r) for r in clean] if target is None else np.clip(target, 0, K - 1).tolist())
        p_f, p_r = curves[0, :, 0].cpu().numpy(), clean_prob.cpu().numpy()
        assert equal_bits(p_f, p_r)
        with np.errstate(all="ignore"):
            wants = (fo.curves(rows.cpu().numpy(), S, N, used.tolist())["deletion"][:, 0], ro.probabilities(clean, used))
        for want in wants:
            assert np.array_equal(np.isnan(p_f), np.isnan(want))
            err = float(np.nanmax(np.abs(p_f - want), initial=0.0))
            print(f"K {K} target {'given' if target else 'argmax'}: max |p - restatement| {err:.3e}")
            assert err == 0.0                    # measured: exact on these rows.  Should a later exp differ in its last ulps, the
                                                 # bound to fall back on is test_curves_match_the_restatement's 1e-12


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("C", [2, 6])
def test_curves_match_the_restatement(C, S, N):
    P = 2 * S + 3
    g = torch.Generator().manual_seed(100 * C + 10 * S + N)
    logits = torch.randn(N * P + 2, C, generator=g) * 3                             # two rows past the end: never read
    ld = logits.to(DEV)
    for target in (None, [(2 * n + 1) % C for n in range(N)]):
        td = None if target is None else torch.tensor(target, dtype=torch.int32, device=DEV)
        curves, scalars, means, used = ops.faith_curves(ld, S, N, td)
        again = ops.faith_curves(ld, S, N, td)
        want = fo.curves(logits.numpy(), S, N, target)
        assert used.cpu().numpy().tolist() == want["target"].tolist()
        got = {"deletion": curves[0], "insertion": curves[1], "deletion_auc": scalars[0], "insertion_auc": scalars[1],
               "average_drop": scalars[2], "increase": scalars[3], "mean_deletion_auc": means[0], "mean_insertion_auc": means[1],
               "mean_average_drop": means[2], "mean_increase": means[3]}
        for name, t in got.items():
            assert t.dtype == torch.float64
            err = float(np.abs(t.cpu().numpy() - want[name]).max())
            assert err <= 1e-12, (name, err)
        for a, b in zip((curves, scalars, means, used), again):
            assert torch.equal(a, b)                                                # bitwise repeatable
