"""-m gpu: the RISE kernels (csrc/rise.hip) against their numpy restatement (tests/rise_oracle.py, held to torch's bilinear
interpolate by tests/test_cpu_rise.py).  Shapes: 64x64 grid 8 (cells divide the image, the 16-byte path), 30x44 grid 4 and
17x33 grid 16 (ragged cells, more than one workgroup, the dword path for 17x33), 7x9 grid 2 (a single partial workgroup, cells
larger than half the image), 224x224 grid 7 (the working size: 196 workgroups)."""
import numpy as np
import pytest
import torch

import rise_oracle as ro
from gpu_util import DEV
from mmskin import _lib, ops
from mmskin._lib import call, ptr, stream

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64, 8), (30, 44, 4), (7, 9, 2), (17, 33, 16), (224, 224, 7)]
SEED, P1, NM, N, K = 9, 0.5, 5, 2, 6
SENTINEL = -77.0


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


@pytest.fixture(scope="module")
def mask_sets():
    """the oracle's five masks of every shape, computed once"""
    return {(H, W, g): ro.masks(SEED, 0, NM, g, P1, H, W) for H, W, g in SHAPES}


@pytest.mark.parametrize("H,W,g", SHAPES)
def test_masks_match_the_oracle(H, W, g, mask_sets):
    want = mask_sets[(H, W, g)]
    buf = torch.full((NM + 2, H, W), SENTINEL, device=DEV)
    got = ops.rise_masks(SEED, 0, NM, g, P1, H, W, out=buf[1:1 + NM]).cpu().numpy()
    host = buf.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all(), "bytes outside the n masks were written"
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"{H}x{W} grid {g}: max abs error {err:.3e}")
    assert got.dtype == np.float32 and got.shape == want.shape and err <= 2.0 ** -24
    assert got.min() >= 0 and got.max() <= 1 and 0 < got.mean() < 1
    tail = ops.rise_masks(SEED, 3, NM - 3, g, P1, H, W, device=DEV).cpu().numpy()
    assert np.array_equal(tail, got[3:])                                            # bitwise
    assert np.array_equal(ops.rise_masks(SEED, 0, NM, g, P1, H, W, device=DEV).cpu().numpy(), got)      # repeatable
    other = ops.rise_masks(SEED + 1, 0, NM, g, P1, H, W, device=DEV).cpu().numpy()
    assert not np.array_equal(other, got)


@pytest.mark.parametrize("H,W,g", SHAPES)
def test_apply_matches_the_fp64_oracle(H, W, g, mask_sets):
    """r0 = 3 starts inside image 0 (mask 3) and n = 5 rows cross into image 1; 3 padded rows"""
    mask_set = mask_sets[(H, W, g)]
    rng = np.random.default_rng(H * W + g)
    img = rng.standard_normal((N, 3, H, W)).astype(np.float32)
    base = rng.standard_normal((N, 3, H, W)).astype(np.float32)
    r0, n, n_pad = 3, 5, 8
    want64 = ro.apply(img, base, SEED, g, P1, NM, r0, n, n_pad, dtype=np.float64, mask_set=mask_set)
    rows = [divmod(r0 + i, NM) for i in range(n)]
    m32 = torch.from_numpy(np.stack([mask_set[j] for _, j in rows]))[:, None]
    xi, bi = torch.from_numpy(img)[[a for a, _ in rows]], torch.from_numpy(base)[[a for a, _ in rows]]
    cpu32 = (bi + m32 * (xi - bi)).numpy()                                          # the same formula in torch CPU fp32
    assert [a for a, _ in rows] == [0, 0, 1, 1, 1]
    buf = torch.full((n_pad + 2, 3, H, W), SENTINEL, device=DEV)
    dev = [torch.from_numpy(a).to(DEV) for a in (img, base)]
    got = ops.rise_apply(*dev, SEED, g, P1, NM, r0, n, n_pad, out=buf[1:1 + n_pad]).cpu().numpy()
    host = buf.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all(), "bytes outside the n_pad rows were written"
    assert not host[1 + n:1 + n_pad].any()                                          # padded rows are exactly zero
    hip, cpu = rel_l2(got[:n], want64[:n]), rel_l2(cpu32, want64[:n])
    print(f"{H}x{W} grid {g}: rel L2 hip {hip:.3e}, torch cpu fp32 {cpu:.3e}")
    assert hip <= 3 * cpu + 1e-6
    again = ops.rise_apply(*dev, SEED, g, P1, NM, r0, n, n_pad).cpu().numpy()
    assert np.array_equal(again, got)                                               # repeatable; a fresh buffer takes the same path


@pytest.mark.parametrize("H,W", [(7, 9), (32, 33), (36, 36)])
def test_apply_tile_matches_the_restatement_bit_for_bit(H, W):
    """The pixel tile and the blend that rise_apply shares with faith_perturb (csrc/perturb_tile.h), bit for bit against
    rise_oracle.apply in fp32 (the test above holds the kernel to the fp64 formula only).  7x9: 63 pixels, no multiple of 4 and
    less than one tile of 1024: the dword path.  32x33: 1056 pixels, the 16-byte path with a second tile that is mostly empty
    (threads whose first pixel lies past the end).  36x36: 1296 pixels, two tiles of the 16-byte path.  Two images, rows 1 .. 3
    of two masks each (image 0 once, image 1 twice), two padded rows.  Image 1 is its own baseline, so its rows must come back
    exactly; image 0 has one NaN pixel."""
    g, n_masks, r0, n, n_pad = 4, 2, 1, 3, 5
    rng = np.random.default_rng(H * W)
    img = rng.standard_normal((2, 3, H, W)).astype(np.float32)
    base = rng.standard_normal((2, 3, H, W)).astype(np.float32)
    base[1] = img[1]
    img[0, 1, H // 2, W // 3] = np.nan
    want = ro.apply(img, base, SEED, g, P1, n_masks, r0, n, n_pad)
    buf = torch.full((n_pad + 2, 3, H, W), SENTINEL, device=DEV)
    got = ops.rise_apply(torch.from_numpy(img).to(DEV), torch.from_numpy(base).to(DEV), SEED, g, P1, n_masks, r0, n, n_pad,
                         out=buf[1:1 + n_pad]).cpu().numpy()
    host = buf.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[-1] == SENTINEL).all(), "bytes outside the n_pad rows were written"
    print(f"{H}x{W}: {int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())} of {got.size} values differ")
    assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
    assert not host[1 + n:1 + n_pad].any()                                          # padded rows are exactly zero
    assert np.array_equal(got[1], img[1]) and np.array_equal(got[2], img[1])        # baseline == image: the blend returns it
    assert int(np.isnan(got).sum()) == 1 and np.isnan(got[0, 1, H // 2, W // 3])


@pytest.mark.parametrize("n_masks", [1, 5, 67])
@pytest.mark.parametrize("H,W,g", SHAPES)
def test_accumulate_matches_the_oracle(H, W, g, n_masks, mask_sets):
    """67 masks = two LDS rounds of 32 and a ragged third"""
    mask_set = mask_sets[(H, W, g)][:n_masks] if n_masks <= NM else ro.masks(SEED, 0, n_masks, g, P1, H, W)
    gen = torch.Generator().manual_seed(H + n_masks)
    logits = torch.randn(N * n_masks + 2, K, generator=gen) * 3                     # two rows past the end: never read
    clean = torch.randn(N, K, generator=gen) * 3
    ld, cd = logits.to(DEV), clean.to(DEV)
    for target in (None, [4, 1]):
        td = None if target is None else torch.tensor(target, dtype=torch.int32, device=DEV)
        want = ro.accumulate(logits.numpy(), clean.numpy(), mask_set, target)
        out = (torch.full((N, H, W), float("nan"), device=DEV, dtype=torch.float64),
               torch.full((H, W), float("nan"), device=DEV, dtype=torch.float64),
               torch.full((N,), float("nan"), device=DEV, dtype=torch.float64), torch.full((N,), -1, device=DEV, dtype=torch.int32))
        total, coverage, clean_prob, used = ops.rise_accumulate(ld, cd, (H, W), SEED, g, P1, n_masks, td, out=out)
        assert used.cpu().tolist() == want["target"].tolist() == (target or clean.argmax(dim=1).tolist())
        for name, t in (("saliency_sum", total), ("coverage", coverage), ("clean_prob", clean_prob)):
            v = t.cpu().numpy()
            err = rel_l2(v, want[name])
            print(f"{H}x{W} grid {g} n_masks {n_masks} {name}: rel L2 {err:.3e}")
            assert t.dtype == torch.float64 and v.shape == want[name].shape and np.isfinite(v).all() and err <= 1e-10, name
        again = ops.rise_accumulate(ld, cd, (H, W), SEED, g, P1, n_masks, td)
        for a, b in zip((total, coverage, clean_prob, used), again):
            assert torch.equal(a, b)                                                # bitwise repeatable


def test_accumulate_more_images_than_one_workgroup_takes():
    """N = 6: two image groups of four, the second ragged; every image's sum is its own"""
    H, W, g, n_masks, N6 = 30, 44, 4, 5, 6
    mask_set = ro.masks(SEED, 0, n_masks, g, P1, H, W)
    gen = torch.Generator().manual_seed(6)
    logits, clean = torch.randn(N6 * n_masks, K, generator=gen) * 3, torch.randn(N6, K, generator=gen) * 3
    want = ro.accumulate(logits.numpy(), clean.numpy(), mask_set)
    total, coverage, clean_prob, used = ops.rise_accumulate(logits.to(DEV), clean.to(DEV), (H, W), SEED, g, P1, n_masks)
    assert used.cpu().tolist() == want["target"].tolist()
    assert rel_l2(total.cpu().numpy(), want["saliency_sum"]) <= 1e-10 and rel_l2(coverage.cpu().numpy(), want["coverage"]) <= 1e-10
    assert rel_l2(clean_prob.cpu().numpy(), want["clean_prob"]) <= 1e-10


def test_refused_arguments_launch_nothing():
    lib = _lib.load()
    H = W = 8
    x = torch.zeros(2, 3, H, W, device=DEV)
    out = torch.full((4, 3, H, W), 5.0, device=DEV)
    logits, clean = torch.zeros(10, K, device=DEV), torch.zeros(2, K, device=DEV)
    sums = [torch.full(s, 5.0, device=DEV, dtype=torch.float64) for s in ((2, H, W), (H, W), (2,))]
    used = torch.full((2,), 5, device=DEV, dtype=torch.int32)
    big = torch.zeros(1 << 16, device=DEV, dtype=torch.uint8)

    def masks(grid=4, p1=0.5, h=H, w=W, n=2):
        call("mmskin_rise_masks", 7, 0, n, grid, p1, h, w, ptr(out), stream())

    def apply(grid=4, p1=0.5, n_masks=5, r0=0, n=4, n_pad=4):
        call("mmskin_rise_apply", ptr(x), ptr(x), 2, H, W, 7, grid, p1, n_masks, r0, n, n_pad, ptr(out), stream())

    def accumulate(grid=4, p1=0.5, n_masks=5, k=K):
        call("mmskin_rise_accumulate", ptr(logits), None, ptr(clean), 2, k, H, W, 7, grid, p1, n_masks, ptr(sums[0]), ptr(sums[1]),
             ptr(sums[2]), ptr(used), ptr(big), stream())

    cases = [(masks, dict(grid=1), 1), (masks, dict(p1=0.0), 1), (masks, dict(n=0), 1), (masks, dict(h=257, w=256), 3),
             (apply, dict(grid=17), 1), (apply, dict(p1=1.0), 1), (apply, dict(n=5), 1), (apply, dict(r0=7), 1),
             (apply, dict(n_masks=0), 1), (apply, dict(n_masks=(1 << 20) + 1), 3),
             (accumulate, dict(grid=0), 1), (accumulate, dict(p1=-0.5), 1), (accumulate, dict(n_masks=(1 << 20) + 1), 3),
             (accumulate, dict(k=0), 1)]
    for fn, kw, code in cases:
        with pytest.raises(_lib.MMSkinError, match=f"error {code}"):
            fn(**kw)
    assert lib.mmskin_rise_workspace_bytes(2, 5) <= big.numel()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and all(bool((s == 5.0).all()) for s in sums) and bool((used == 5).all()), \
        "a refused call wrote to an output"
