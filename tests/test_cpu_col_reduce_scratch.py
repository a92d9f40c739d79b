"""CPU: the scratch rule of the fp64 column reducer (csrc/bn.hip finalize_columns; no device needed: host arithmetic behind the C ABI).

Above MMSKIN_BN_SINGLE_ROWS partial rows a finalize entry first reduces every slab to G = min(64, ceil(nrows / 32)) rows of doubles and checks
slabs * G * cols_total against the capacity its caller carved (mmskin_col_reduce_scratch_check IS that check).  Every plan and op carves
bn_reduce_scratch_bytes(maxC) = col_reduce_scratch_doubles(2 * maxC) doubles; the table below is every call site's (slabs, cols_total)
against the maxC of its carve.  Each must fit at any row count, the worst of them exactly, and a carve one group row short must be refused
once the row count needs all 64 groups."""
import pytest

from mmskin import _lib

# (site, slabs, cols_total, channels the scratch was carved for)
SITES = [
    ("bn_finalize: two split slabs of C columns", 2, 512, 512),
    ("bn_finalize, ResNet-50 layer 4", 2, 2048, 2048),
    ("bn_bwd_finalize / slice_stats table: one interleaved [row][2][C] slab", 1, 2 * 2048, 2048),
    ("bn_table_finalize, MBConv: two split slabs of Cp columns", 2, 2560, 2560),
    ("bn_table_finalize, DenseNet conv2: two split slabs of G_PAD = 64 columns in a carve for at least BOTTLE = 128 channels", 2, 64, 128),
    ("bias_grad_finalize, VGG column_stats: one slab of Cout columns", 1, 512, 512),
    ("bias_grad_finalize, VGG after a fused dgrad: one slab of 2 * Cin columns", 1, 2 * 512, 512),
    ("the smallest carve: 64 channels", 2, 64, 64),
]


def test_scratch_doubles_is_64_rows_of_the_slab():
    lib = _lib.load()
    for cols in (1, 64, 72, 4096):
        assert lib.mmskin_col_reduce_scratch_doubles(cols) == 64 * cols
    assert lib.mmskin_col_reduce_scratch_doubles(-1) == -1


@pytest.mark.parametrize("site", SITES, ids=lambda s: s[0].split(":")[0].replace(" ", "_"))
def test_every_call_site_fits_its_carve_and_a_short_carve_is_refused(site):
    _, slabs, cols, carved_c = site
    lib = _lib.load()
    cap = lib.mmskin_col_reduce_scratch_doubles(2 * carved_c)
    assert slabs * 64 * cols <= cap
    for nrows in (1, 5, 513, 2017, 2048, 25088, 10 ** 6):               # G = 1, 1, 17, 64 (2017 = 63 * 32 + 1), 64, 64, 64
        _lib.check(lib.mmskin_col_reduce_scratch_check(slabs, nrows, cols, cap))
    exact = slabs * 64 * cols                                          # what 64 groups write
    _lib.check(lib.mmskin_col_reduce_scratch_check(slabs, 2048, cols, exact))
    _lib.check(lib.mmskin_col_reduce_scratch_check(slabs, 63 * 32, cols, exact - slabs * cols))   # 63 groups fit a carve one group row short
    for nrows in (2017, 2048, 25088):                                  # ... 64 groups do not
        with pytest.raises(_lib.MMSkinError, match="finalize_columns"):
            _lib.check(lib.mmskin_col_reduce_scratch_check(slabs, nrows, cols, exact - 1))
        with pytest.raises(_lib.MMSkinError, match="finalize_columns"):
            _lib.check(lib.mmskin_col_reduce_scratch_check(slabs, nrows, cols, exact - slabs * cols))


def test_a_wider_stride_than_the_carve_is_refused():
    """The case the rule exists for: a caller whose slab rows are wider apart than 2 * maxC (here a stride of 3 * C in a carve for C)."""
    lib = _lib.load()
    cap = lib.mmskin_col_reduce_scratch_doubles(2 * 256)
    _lib.check(lib.mmskin_col_reduce_scratch_check(1, 600, 3 * 256, cap))          # 19 groups still fit
    with pytest.raises(_lib.MMSkinError, match="finalize_columns"):
        _lib.check(lib.mmskin_col_reduce_scratch_check(1, 2048, 3 * 256, cap))
    for bad in ((0, 10, 64, cap), (1, 0, 64, cap), (1, 10, 0, cap), (1, 10, 64, -5)):
        with pytest.raises(_lib.MMSkinError):
            _lib.check(lib.mmskin_col_reduce_scratch_check(*bad))
