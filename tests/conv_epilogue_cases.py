"""The op-level epilogue cases of tests/test_gpu_conv_epilogues.py as data, each with the conv_gemm_kernel instantiation it is meant to run:
the first six values of mmskin_conv_route (family, bm, step, bn, nst, epi) for its shape, element size and flags.  The flags are the ones the
case passes to mmskin_conv2d_dgrad_epilogue / mmskin_conv2d_forward_epilogue, so tests/test_cpu_conv_epilogues.py can check the coverage
claim against the route table without a device: every (bn, nst) of the 128-row tile for epilogues 1, 2, 4, 5 and 7 in both element types,
and epilogues 2, 4 and 5 of the pipelined tiles (256 rows, 224 rows, 196 valid rows of 224).

Shapes are the LAYER's (N, Cin, H, W, Cout, k, stride, pad): a data gradient has Cin output columns over a reduction of taps x Cout."""
from collections import namedtuple

from conv_route_cases import (ADDEND, BF16, BIAS, CG_PIPE, CG_TILE128, D_ADDEND, D_ADDEND_IS_DIN, D_ADDEND_S2, D_MASK_BITS, D_MASK_Y, D_PARTIAL, D_SCALE_SHIFT,
                              D_X, D_X2, DGRAD, F32, FWD, KNOB_TILES, MASK_OUT, MUL, NO_OUT, RELU, ROWS_FREE, STATS, conv)

Case = namedtuple("Case", "name op shape dtype flags want")
EB = {"bf16": BF16, "fp32": F32}
DTYPES = ("fp32", "bf16")

# data-gradient flags by the epilogue they select (the residual-block profiles with the skip gradient as the addend)
P = {
    1: D_ADDEND | D_X | D_MASK_Y | D_PARTIAL,
    2: D_ADDEND,
    4: D_ADDEND | D_X | D_MASK_BITS | D_PARTIAL,
    5: D_ADDEND | D_X | D_X2 | D_MASK_BITS | D_PARTIAL,
    7: D_ADDEND | D_MASK_BITS | D_PARTIAL,
}
# the mask from x * scale + shift: alone (profile 3, what mmskin_conv2d_dgrad_fused attaches) and beside an addend and mask bits (profile 1)
SS3 = D_X | D_SCALE_SHIFT | D_PARTIAL
SS1 = D_ADDEND | D_X | D_SCALE_SHIFT | D_MASK_BITS | D_PARTIAL
F2 = MUL | BIAS | ADDEND | RELU | MASK_OUT      # second pass of the two-pass forward


def _t(bn, nst, epi):
    return (CG_TILE128, 128, 128, bn, nst, epi)


def _dgrad_cases():
    out = []
    for dt in DTYPES:
        def add(tag, shape, epi, nst, flags=None):
            bn = 128 if shape[1] % 128 == 0 else 64
            out.append(Case("dgrad-%s-epi%d-%s" % (tag, epi, dt), DGRAD, shape, dt, P[epi] if flags is None else flags, _t(bn, nst, epi)))
        for epi in (1, 2, 4, 5, 7):
            add("198rows-bn64", conv(2, 64, 9, 11, 128), epi, 2)          # ragged last row block, two row blocks
            add("198rows-bn128", conv(2, 128, 9, 11, 64), epi, 2)
        for epi in (4, 5):
            add("two-column-blocks", conv(2, 256, 9, 11, 128), epi, 2)    # a partial-sum column offset by n0
        for epi in (4, 7):
            add("49rows-3x3", conv(1, 128, 7, 7, 128, 3, 1, 1), epi, 2)   # fewer rows than one tile
        add("3x3-c64", conv(3, 64, 12, 12, 64, 3, 1, 1), 4, 2)            # width 12: not the all-taps kernel's
        for epi in (4, 1):
            add("3x3s2-odd", conv(2, 128, 15, 13, 128, 3, 2, 1), epi, 2)  # four parity classes, s_orow row indexing
        for epi in (2, 4, 5, 7):                                          # 644 row blocks: single buffer
            add("nst1-bn64", conv(2, 64, 203, 203, 64), epi, 1)
            add("nst1-bn128", conv(2, 128, 203, 203, 64), epi, 1)
        add("nst1-bn64", conv(2, 64, 227, 227, 64), 1, 1)                 # 806 row blocks: above the everything-profile's 800
        add("nst1-bn128", conv(2, 128, 227, 227, 64), 1, 1)
        add("638blocks", conv(2, 64, 202, 202, 64), 4, 2)                 # the sibling below the threshold keeps two stages
        add("addend-s2", conv(2, 128, 9, 11, 64), 4, 2, P[4] | D_ADDEND_S2)
        add("scale-shift", conv(2, 64, 9, 11, 128), 3, 2, SS3)
        add("scale-shift-bits", conv(2, 128, 9, 11, 64), 1, 2, SS1)
        add("in-place-1x1s2", conv(2, 256, 14, 14, 512, 1, 2, 0), 2, 2, D_ADDEND | D_ADDEND_IS_DIN)
        add("in-place-3x3", conv(3, 64, 12, 12, 64, 3, 1, 1), 2, 2, D_ADDEND | D_ADDEND_IS_DIN)
    return out


def _fwd_cases():
    out = []
    for dt in DTYPES:
        def add(tag, shape, flags, nst, epi):
            bn = 128 if shape[4] % 128 == 0 else 64
            out.append(Case("fwd-%s-%x-%s" % (tag, flags, dt), FWD, shape, dt, flags, _t(bn, nst, epi)))
        add("198rows", conv(2, 128, 9, 11, 256), F2, 2, 2)
        add("49rows", conv(1, 512, 7, 7, 64), F2, 2, 2)
        add("198rows", conv(2, 128, 9, 11, 256), BIAS | RELU, 2, 2)
        add("49rows", conv(1, 512, 7, 7, 64), MUL | BIAS | MASK_OUT, 2, 2)     # no ReLU: the mask is still written
        add("nst1-bn64", conv(2, 64, 203, 203, 64), F2, 1, 2)
        add("nst1-bn128", conv(2, 64, 203, 203, 128), F2, 1, 2)
        for tag, shape in (("198rows", conv(2, 128, 9, 11, 256)), ("49rows", conv(1, 512, 7, 7, 64)), ("3x3s2", conv(2, 128, 15, 13, 128, 3, 2, 1))):
            for flags in (STATS, STATS | ROWS_FREE, STATS | ROWS_FREE | NO_OUT):
                add("stats-" + tag, shape, flags, 2, 0)
    return out


DGRAD_CASES = _dgrad_cases()
FWD_CASES = _fwd_cases()
TWO_PASS_SHAPE = conv(2, 128, 9, 11, 256)       # pass 1: STATS | ROWS_FREE | NO_OUT, pass 2: F2, then a profile-4 data gradient of a 1x1 256 -> 128 layer
TWO_PASS_NEXT = conv(2, 256, 9, 11, 128)

# pipelined tiles: MMSKIN_CONV_PIPE_FORCE=1 and MMSKIN_CONV_PIPE_TILE=tile in a fresh interpreter (bf16 only)
PIPE_LAUNCHES = [
    ("dgrad", conv(3, 256, 14, 14, 256, 3, 1, 1), P[4], 4), ("dgrad", conv(3, 256, 14, 14, 256, 3, 1, 1), P[5], 5),
    ("dgrad", conv(2, 256, 9, 11, 512), P[4], 4), ("dgrad", conv(2, 256, 9, 11, 512), P[5], 5),
    ("fwd", conv(3, 256, 14, 14, 256, 3, 1, 1), BIAS | ADDEND | RELU, 2),
]


def pipe_cases(tile):
    bm, step, _ = KNOB_TILES[tile]
    return [Case("pipe%s-%s-%s-epi%d" % (tile, kind, "x".join(map(str, shape)), epi), DGRAD if kind == "dgrad" else FWD, shape, "bf16", flags,
                 (CG_PIPE, bm, step, 256, 8, epi)) for kind, shape, flags, epi in PIPE_LAUNCHES]


# A statistics-only forward pass (no output) of the layer-1 3x3 shape the all-taps kernel takes: that kernel always stores its tile, so the
# route must keep the launch on the 128-row tile; with an output the same launch goes to the all-taps kernel (one statistics row per image)
from conv_route_cases import CG_C64
NO_OUT_C64_SHAPE = conv(32, 64, 8, 56, 64, 3, 1, 1)
NO_OUT_C64_ROUTES = [
    (STATS | ROWS_FREE, (CG_C64, 0, 0, 0, 0, 0, 0, 32, 1)),
    (STATS | ROWS_FREE | NO_OUT, (CG_TILE128, 128, 128, 64, 2, 0, 0, 32 * 8 * 56 // 128, 1)),
]

# the launches every entry point must refuse before it launches anything: (name, op, shape, flags, operands to drop / add)
REFUSALS = [
    ("flag-without-pointer", DGRAD, conv(2, 64, 9, 11, 128), P[4], {"x": None}),
    ("pointer-without-flag", DGRAD, conv(2, 64, 9, 11, 128), P[4] & ~D_X, {}),
    ("scale-shift-without-x", DGRAD, conv(2, 64, 9, 11, 128), D_SCALE_SHIFT | D_PARTIAL, {}),
    ("addend-s2-on-3x3", DGRAD, conv(3, 64, 12, 12, 64, 3, 1, 1), P[4] | D_ADDEND_S2, {}),
    ("fusion-on-in-place-1x1s2", DGRAD, conv(2, 256, 14, 14, 512, 1, 2, 0), D_ADDEND | D_ADDEND_IS_DIN | D_X | D_MASK_BITS | D_PARTIAL, {}),
]
