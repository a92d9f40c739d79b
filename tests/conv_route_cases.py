"""The conv-GEMM route table as data (csrc/conv_gemm.hip conv_gemm_route, DESIGN.md section 4 "The conv-GEMM route").

Row = op, (N, Cin, H, W, Cout, k, stride, pad), element bytes, flags, the nine values mmskin_conv_route returns (family, bm, step, bn, nst, epi,
group_m, total_mblk, nblk_n), note.  tests/test_cpu_conv_route.py compares all nine without a device; the GPU tests take the route their
cases must run from route().  A Linear of M rows, K -> N is the convolution (M, K, 1, 1, N, 1, 1, 0).  Shapes are the LAYER's: a data
gradient (op 1) of (N, Cin, H, W, Cout, ...) is a GEMM with Cin output columns over a reduction of taps x Cout.

The expected values are worked out from the rules of DESIGN.md, e.g. ResNet-50 layer4 conv1 at batch 256 (1x1, 1024 -> 512 at 14 x 14): 50 176
rows, K = 1024 >= 1024; two 256-column blocks; 256-row tiles: 196 x 2 = 392 tiles = 2 rounds x 256 rows; 224-row tiles: 224 x 2 = 448 tiles
= 2 rounds x 224 rows -> the 224-row tile, 448 >= 192 tiles: pipelined, 224 row blocks.

Every template instantiation behind launch_route's switch is named by a row, or by UNREACHABLE with the reason."""
from collections import namedtuple

CG_TILE128, CG_BIG256, CG_PIPE, CG_C64, CG_STEM7 = 0, 1, 2, 3, 4
BF16, F32 = 2, 4
FWD, DGRAD, STEM, FIRST = 0, 1, 2, 3
# mmskin.h MMSKIN_CRF_* (op 0) and MMSKIN_CRD_* (op 1)
STATS, ROWS_FREE, BIAS, ADDEND, RELU, GELU, OUT_F32, RESIDUAL, MASK_OUT, MUL, NO_OUT = (1 << i for i in range(11))
D_ADDEND, D_ADDEND_IS_DIN, D_MASK_Y, D_MASK_BITS, D_X, D_SCALE_SHIFT, D_X2, D_IN2, D_BIAS, D_ADDEND_S2, D_PARTIAL, D_EMPTY = (1 << i for i in range(12))

TRAIN = STATS | ROWS_FREE                       # a training forward of the ResNet / MBConv plans: statistics, any row count
TR = RESIDUAL | OUT_F32 | BIAS                  # Linear + bias + layer scale + residual into the fp32 stream (BEiT / DaViT fc2, attention projection)
# the fused BatchNorm-backward prologues of the plans' data gradients, by the epilogue instantiation they select
EPI_FLAGS = {
    3: D_X | D_SCALE_SHIFT | D_PARTIAL,                       # conv -> BatchNorm -> ReLU unit (mmskin_conv2d_dgrad_fused)
    4: D_ADDEND | D_X | D_MASK_BITS | D_PARTIAL,              # the block's first conv: skip gradient added, mask from the block output's bits
    5: D_ADDEND | D_X | D_X2 | D_MASK_BITS | D_PARTIAL,       # ... of a block with a downsample BatchNorm
    7: D_MASK_BITS | D_PARTIAL,                               # mask bits alone (the algebraic BatchNorm backward takes no x)
    1: D_ADDEND | D_X | D_MASK_Y | D_PARTIAL,                 # everything else: the mask from the block output itself
}

Row = namedtuple("Row", "op shape eb flags want note")


def conv(N, Cin, H, W, Cout, k=1, stride=1, pad=0):
    return (N, Cin, H, W, Cout, k, stride, pad)


def linear(M, K, N):
    return (M, K, 1, 1, N, 1, 1, 0)


def _t128(Cout, bn, nst, epi, rows, gm=0):
    return (CG_TILE128, 128, 128, bn, nst, epi, gm, -(-rows // 128), Cout // bn)


def _pipe(Cout, bm, step, epi, blocks, gm=0):
    return (CG_PIPE, bm, step, 256, 8, epi, gm, blocks, Cout // 256)


def _big(Cout, epi, rows, gm=0):
    return (CG_BIG256, 256, 256, 256, 2, epi, gm, -(-rows // 256), Cout // 256)


R50 = 256 * 56 * 56   # rows of a ResNet-50 layer-1 map at batch 256
BEIT_M = 256 * 197    # BEiT-large tokens at batch 256

# ---- real layers: ResNet-50 at batch 256 (224 x 224), the DenseNet bottleneck, BERT-base / BEiT-large Linear layers
LAYER_ROWS = [
    Row(STEM, conv(256, 3, 224, 224, 64, 7, 2, 3), BF16, STATS, (CG_STEM7, 0, 0, 0, 0, 0, 0, 256 * 28, 1), "the direct 7x7 stem: one statistics row per four output rows"),
    Row(STEM, conv(256, 3, 224, 224, 64, 7, 2, 3), F32, STATS, _t128(64, 64, 1, 0, 256 * 112 * 112), "fp32 stem: the virtual 8-tap form"),
    Row(STEM, conv(8, 3, 64, 64, 64, 7, 2, 3), BF16, STATS, _t128(64, 64, 2, 0, 8 * 32 * 32), "a 32-wide stem output is not the direct kernel's"),
    Row(FIRST, conv(256, 3, 224, 224, 64, 3, 2, 1), BF16, STATS, _t128(64, 64, 1, 0, 256 * 112 * 112), "MobileNet-V2 / EfficientNet first conv (virtual 4-tap form)"),
    Row(FIRST, conv(8, 3, 64, 64, 64, 3, 1, 1), BF16, BIAS | RELU, _t128(64, 64, 2, 2, 8 * 64 * 64), "VGG first conv, folded inference epilogue"),
    Row(FWD, conv(256, 64, 56, 56, 64), BF16, TRAIN, _t128(64, 64, 1, 0, R50), "layer1 conv1: 6272 workgroups, single buffer"),
    Row(FWD, conv(256, 64, 56, 56, 64, 3, 1, 1), BF16, TRAIN, (CG_C64, 0, 0, 0, 0, 0, 0, 256, 1), "layer1 conv2: the all-taps kernel, one statistics row per image"),
    Row(FWD, conv(256, 64, 56, 56, 64, 3, 1, 1), BF16, STATS, _t128(64, 64, 1, 0, R50), "... a caller that sized 128-row statistics slabs keeps the 128-row tile"),
    Row(FWD, conv(256, 64, 56, 56, 64, 3, 1, 1), F32, TRAIN, _t128(64, 64, 1, 0, R50), "... and fp32"),
    Row(FWD, conv(256, 64, 56, 56, 256), BF16, TRAIN, _t128(256, 128, 1, 0, R50), "layer1 conv3: K = 64 is far below the pipelined kernel's depth"),
    Row(FWD, conv(256, 128, 28, 28, 128, 3, 1, 1), BF16, TRAIN, _t128(128, 128, 1, 0, R50 // 4), "layer2 conv2: K = 1152 but 128 columns"),
    Row(FWD, conv(256, 256, 14, 14, 256, 3, 1, 1), BF16, TRAIN, _pipe(256, 224, 224, 0, 224), "layer3 conv2: 196 tiles x 256 rows > 224 x 224"),
    Row(FWD, conv(256, 256, 14, 14, 256, 3, 1, 1), BF16, STATS, _t128(256, 128, 1, 0, R50 // 16), "... with fixed statistics rows: 392 x 2 workgroups"),
    Row(FWD, conv(256, 256, 14, 14, 1024), BF16, TRAIN, _t128(1024, 128, 1, 0, R50 // 16), "layer3 conv3: K = 256"),
    Row(FWD, conv(256, 1024, 14, 14, 512), BF16, TRAIN, _pipe(512, 224, 224, 0, 224), "layer4 conv1 (see the module docstring)"),
    Row(FWD, conv(256, 512, 7, 7, 512, 3, 1, 1), BF16, TRAIN, _t128(512, 128, 2, 0, R50 // 64), "layer4 conv2: 112 tiles < 192; 98 x 4 = 392 workgroups keep two stages"),
    Row(FWD, conv(256, 512, 7, 7, 2048), BF16, MUL | BIAS | ADDEND | RELU | MASK_OUT, _t128(2048, 128, 1, 2, R50 // 64),
        "layer4 conv3, second pass of the two-pass forward: BatchNorm scale / shift, residual, ReLU and its mask"),
    Row(FWD, conv(256, 512, 7, 7, 2048), BF16, STATS | ROWS_FREE | NO_OUT, _t128(2048, 128, 1, 0, R50 // 64), "... its first pass stores nothing: statistics only"),
    Row(FWD, conv(256, 1024, 14, 14, 2048, 1, 2, 0), BF16, TRAIN, _pipe(2048, 224, 224, 0, 56), "layer4 downsample: stride-2 gather, 56 x 8 = 448 tiles"),
    Row(FWD, conv(256, 256, 14, 14, 128), BF16, TRAIN, _t128(128, 128, 2, 0, R50 // 16), "DenseNet bottleneck: 392 workgroups"),
    Row(DGRAD, conv(256, 256, 14, 14, 256, 3, 1, 1), BF16, EPI_FLAGS[3], _pipe(256, 224, 224, 3, 224), "layer3 conv2 data gradient with conv1's BatchNorm backward"),
    Row(DGRAD, conv(256, 64, 56, 56, 64, 3, 1, 1), BF16, EPI_FLAGS[3], (CG_C64, 0, 0, 0, 0, 0, 0, 256, 1), "layer1 conv2 data gradient: the all-taps kernel's own fused form"),
    Row(DGRAD, conv(256, 64, 56, 56, 64, 3, 1, 1), BF16, EPI_FLAGS[4], _t128(64, 64, 1, 4, R50), "... it has no other profile"),
    Row(DGRAD, conv(256, 1024, 14, 14, 256), BF16, EPI_FLAGS[4], _t128(1024, 128, 1, 4, R50 // 16), "layer3 conv1 data gradient: the GEMM's K is the layer's Cout = 256"),
    Row(DGRAD, conv(256, 256, 14, 14, 1024), BF16, EPI_FLAGS[4], _pipe(256, 224, 224, 4, 224), "layer3 conv3 data gradient: K = 1024, pipelined with profile 4"),
    Row(DGRAD, conv(256, 512, 28, 28, 1024, 1, 2, 0), BF16, 0, _pipe(512, 224, 224, 0, 224), "layer3 downsample data gradient: three zero-filled parity classes + one GEMM class"),
    Row(DGRAD, conv(256, 256, 28, 28, 256, 3, 2, 1), BF16, EPI_FLAGS[3], _t128(256, 128, 1, 3, R50 // 4),
        "layer3 conv2 of the first block: four parity classes of 4, 2, 2, 1 taps, row-weighted K = 2.25 x 256 = 576"),
    Row(FWD, linear(BEIT_M, 1024, 4096), BF16, BIAS | GELU, _pipe(4096, 256, 256, 2, 197, 8), "BEiT-large fc1: 13 rounds x 256 rows < 15 x 224; 8 MB weight: grouped order"),
    Row(FWD, linear(BEIT_M, 4096, 1024), BF16, TR, _pipe(1024, 224, 224, 6, 226, 8), "BEiT-large fc2 with layer scale and residual: 4 rounds x 224 < 4 x 256"),
    Row(FWD, linear(256 * 128, 768, 3072), BF16, BIAS | GELU, _pipe(3072, 256, 256, 2, 128, 8), "BERT-base fc1 at 128 tokens: K = 768 pays for a Linear"),
    Row(FWD, linear(256 * 128, 3072, 768), BF16, BIAS | OUT_F32, _pipe(768, 224, 224, 2, 147), "BERT-base output.dense: 441 tiles of 224 rows = 2 rounds; three column blocks: no grouping"),
]

# ---- one row per instantiation class the layers above leave out.  128-row tiles: bn = 128 | 64 by the column count, NST 1 above 640 workgroups
# (800 for epilogue 1); shapes: a 1x1 layer over a 14 x 14 map at batch 512 / 8 (784 / 13 row blocks) with 128 | 64 columns
def _class_rows():
    rows = []
    for eb in (BF16, F32):
        for cols in (128, 64):
            for N in (512, 8):
                r = N * 196
                nst = 1 if -(-r // 128) * 1 > 640 else 2
                rows.append(Row(FWD, conv(N, 64, 14, 14, cols), eb, 0, _t128(cols, cols, nst, 0, r), "plain store"))
                rows.append(Row(FWD, conv(N, 64, 14, 14, cols), eb, BIAS | RELU, _t128(cols, cols, nst, 2, r), "light epilogue"))
                for epi in (3, 4, 5, 7):
                    rows.append(Row(DGRAD, conv(N, cols, 14, 14, 64), eb, EPI_FLAGS[epi], _t128(cols, cols, nst, epi, r), "BatchNorm-backward profile %d" % epi))
                # the everything-profile keeps two stages up to 800 workgroups: 784 stay, 1024 (batch 669 -> 1025 row blocks) go
                rows.append(Row(DGRAD, conv(N, cols, 14, 14, 64), eb, EPI_FLAGS[1], _t128(cols, cols, 2, 1, r), "everything-profile, 784 | 13 workgroups"))
            rows.append(Row(DGRAD, conv(669, cols, 14, 14, 64), eb, EPI_FLAGS[1], _t128(cols, cols, 1, 1, 669 * 196), "everything-profile above 800 workgroups"))
    return rows


CLASS_ROWS = _class_rows() + [
    Row(FWD, linear(BEIT_M, 1024, 384), BF16, TR, _t128(384, 128, 1, 6, BEIT_M), "transformer residual on 384 columns (no 256-column tile): 394 x 3 workgroups"),
    Row(FWD, linear(8 * 197, 1024, 384), BF16, TR, _t128(384, 128, 2, 6, 8 * 197), "... and 13 x 3"),
    Row(FWD, conv(1, 8256, 120, 120, 1024), BF16, 0, _big(1024, 0, 14400), "K = 8256 = 129 K-tiles is past the pipelined kernel's table: 57 x 4 = 228 tiles of 256 x 256"),
    Row(FWD, linear(14400, 8256, 1024), BF16, BIAS | RELU, _big(1024, 2, 14400, 8), "... as a Linear + bias + ReLU (16 MB weight: grouped order)"),
    Row(FWD, linear(14400, 8256, 1024), BF16, TR, _big(1024, 6, 14400, 8), "... and with the transformer-residual epilogue"),
    Row(FWD, conv(256, 1024, 14, 14, 512), BF16, BIAS | RELU, _pipe(512, 224, 224, 2, 224), "pipelined, folded-BatchNorm inference epilogue"),
    Row(DGRAD, conv(256, 512, 14, 14, 1024), BF16, EPI_FLAGS[5], _pipe(512, 224, 224, 5, 224), "pipelined, profile 5"),
    Row(FWD, linear(65536, 768, 256), BF16, 0, _pipe(256, 256, 256, 0, 256), "256 tiles of 256 rows = one round; 293 of 224 = two"),
    Row(DGRAD, linear(65536, 256, 768), BF16, EPI_FLAGS[3], _pipe(256, 256, 256, 3, 256), "... profile 3"),
    Row(DGRAD, linear(65536, 256, 768), BF16, EPI_FLAGS[4], _pipe(256, 256, 256, 4, 256), "... profile 4"),
    Row(DGRAD, linear(65536, 256, 768), BF16, EPI_FLAGS[5], _pipe(256, 256, 256, 5, 256), "... profile 5"),
    Row(FWD, linear(65536, 768, 256), BF16, TR, _pipe(256, 256, 256, 6, 256), "... transformer residual"),
]

# ---- both sides of every threshold
THRESHOLD_ROWS = [
    Row(FWD, linear(640 * 128, 64, 128), BF16, 0, _t128(128, 128, 2, 0, 640 * 128), "640 workgroups: two stages"),
    Row(FWD, linear(640 * 128 + 1, 64, 128), BF16, 0, _t128(128, 128, 1, 0, 641 * 128), "641: single buffer"),
    Row(FWD, conv(2, 64, 202, 202, 128), BF16, 0, _t128(128, 128, 2, 0, 2 * 202 * 202), "638 workgroups (tests/test_gpu_kernels.py runs it)"),
    Row(FWD, conv(2, 64, 203, 203, 128), BF16, 0, _t128(128, 128, 1, 0, 2 * 203 * 203), "644 workgroups (tests/test_gpu_kernels.py runs it)"),
    Row(FWD, conv(2, 64, 202, 202, 128), F32, 0, _t128(128, 128, 2, 0, 2 * 202 * 202), ""),
    Row(FWD, conv(2, 64, 203, 203, 128), F32, 0, _t128(128, 128, 1, 0, 2 * 203 * 203), ""),
    Row(DGRAD, linear(800 * 128, 128, 64), BF16, EPI_FLAGS[1], _t128(128, 128, 2, 1, 800 * 128), "everything-profile, 800 workgroups: two stages"),
    Row(DGRAD, linear(800 * 128 + 1, 128, 64), BF16, EPI_FLAGS[1], _t128(128, 128, 1, 1, 801 * 128), "801: single buffer"),
    Row(DGRAD, linear(641 * 128, 128, 64), BF16, EPI_FLAGS[3], _t128(128, 128, 1, 3, 641 * 128), "every other profile switches at 640"),
    Row(FWD, conv(256, 960, 14, 14, 256), BF16, TRAIN, _t128(256, 128, 1, 0, R50 // 16), "a convolution's K = 960 (the multiple of 64 below 1024): 128-row tile"),
    Row(FWD, conv(256, 1024, 14, 14, 256), BF16, TRAIN, _pipe(256, 224, 224, 0, 224), "K = 1024: pipelined"),
    Row(DGRAD, conv(256, 256, 28, 28, 448, 3, 2, 1), BF16, 0, _t128(256, 128, 1, 0, 4 * 256 * 196), "four parity classes of 4, 2, 2, 1 taps: row-weighted K = 2.25 x 448 = 1008"),
    Row(FWD, linear(65536, 704, 256), BF16, 0, _t128(256, 128, 1, 0, 65536), "a Linear's K = 704 (the multiple of 64 below 768)"),
    Row(FWD, linear(191 * 224, 768, 256), BF16, 0, _t128(256, 128, 1, 0, 191 * 224), "191 tiles of 224 rows: 335 x 2 workgroups of the 128-row tile"),
    Row(FWD, linear(191 * 224 + 1, 768, 256), BF16, 0, _pipe(256, 224, 224, 0, 192), "192 tiles"),
    Row(FWD, linear(56 * 256, 8256, 1024), BF16, 0, _big(1024, 0, 56 * 256, 8), "56 x 4 = 224 tiles of 256 x 256"),
    Row(FWD, linear(55 * 256, 8256, 1024), BF16, 0, _t128(1024, 128, 1, 0, 55 * 256, 8), "220 tiles: 128-row tile (110 x 8 workgroups)"),
    Row(FWD, linear(4096, 1024, 1024), BF16, 0, _t128(1024, 128, 2, 0, 4096), "a 2 MB weight is not above 2 MB: column blocks fastest"),
    Row(FWD, linear(4096, 1088, 1024), BF16, 0, _t128(1024, 128, 2, 0, 4096, 8), "2.125 MB: groups of 8 row blocks"),
    Row(FWD, linear(4096, 544, 1024), F32, 0, _t128(1024, 128, 2, 0, 4096, 8), "fp32: the same bytes at half the K"),
    Row(FWD, linear(15 * 128, 2048, 1024), BF16, 0, _t128(1024, 128, 2, 0, 15 * 128), "15 row blocks < two groups"),
    Row(FWD, linear(15 * 128 + 1, 2048, 1024), BF16, 0, _t128(1024, 128, 2, 0, 16 * 128, 8), "16 row blocks"),
    Row(FWD, linear(4096, 2048, 384), BF16, 0, _t128(384, 128, 2, 0, 4096), "three column blocks: no grouping"),
]

ROWS = LAYER_ROWS + CLASS_ROWS + THRESHOLD_ROWS

# MMSKIN_CONV_PIPE_FORCE=1 + MMSKIN_CONV_PIPE_TILE -> (bm, step, row blocks) of the first case of tests/test_gpu_conv_pipe.py (588 rows)
KNOB_SHAPE = conv(3, 256, 14, 14, 256, 3, 1, 1)
KNOB_TILES = {"256": (256, 256, 3), "224": (224, 224, 3), "196": (224, 196, 3)}

# Instantiation classes (element bytes, family, bm, step, bn, nst, epi) no launch reaches without a knob: a 196-row step never has fewer
# tiles than a 224-row step of the same 224 computed rows, and the tile-count model keeps the first of two equal costs
UNREACHABLE = {(BF16, CG_PIPE, 224, 196, 256, 8, epi): "only MMSKIN_CONV_PIPE_TILE=196 selects 196 valid rows" for epi in (0, 2, 3, 4, 5, 6)}


def route(lib, op, shape, eb, flags=0):
    """The nine values of mmskin_conv_route, or None when the route refuses the launch."""
    import ctypes
    out = (ctypes.c_int64 * 9)()
    N, Cin, H, W, Cout, k, stride, pad = shape
    if lib.mmskin_conv_route(op, N, Cin, H, W, Cout, k, k, stride, pad, eb, flags, out):
        return None
    return tuple(out)
