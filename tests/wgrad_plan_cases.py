"""The weight-gradient route table as data (csrc/wgrad.hip wgrad_plan, DESIGN.md section 4 "The weight-gradient plan").

Row = (N, Cin, H, W, Cout, k, stride, pad), element type, expected (family, tile_o, tile_k, variant), note.  The split count, rows or
stages per split, reduction form and slab floats of every row are pinned in EXPECT below (what mmskin_conv_wgrad_plan returns: eight values).
tests/test_cpu_wgrad_plan.py compares all eight without a device; tests/test_gpu_wgrad_ring.py and test_gpu_kernels.py take the family and tile
their cases must run from here.  The 7x7 / stride 2 stem and the 3-channel 3x3 first conv are planned in the virtual form the plans run.

Every template instantiation behind the launchers' switches is named by a row:
  WG_STAGED  wgrad_kernel<T, 128x128 | 128x64 | 64x128 | 64x64>, the three wide bf16 tiles also in the S1 form (variant 1)
  WG_TAPS3   wgrad3x3_kernel
  WG_RING    wgrad_ring_kernel 256x128, 128x256, 128x128, 256x64, 64x256, 128x64, 64x128, each plain (variant 0) and S1 (variant 1)
  WG_RING3   wgrad3_ring_kernel 128-cout tile with 2 | 3 window pieces per wave, 64-cout tile with 3 | 4 | 5 | 6
UNREACHABLE lists the instantiations no shape reaches."""
from collections import namedtuple

WG_STAGED, WG_TAPS3, WG_RING, WG_RING3 = 0, 1, 2, 3
WGR_DIRECT, WGR_LANES = 0, 1
BF16, F32 = 2, 4

Row = namedtuple("Row", "shape eb family tile_o tile_k variant note")


def conv(N, Cin, H, W, Cout, k=1, stride=1, pad=0):
    return (N, Cin, H, W, Cout, k, stride, pad)


def c3(N, Cin, H, W, Cout):
    return (N, Cin, H, W, Cout, 3, 1, 1)


# ---- tests/test_gpu_wgrad_ring.py CASES (bf16), in its order; the notes say what runs
RING_ROWS = [
    Row(conv(2, 64, 14, 14, 256), BF16, WG_RING, 256, 64, 1, "256x64 tile, two pixel groups meet in LDS, ragged last iteration (392 = 6*64 + 8)"),
    Row(conv(2, 256, 14, 14, 64), BF16, WG_RING, 64, 256, 1, "Cout = 64: 64x256 tile, two groups"),
    Row(conv(2, 256, 9, 11, 128), BF16, WG_RING, 128, 128, 1, "128x128 tile (1x1 / stride 1 takes it before 128x256), two groups, odd sizes, ragged last stage"),
    Row(conv(3, 128, 10, 10, 256), BF16, WG_RING, 128, 128, 1, "128x128 tile (1x1 / stride 1 takes it before 256x128), two cout tiles"),
    Row(conv(2, 128, 12, 12, 128), BF16, WG_RING, 128, 128, 1, "128x128 tile, two groups"),
    Row(conv(24, 128, 14, 14, 256), BF16, WG_RING, 128, 128, 1, "128x128 tiles over 9 splits of 576 rows, the last one short (4704 = 8*576 + 96)"),
    Row(conv(40, 64, 14, 14, 256), BF16, WG_RING, 256, 64, 1, "two-group tile over 14 splits"),
    Row(conv(2, 256, 14, 14, 512, 1, 2, 0), BF16, WG_RING, 256, 128, 0, "stride-2 gather (downsample 1x1), 256x128 tiles: 2 cout tiles x 2 k tiles"),
    Row(conv(3, 256, 15, 13, 256, 1, 2, 0), BF16, WG_RING, 256, 128, 0, "stride-2 gather on odd sizes"),
    Row(conv(2, 128, 14, 14, 128, 3, 2, 1), BF16, WG_RING, 128, 128, 0, "3x3 stride 2: nine taps, padding taps zero-filled by out-of-range offsets"),
    Row(conv(2, 128, 15, 13, 128, 3, 2, 1), BF16, WG_RING, 128, 128, 0, "3x3 stride 2, odd sizes"),
    Row(conv(16, 128, 28, 28, 128, 3, 2, 1), BF16, WG_RING, 128, 128, 0, "3x3 stride 2 over 6 splits that cross image boundaries"),
    Row(conv(2, 64, 12, 12, 256, 3, 2, 1), BF16, WG_RING, 256, 64, 0, "Cin = 64: nine 64-wide k tiles, one tap each, 256x64 tiles"),
    Row(conv(3, 192, 14, 14, 128), BF16, WG_RING, 128, 64, 1, "128x64 tiles, FOUR pixel groups of two waves (DenseNet bottleneck: Ktot = 64 x 3), ragged"),
    Row(conv(24, 320, 14, 14, 128), BF16, WG_RING, 128, 64, 1, "128x64 tiles over several splits"),
    Row(conv(3, 128, 14, 14, 64), BF16, WG_RING, 64, 128, 1, "64x128 tiles, four groups"),
    # the instantiations the cases above leave out: the smallest shape that reaches each
    Row(conv(2, 256, 14, 14, 128, 1, 2, 0), BF16, WG_RING, 128, 256, 0, "128x256 tile (one group of 8 waves) on a stride-2 gather"),
    Row(conv(2, 64, 14, 14, 128, 1, 2, 0), BF16, WG_RING, 128, 64, 0, "128x64 tile, four groups, on a stride-2 gather"),
    Row(conv(2, 128, 14, 14, 64, 1, 2, 0), BF16, WG_RING, 64, 128, 0, "64x128 tile, four groups, on a stride-2 gather"),
    Row(conv(2, 256, 14, 14, 64, 1, 2, 0), BF16, WG_RING, 64, 256, 0, "64x256 tile, two groups, on a stride-2 gather"),
]
# ---- tests/test_gpu_wgrad_ring.py CASES3 (3x3 / stride 1 / pad 1, bf16)
RING3_ROWS = [
    Row(c3(3, 64, 56, 56, 64), BF16, WG_RING3, 64, 64, 6, "one 56-wide row per stage, 64-cout tile: two groups take alternate stages and meet in LDS"),
    Row(c3(5, 64, 14, 14, 128), BF16, WG_RING3, 128, 64, 2, "four rows per stage, ragged last stage of every image (14 = 4+4+4+2), 128-cout tile"),
    Row(c3(3, 128, 28, 28, 128), BF16, WG_RING3, 128, 64, 2, "two rows per stage, two cin tiles"),
    Row(c3(4, 128, 7, 7, 256), BF16, WG_RING3, 128, 64, 3, "whole 7x7 images per stage, two cout tiles x two cin tiles"),
    Row(c3(2, 64, 9, 13, 64), BF16, WG_RING3, 64, 64, 3, "odd sizes: 4 rows of 13"),
    Row(c3(6, 64, 28, 28, 64), BF16, WG_RING3, 64, 64, 4, "64-cout tile at width 28"),
    Row(c3(9, 64, 7, 7, 64), BF16, WG_RING3, 64, 64, 5, "64-cout tile at width 7: odd stage count, the second group's last stage is empty"),
    Row(c3(70, 64, 14, 14, 64), BF16, WG_RING3, 64, 64, 3, "16 splits that start inside images"),
    Row(c3(40, 128, 14, 14, 128), BF16, WG_RING3, 128, 64, 2, "128-cout tile over 10 splits"),
]
# ---- tests/test_gpu_kernels.py test_wgrad3x3_multi_stage_splits: its three shapes run the ring; the fourth reaches the register-staged
# all-taps kernel (the ring refuses a window of (12 + 2) x 16 rows), whose split count MMSKIN_WGRAD3_BLOCKS sets
MULTI_STAGE_ROWS = [
    Row(c3(5, 64, 14, 14, 128), BF16, WG_RING3, 128, 64, 2, ""),
    Row(c3(3, 128, 9, 13, 64), BF16, WG_RING3, 64, 64, 3, ""),
    Row(c3(2, 64, 56, 56, 64), BF16, WG_RING3, 64, 64, 6, ""),
    Row(c3(37, 64, 30, 5, 64), BF16, WG_TAPS3, 64, 64, 0, "12 rows of 5 per stage, 3 stages per image (12 + 12 + 6), 111 stages"),
]
# MMSKIN_WGRAD3_BLOCKS -> (nsplit, stages per split) of the WG_TAPS3 row: splits start inside images (37 and 19 are no multiples of 3)
TAPS3_KNOB = {"3": (3, 37), "7": (6, 19)}
# ---- the register-staged forms, the virtual geometries, and a bf16 shape the ring does not tile
OTHER_ROWS = [
    Row(conv(2, 128, 14, 14, 128), F32, WG_STAGED, 128, 128, 0, "fp32 128x128"),
    Row(conv(2, 64, 14, 14, 128), F32, WG_STAGED, 128, 64, 0, "fp32 128x64"),
    Row(conv(2, 128, 14, 14, 64), F32, WG_STAGED, 64, 128, 0, "fp32 64x128"),
    Row(conv(2, 64, 14, 14, 64), F32, WG_STAGED, 64, 64, 0, "fp32 64x64"),
    Row(c3(3, 64, 12, 12, 64), F32, WG_STAGED, 64, 64, 0, "fp32 3x3: the all-taps families are bf16 only"),
    Row(conv(2, 64, 14, 14, 64), BF16, WG_STAGED, 64, 64, 0, "bf16 Cout = 64 with Ktot = 64 x odd: no ring tile"),
    Row(conv(2, 192, 14, 14, 64), BF16, WG_STAGED, 64, 64, 0, "bf16 Cout = 64, Ktot = 64 x 3"),
    Row(conv(2, 3, 64, 64, 64, 7, 2, 3), BF16, WG_RING, 64, 256, 0, "virtual stem: 8 row taps x 32 elements, Ktot = 256"),
    Row(conv(2, 3, 64, 64, 64, 7, 2, 3), F32, WG_STAGED, 64, 128, 0, "virtual stem, fp32"),
    Row(conv(2, 3, 64, 64, 64, 3, 1, 1), BF16, WG_RING, 64, 128, 0, "virtual first conv (VGG): 4 taps x 32 elements, Ktot = 128"),
    Row(conv(2, 3, 64, 64, 64, 3, 2, 1), BF16, WG_RING, 64, 128, 0, "virtual first conv, stride 2 (MobileNet-V2 / EfficientNet)"),
    Row(conv(2, 3, 64, 64, 64, 3, 1, 1), F32, WG_STAGED, 64, 128, 0, "virtual first conv, fp32"),
]
# The bf16 register-staged kernel is reached where the ring refuses: past its 32-bit byte offsets (a tensor of 3.75 GB or more) or its
# reciprocal pixel stepping ((OW + step) * OW >= 65536 on a gathering launch).  Rows whose tensors are never allocated: plan only.
PLAN_ONLY_ROWS = [
    Row(conv(7340032, 128, 1, 1, 256), BF16, WG_STAGED, 128, 128, 1, "bf16 staged 128x128 S1: dy of 3.76 GB (a Linear of 7.3 M rows)"),
    Row(conv(7340032, 64, 1, 1, 256), BF16, WG_STAGED, 128, 64, 1, "bf16 staged 128x64 S1"),
    Row(conv(14680064, 128, 1, 1, 192), BF16, WG_STAGED, 64, 128, 1, "bf16 staged 64x128 S1: dy of 5.6 GB"),
    Row(conv(4, 128, 239, 239, 128, 3, 1, 1), BF16, WG_STAGED, 128, 128, 0, "bf16 staged 128x128 gather: W > 64 keeps the 3x3 families out, 239 * (239 + 64) >= 65536 the ring"),
    Row(conv(4, 64, 239, 239, 128, 3, 1, 1), BF16, WG_STAGED, 128, 64, 0, "bf16 staged 128x64 gather"),
    Row(conv(4, 128, 239, 239, 64, 3, 1, 1), BF16, WG_STAGED, 64, 128, 0, "bf16 staged 64x128 gather"),
]
# ---- more than 32 splits (the four-lane reduction) in every class a plan's layers reach it in: the smallest such layer of the seven plans
# at 224 x 224 batch 256 or 64 x 64 batch 8
LANES_ROWS = [
    Row(c3(8, 64, 64, 64, 64), BF16, WG_STAGED, 64, 64, 0, "VGG conv1_2 at 64^2: W = 64 is past both 3x3 families, Ktot = 64 x 9 has no ring tile"),
    Row(c3(8, 64, 64, 64, 64), F32, WG_STAGED, 64, 64, 0, ""),
    Row(conv(8, 64, 32, 32, 128), F32, WG_STAGED, 128, 64, 0, ""),
    Row(c3(8, 128, 32, 32, 128), F32, WG_STAGED, 128, 128, 0, ""),
    Row(conv(256, 384, 14, 14, 64), BF16, WG_RING, 64, 128, 1, "MobileNet-V2 projection"),
    Row(conv(256, 512, 14, 14, 192), BF16, WG_RING, 64, 256, 1, ""),
    Row(conv(256, 64, 14, 14, 384), BF16, WG_RING, 128, 64, 1, "MobileNet-V2 expansion"),
    Row(conv(256, 256, 14, 14, 128), BF16, WG_RING, 128, 128, 1, "DenseNet bottleneck"),
    Row(conv(256, 64, 28, 28, 256), BF16, WG_RING, 256, 64, 1, ""),
    Row(conv(256, 256, 14, 14, 512, 1, 2, 0), BF16, WG_RING, 256, 128, 0, "ResNet-50 layer4 downsample"),
    Row(c3(256, 128, 14, 14, 64), BF16, WG_RING3, 64, 64, 3, "DenseNet conv2"),
    Row(c3(256, 128, 28, 28, 128), BF16, WG_RING3, 128, 64, 2, "ResNet layer2 conv2"),
]
# The plan gives a 1x1 / stride 1 launch the 128x128 tile wherever both widths divide by 128, so it never asks for the S1 form of these two;
# the Gram launcher (launch_wgrad_gram, tests/test_gpu_abn.py) runs them.
UNREACHABLE = [(WG_RING, 256, 128, 1), (WG_RING, 128, 256, 1)]

ROWS = RING_ROWS + RING3_ROWS + MULTI_STAGE_ROWS + OTHER_ROWS + PLAN_ONLY_ROWS + LANES_ROWS

# (shape, element bytes) -> (nsplit, rows or stages per split, reduce, slab floats), worked out from the split rules of DESIGN.md section 4.
# E.g. (24, 128, 14, 14, 256) bf16: M = 4704 rows, 128x128 tiles with two groups step 64 rows; 256 / 2 tiles = 128 splits wanted, at most
# 4704 / (8 * 64) = 9; ceil(4704 / 9) = 523 -> 576 rows per split, 9 splits; 9 * 256 * 128 floats.
EXPECT = {
    ((2, 64, 14, 14, 256, 1, 1, 0), 2): (1, 448, 0, 16384),
    ((2, 256, 14, 14, 64, 1, 1, 0), 2): (1, 448, 0, 16384),
    ((2, 256, 9, 11, 128, 1, 1, 0), 2): (1, 256, 0, 32768),
    ((3, 128, 10, 10, 256, 1, 1, 0), 2): (1, 320, 0, 32768),
    ((2, 128, 12, 12, 128, 1, 1, 0), 2): (1, 320, 0, 16384),
    ((24, 128, 14, 14, 256, 1, 1, 0), 2): (9, 576, 0, 294912),
    ((40, 64, 14, 14, 256, 1, 1, 0), 2): (14, 576, 0, 229376),
    ((2, 256, 14, 14, 512, 1, 2, 0), 2): (1, 128, 0, 131072),
    ((3, 256, 15, 13, 256, 1, 2, 0), 2): (1, 192, 0, 65536),
    ((2, 128, 14, 14, 128, 3, 2, 1), 2): (1, 128, 0, 147456),
    ((2, 128, 15, 13, 128, 3, 2, 1), 2): (1, 128, 0, 147456),
    ((16, 128, 28, 28, 128, 3, 2, 1), 2): (6, 576, 0, 884736),
    ((2, 64, 12, 12, 256, 3, 2, 1), 2): (1, 128, 0, 147456),
    ((3, 192, 14, 14, 128, 1, 1, 0), 2): (1, 640, 0, 24576),
    ((24, 320, 14, 14, 128, 1, 1, 0), 2): (4, 1280, 0, 163840),
    ((3, 128, 14, 14, 64, 1, 1, 0), 2): (1, 640, 0, 8192),
    ((2, 256, 14, 14, 128, 1, 2, 0), 2): (1, 128, 0, 32768),
    ((2, 64, 14, 14, 128, 1, 2, 0), 2): (1, 128, 0, 8192),
    ((2, 128, 14, 14, 64, 1, 2, 0), 2): (1, 128, 0, 8192),
    ((2, 256, 14, 14, 64, 1, 2, 0), 2): (1, 128, 0, 16384),
    ((3, 64, 56, 56, 64, 3, 1, 1), 2): (10, 18, 0, 368640),
    ((5, 64, 14, 14, 128, 3, 1, 1), 2): (1, 20, 0, 73728),
    ((3, 128, 28, 28, 128, 3, 1, 1), 2): (2, 21, 0, 294912),
    ((4, 128, 7, 7, 256, 3, 1, 1), 2): (1, 4, 0, 294912),
    ((2, 64, 9, 13, 64, 3, 1, 1), 2): (1, 6, 0, 36864),
    ((6, 64, 28, 28, 64, 3, 1, 1), 2): (5, 18, 0, 184320),
    ((9, 64, 7, 7, 64, 3, 1, 1), 2): (1, 10, 0, 36864),
    ((70, 64, 14, 14, 64, 3, 1, 1), 2): (16, 18, 0, 589824),
    ((40, 128, 14, 14, 128, 3, 1, 1), 2): (10, 16, 0, 1474560),
    ((3, 128, 9, 13, 64, 3, 1, 1), 2): (1, 10, 0, 73728),
    ((2, 64, 56, 56, 64, 3, 1, 1), 2): (7, 16, 0, 258048),
    ((37, 64, 30, 5, 64, 3, 1, 1), 2): (6, 19, 0, 221184),
    ((2, 128, 14, 14, 128, 1, 1, 0), 4): (3, 160, 0, 49152),
    ((2, 64, 14, 14, 128, 1, 1, 0), 4): (3, 160, 0, 24576),
    ((2, 128, 14, 14, 64, 1, 1, 0), 4): (3, 160, 0, 24576),
    ((2, 64, 14, 14, 64, 1, 1, 0), 4): (1, 448, 0, 4096),
    ((3, 64, 12, 12, 64, 3, 1, 1), 4): (1, 448, 0, 36864),
    ((2, 64, 14, 14, 64, 1, 1, 0), 2): (1, 512, 0, 4096),
    ((2, 192, 14, 14, 64, 1, 1, 0), 2): (1, 512, 0, 12288),
    ((2, 3, 64, 64, 64, 7, 2, 3), 2): (4, 512, 0, 65536),
    ((2, 3, 64, 64, 64, 7, 2, 3), 4): (16, 128, 0, 262144),
    ((2, 3, 64, 64, 64, 3, 1, 1), 2): (8, 1024, 0, 65536),
    ((2, 3, 64, 64, 64, 3, 2, 1), 2): (2, 1024, 0, 16384),
    ((2, 3, 64, 64, 64, 3, 1, 1), 4): (64, 128, 1, 524288),
    ((7340032, 128, 1, 1, 256, 1, 1, 0), 2): (256, 28672, 1, 8388608),
    ((7340032, 64, 1, 1, 256, 1, 1, 0), 2): (256, 28672, 1, 4194304),
    ((14680064, 128, 1, 1, 192, 1, 1, 0), 2): (170, 86400, 1, 4177920),
    ((4, 128, 239, 239, 128, 3, 1, 1), 2): (112, 2048, 1, 16515072),
    ((4, 64, 239, 239, 128, 3, 1, 1), 2): (112, 2048, 1, 8257536),
    ((4, 128, 239, 239, 64, 3, 1, 1), 2): (112, 2048, 1, 8257536),
    ((8, 64, 64, 64, 64, 3, 1, 1), 2): (64, 512, 1, 2359296),
    ((8, 64, 64, 64, 64, 3, 1, 1), 4): (103, 320, 1, 3796992),
    ((8, 64, 32, 32, 128, 1, 1, 0), 4): (64, 128, 1, 524288),
    ((8, 128, 32, 32, 128, 3, 1, 1), 4): (64, 128, 1, 9437184),
    ((256, 384, 14, 14, 64, 1, 1, 0), 2): (49, 1024, 1, 1204224),
    ((256, 512, 14, 14, 192, 1, 1, 0), 2): (42, 1216, 1, 4128768),
    ((256, 64, 14, 14, 384, 1, 1, 0), 2): (49, 1024, 1, 1204224),
    ((256, 256, 14, 14, 128, 1, 1, 0), 2): (98, 512, 1, 3211264),
    ((256, 64, 28, 28, 256, 1, 1, 0), 2): (242, 832, 1, 3964928),
    ((256, 256, 14, 14, 512, 1, 2, 0), 2): (49, 256, 1, 6422528),
    ((256, 128, 14, 14, 64, 3, 1, 1), 2): (64, 16, 1, 4718592),
    ((256, 128, 28, 28, 128, 3, 1, 1), 2): (128, 28, 1, 18874368),
}


def plan(lib, shape, eb):
    """The eight values of mmskin_conv_wgrad_plan, or None when no kernel takes the shape."""
    import ctypes
    out = (ctypes.c_int64 * 8)()
    N, Cin, H, W, Cout, k, stride, pad = shape
    if lib.mmskin_conv_wgrad_plan(N, Cin, H, W, Cout, k, k, stride, pad, eb, out):
        return None
    return tuple(out)


def pad64(c):
    return (c + 63) // 64 * 64


# ---- the convolutions whose weight gradient a plan computes through launch_conv_wgrad / the virtual launchers, as (N, Cin, H, W, Cout, k, stride, pad)
# with the operand padding the plan applies
def plan_conv_units(lib, arch, N, H, W):
    import ctypes
    import re
    if arch.startswith("densenet"):
        units = [conv(N, 3, H, W, 64, 7, 2, 3)]
        h, w = ((H - 1) // 2 + 1 - 1) // 2 + 1, ((W - 1) // 2 + 1 - 1) // 2 + 1
        c = 64
        for bi, layers in enumerate((6, 12, 32, 32)):
            for i in range(layers):
                units += [conv(N, pad64(c + 32 * i), h, w, 128), c3(N, 128, h, w, 64)]
            c += 32 * layers
            if bi < 3:
                units.append(conv(N, c, h, w, c // 2))
                c, h, w = c // 2, h // 2, w // 2
        return units
    if arch.startswith("vgg"):
        units, c, h, w = [conv(N, 3, H, W, 64, 3, 1, 1)], 64, H, W
        for v in (64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512):
            if v == "M":
                h, w = h // 2, w // 2
            else:
                units.append(c3(N, c, h, w, v))
                c = v
        return units
    hd = ctypes.c_void_p()
    assert lib.mmskin_backbone_create(arch.encode(), N, H, W, 1, ctypes.byref(hd)) == 0
    units = []
    try:
        for i in range(lib.mmskin_backbone_num_units(hd)):
            info, name = (ctypes.c_int64 * 12)(), ctypes.create_string_buffer(128)
            assert lib.mmskin_backbone_unit_info(hd, i, name, 128, info) == 0
            _, cout, oh, ow, cin, h, w = list(info)[3:10]
            name = name.value.decode()
            stride = 1 if oh == h else 2
            if cin == 3:                                       # the stem (7x7) or the first conv (3x3) in their virtual forms
                k = 7 if arch.startswith("resnet") else 3
                units.append(conv(N, 3, h, w, 64, k, 2, k // 2))
            elif arch.startswith("resnet"):
                k = 1 if ("downsample" in name or (arch != "resnet-18" and "conv2" not in name)) else 3
                units.append(conv(N, cin, h, w, cout, k, stride, k // 2))
            elif cin == cout and re.search(r"\.(conv|block)\.[01]\.0\.weight$", name):
                continue                                       # depthwise: its weight gradient is not a GEMM
            else:
                units.append(conv(N, pad64(cin), h, w, pad64(cout)))
    finally:
        lib.mmskin_backbone_destroy(hd)
    return units


ARCHS = ["resnet-18", "resnet-50", "densenet169", "vgg16-features", "mobilenet-v2", "efficientnet-b0", "efficientnet-b7"]
