"""CPU: the sizes the C ABI reports for op-level workspaces and attention scratch buffers (no device needed: every size function is
host arithmetic over the layout struct that the op itself carves, csrc/capi.hip `ws_bytes`).

* mmskin_*_scratch_floats are on the model path (mmskin/ops.py allocates exactly that many floats), so they are pinned to the integers the
  formulas returned before the layouts were written once: any change would move an allocation or an offset.
* mmskin_*_workspace_bytes serve the op-by-op tests.  They are a carve now, so there is no second formula to compare with; what can be
  checked without one: a positive multiple of the carver's 256-byte alignment, not smaller for a larger batch, and not smaller than the
  tensors the op must hold (counted here from the shapes alone, fp32 elements unless the op is bf16-only).
* mmskin_backbone_create needs no device either: the carve-up of every plan (workspace bytes, parameter and buffer counts, and the
  twelve unit_info fields of the first and last unit where a plan reports units) is pinned to the values of commit a9b9008, before the
  stem geometry and the side-stream slots were each written once; the DynamicCNN rows to those of commit 4961f46, before the 3-channel
  first conv's geometry and the stage-table append were each written once."""
import ctypes

import pytest

from densenet_cases import ADAPTIVE_CASES, BLOCK_CASES, MAXPOOL_CASES, SLICE_CASES, TRANS_CASES
from mbconv_cases import BN_SHAPES, DW_CASES, SE_SHAPES, out_hw, pad64
from mmskin import _lib

# ---- scratch floats: values of commit 3050f3f ("Test the MBConv kernels op by op"), evaluated from its library
# (B, H, W, Ch): every (stage, head width) of models/hip_coat.py COAT_CONFIGS at 224 x 224, batch 2, plus one tiny shape -> (forward, backward)
FACTOR_ATTENTION = {
    (2, 56, 56, 8): (32000, 346624), (2, 56, 56, 16): (115200, 746496), (2, 28, 28, 16): (32256, 196352),
    (2, 28, 28, 32): (121856, 458240), (2, 14, 14, 32): (34816, 140800), (2, 14, 14, 40): (53760, 191360),
    (2, 7, 7, 40): (26880, 84480), (2, 7, 7, 64): (67584, 184320), (1, 3, 5, 8): (640, 4352),
}
# (N, H, W, C): the two convolutional stages of models/hip_caformer.py CAFORMER_CONFIGS (C = 2 * dim) at 224 x 224, batch 2, plus one tiny shape
DW7_STAR = {
    (2, 56, 56, 128): 351456, (2, 28, 28, 256): 200832, (2, 56, 56, 192): 527184, (2, 28, 28, 384): 301248,
    (2, 56, 56, 256): 702912, (2, 28, 28, 512): 401664, (1, 5, 3, 4): 198,
}
# (B, G, N): the four stages of models/hip_davit.py DAVIT_CONFIGS at 224 x 224, batch 2 (one chunk from stage 3 on: no scratch), plus two
# tiny shapes either side of the chunk size
CHANNEL_ATTENTION = {(2, 3, 3136): 79872, (2, 6, 784): 49152, (2, 12, 196): 0, (2, 24, 49): 0, (1, 1, 257): 2048, (1, 1, 5): 0}


def test_scratch_floats_are_what_the_model_path_allocated_before():
    lib = _lib.load()
    for shape, (fwd, bwd) in FACTOR_ATTENTION.items():
        assert lib.mmskin_factor_attention_scratch_floats(*shape, 0) == fwd, shape
        assert lib.mmskin_factor_attention_scratch_floats(*shape, 1) == bwd, shape
    for shape, n in DW7_STAR.items():
        assert lib.mmskin_dw7_star_scratch_floats(*shape) == n, shape
    for shape, n in CHANNEL_ATTENTION.items():
        assert lib.mmskin_channel_attention_scratch_floats(*shape) == n, shape


# ---- workspace bytes on the shapes of the GPU tests.  Every row: (size function, arguments with N first, lower bound in bytes)
def _conv(N, Cin, H, W, Cout, k, s, p):
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    # NHWC input and its gradient, NHWC output (or dy), the staged forward and data-gradient weights
    return "mmskin_conv2d_workspace_bytes", (N, Cin, H, W, Cout, k, k, s, p), 4 * (2 * N * H * W * Cin + N * OH * OW * Cout + 2 * Cout * Cin * k * k)


def _dgrad_epilogue(N, Cin, H, W, Cout, k, s, p):
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    # NHWC dy; dz, addend, mask_y, x, x2 of the input's size; the staged forward and data-gradient weights
    return "mmskin_conv2d_dgrad_epilogue_workspace_bytes", (N, Cin, H, W, Cout, k, k, s, p), 4 * (5 * N * H * W * Cin + N * OH * OW * Cout + 2 * Cout * Cin * k * k)


def _forward_epilogue(N, Cin, H, W, Cout, k, s, p):
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    # NHWC input, output and addend; the staged weight
    return "mmskin_conv2d_forward_epilogue_workspace_bytes", (N, Cin, H, W, Cout, k, k, s, p), 4 * (N * H * W * Cin + 2 * N * OH * OW * Cout + Cout * Cin * k * k)


def _bn(N, C, H, W):
    return "mmskin_batchnorm_workspace_bytes", (N, C, H, W), 4 * 3 * N * C * H * W                # x, y or dy, dx


def _abn(N, Cw, C4, H, W):
    M = N * H * W                                                                                 # bf16 g, y, dy and [W | Q]; fp32 S = g^T y
    return "mmskin_abn_workspace_bytes", (N, Cw, C4, H, W), 2 * (M * C4 + 2 * M * Cw + Cw * (C4 + Cw)) + 4 * C4 * Cw


def _stem(N, H, W):
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    # the image padded to four channels, the conv output and two gradients of its size, the pooled map and its gradient
    return "mmskin_stem_workspace_bytes", (N, H, W), 4 * (4 * N * H * W + 3 * N * OH * OW * 64 + 2 * N * PH * PW * 64)


def _dw(N, C, H, W, k, s):
    OH, OW = out_hw(H, W, k, s)
    return "mmskin_dwconv2d_workspace_bytes", (N, C, H, W, k, s), 4 * (2 * N * H * W * C + N * OH * OW * C + k * k * C)


def _bn_act(N, C, H, W):
    return "mmskin_batchnorm_act_workspace_bytes", (N, C, H, W), 4 * 6 * N * C * H * W           # x, y, residual and their three gradients


def _se(N, C, Csq, HW):
    Cp = pad64(C)
    return "mmskin_se_workspace_bytes", (N, Cp, Csq, HW), 4 * (4 * N * HW * Cp + 2 * Csq * Cp)    # y, y_se, two gradients; both padded weights


def _sd(N, per):
    return "mmskin_sd_workspace_bytes", (N, per), 4 * 3 * N * per                                 # branch, residual, result


def _dense_block(c):
    rows, ctot = c.N * c.H * c.W, c.C0 + 32 * c.L
    acts = sum(pad64(c.C0 + 32 * i) + 2 * 128 for i in range(c.L))                                # t, a, u of every layer
    weights = sum(128 * pad64(c.C0 + 32 * i) + 64 * 128 * 9 for i in range(c.L))                  # staged forward and data-gradient copies
    return "mmskin_dense_block_workspace_bytes", (c.N, c.C0, c.L, c.H, c.W), 4 * (rows * (2 * ctot + acts) + 2 * weights)


def _dense_transition(c):
    rows, prows = c.N * c.H * c.W, c.N * (c.H // 2) * (c.W // 2)
    # x, its gradient, relu(norm(x)) and the data gradient; the conv output; the destination rows; both staged weights
    return "mmskin_dense_transition_workspace_bytes", (c.N, c.C, c.H, c.W, c.pitch), 4 * (4 * rows * c.C + rows * c.C // 2 + prows * c.pitch + c.C * c.C)


def _slice_stats(c):
    return "mmskin_slice_stats_workspace_bytes", (c.rows, c.pitch, c.c0, c.C), 4 * c.rows * c.pitch


def _maxpool(N, C, H, W):
    prows = N * (H // 2) * (W // 2)
    return "mmskin_maxpool2_relu_workspace_bytes", (N, C, H, W), 4 * (2 * N * H * W * C + 2 * prows * C) + prows * C   # y, dz, pooled, dpool; argmax bytes


def _adaptive(N, C, H, W):
    return "mmskin_adaptive_avgpool_workspace_bytes", (N, C, H, W), 4 * 2 * N * H * W * C          # x, dx


ROWS = (
    # tests/test_gpu_kernels.py CONV_CASES, the two shapes of tests/test_gpu_workspace_bounds.py and the rejected 3-channel shape
    [_conv(*c) for c in [(2, 64, 14, 14, 64, 1, 1, 0), (2, 64, 14, 14, 256, 1, 1, 0), (2, 256, 9, 11, 128, 1, 1, 0), (3, 64, 12, 12, 64, 3, 1, 1),
                         (2, 128, 14, 14, 128, 3, 2, 1), (2, 128, 15, 13, 128, 3, 2, 1), (2, 256, 14, 14, 512, 1, 2, 0), (1, 512, 7, 7, 512, 3, 1, 1),
                         (2, 64, 56, 56, 64, 3, 1, 1), (3, 128, 28, 28, 64, 3, 1, 1), (5, 64, 14, 14, 128, 3, 1, 1), (2, 64, 9, 13, 64, 3, 1, 1),
                         (2, 64, 8, 8, 64, 3, 1, 1), (2, 64, 8, 8, 64, 1, 2, 0), (1, 3, 8, 8, 16, 3, 1, 1)]]
    # shapes of tests/conv_epilogue_cases.py and the one of tests/test_gpu_workspace_bounds.py
    + [f(*c) for f in (_dgrad_epilogue, _forward_epilogue)
       for c in [(2, 64, 9, 11, 128, 1, 1, 0), (2, 128, 15, 13, 128, 3, 2, 1), (2, 256, 14, 14, 512, 1, 2, 0), (2, 64, 203, 203, 64, 1, 1, 0), (2, 64, 8, 8, 64, 3, 1, 1)]]
    + [_bn(*c) for c in [(4, 64, 9, 7), (2, 2048, 3, 3), (3, 256, 14, 14), (2, 64, 8, 8)]]
    + [_abn(*c) for c in [(2, 64, 256, 14, 14), (3, 128, 512, 9, 11), (20, 64, 256, 14, 14), (6, 128, 512, 14, 14), (256, 64, 256, 56, 56)]]   # tests/test_gpu_abn.py
    + [_stem(*c) for c in [(2, 32, 32), (3, 50, 70), (3, 224, 224)]]
    + [_dw(*c) for c in sorted({(c.N, c.C, c.H, c.W, c.ksize, c.stride) for c in DW_CASES})]
    + [_bn_act(*c) for c in BN_SHAPES]
    + [_se(*c) for c in SE_SHAPES]
    + [_sd(*c) for c in [(5, 7 * 7 * 64), (4, 256)]]
    + [_dense_block(c) for c in BLOCK_CASES]
    + [_dense_transition(c) for c in TRANS_CASES]
    + [_slice_stats(c) for c in SLICE_CASES if c.dtype == "fp32"]
    + [_maxpool(*c) for c in MAXPOOL_CASES]
    + [_adaptive(*c) for c in ADAPTIVE_CASES]
)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r[0][len("mmskin_"):-len("_workspace_bytes")] + "-" + "x".join(map(str, r[1])))
def test_workspace_bytes_are_aligned_monotone_in_the_batch_and_hold_the_tensors(row):
    name, args, lower = row
    fn = getattr(_lib.load(), name)
    size = fn(*args)
    assert size > 0 and size % 256 == 0, size
    assert size >= lower, (size, lower)
    for more in (1, 2, 7):                                    # N is the first argument of every size function
        assert fn(args[0] + more, *args[1:]) >= size, (more, fn(args[0] + more, *args[1:]), size)


def test_one_abn_workspace_serves_both_entry_points():
    """mmskin_abn_workspace_bytes is documented to size mmskin_abn_backward(_kept_gram) AND mmskin_conv1x1_gram_stats: it is at least
    the latter's own tensors (bf16 y, the fp32 Gram tile rows and column sums) for every case of tests/test_gpu_abn.py."""
    lib = _lib.load()
    for N, Cw, C4, H, W in [(2, 64, 256, 14, 14), (3, 128, 512, 9, 11), (256, 64, 256, 56, 56)]:
        assert lib.mmskin_abn_workspace_bytes(N, Cw, C4, H, W) >= 2 * N * H * W * Cw + 4 * (256 * Cw + 256)


# ---- plan carve-ups: (arch, (N, H, W), dtype) -> (workspace bytes, param numel, buffer numel, units, (info12 of the first unit, of the last))
# None: not pinned -- the ResNet stem unit has no post-activation buffer (its output is the pooled map), and its y_off field was
# uninitialised memory in the library these values were recorded from.  The dynamic-cnn rows: recorded from the library of commit 4961f46
PLAN_PINS = {
    ('resnet-18', (2, 64, 64), 'fp32'): (106652672, 11176512, 9600, 20, ((89508864, None, 89507840, 2048, 64, 32, 32, 3, 64, 64, 91206656, 92384256), (91190272, 92366848, 91182080, 8, 512, 2, 2, 512, 2, 2, 91206656, 92384256))),
    ('resnet-18', (2, 64, 64), 'bf16'): (58688512, 11176512, 9600, 20, ((44763136, None, 44762112, 2048, 64, 32, 32, 3, 64, 64, 45649920, 46255104), (45641728, 46246400, 45633536, 8, 512, 2, 2, 512, 2, 2, 45649920, 46255104))),
    ('resnet-18', (3, 96, 128), 'fp32'): (129973248, 11176512, 9600, 20, ((90079232, None, 90078208, 9216, 64, 48, 64, 3, 96, 128, 97454080, 102753280), (97380352, 102674944, 97372160, 36, 512, 3, 4, 512, 3, 4, 97454080, 102753280))),
    ('resnet-18', (3, 96, 128), 'bf16'): (70488064, 11176512, 9600, 20, ((45076992, None, 45075968, 9216, 64, 48, 64, 3, 96, 128, 48802304, 51525632), (48765440, 51486464, 48757248, 36, 512, 3, 4, 512, 3, 4, 48802304, 51525632))),
    ('resnet-50', (2, 64, 64), 'fp32'): (219206656, 23508032, 53120, 53, ((187829248, None, 187828224, 2048, 64, 32, 32, 3, 64, 64, 195511296, 201651200), (195445760, 201581568, 195412992, 8, 2048, 2, 2, 512, 2, 2, 195511296, 201651200))),
    ('resnet-50', (2, 64, 64), 'bf16'): (118606848, 23508032, 53120, 53, ((93931520, None, 93930496, 2048, 64, 32, 32, 3, 64, 64, 97984512, 101070848), (97951744, 101036032, 97918976, 8, 2048, 2, 2, 512, 2, 2, 97984512, 101070848))),
    ('resnet-50', (3, 96, 128), 'fp32'): (279924736, 23508032, 53120, 53, ((188383232, None, 188382208, 9216, 64, 48, 64, 3, 96, 128, 221468672, 249098240), (221173760, 248784896, 221140992, 36, 2048, 3, 4, 512, 3, 4, 221468672, 249098240))),
    ('resnet-50', (3, 96, 128), 'bf16'): (149650944, 23508032, 53120, 53, ((94228992, None, 94227968, 9216, 64, 48, 64, 3, 96, 128, 110983680, 124872192), (110836224, 124715520, 110803456, 36, 2048, 3, 4, 512, 3, 4, 110983680, 124872192))),
    ('densenet169', (2, 64, 64), 'fp32'): (151677696, 12484480, 158400, 0, ()),
    ('densenet169', (2, 64, 64), 'bf16'): (79245056, 12484480, 158400, 0, ()),
    ('densenet169', (3, 96, 128), 'fp32'): (230309632, 12484480, 158400, 0, ()),
    ('densenet169', (3, 96, 128), 'bf16'): (121615616, 12484480, 158400, 0, ()),
    ('densenet169-features', (2, 64, 64), 'fp32'): (151677696, 12484480, 158400, 0, ()),
    ('densenet169-features', (2, 64, 64), 'bf16'): (79245056, 12484480, 158400, 0, ()),
    ('densenet169-features', (3, 96, 128), 'fp32'): (230309632, 12484480, 158400, 0, ()),
    ('densenet169-features', (3, 96, 128), 'bf16'): (121615616, 12484480, 158400, 0, ()),
    ('vgg16-features', (2, 64, 64), 'fp32'): (142340608, 14714688, 0, 0, ()),
    ('vgg16-features', (2, 64, 64), 'bf16'): (76325120, 14714688, 0, 0, ()),
    ('vgg16-features', (3, 96, 128), 'fp32'): (264321792, 14714688, 0, 0, ()),
    ('vgg16-features', (3, 96, 128), 'bf16'): (173257216, 14714688, 0, 0, ()),
    ('mobilenet-v2', (2, 64, 64), 'fp32'): (40450048, 2223872, 34112, 52, ((20440064, 20964352, 21488640, 2048, 32, 32, 32, 3, 64, 64, 0, 36255744), (32996864, 33037824, 33078784, 8, 1280, 2, 2, 320, 2, 2, 32980224, 36255744))),
    ('mobilenet-v2', (2, 64, 64), 'bf16'): (21978624, 2223872, 34112, 52, ((10220032, 10482176, 10744320, 2048, 32, 32, 32, 3, 64, 64, 0, 19881472), (16663552, 16684032, 16704512, 8, 1280, 2, 2, 320, 2, 2, 16652032, 19881472))),
    ('mobilenet-v2', (3, 96, 128), 'fp32'): (102373120, 2223872, 34112, 52, ((21394688, 23753984, 26113280, 9216, 32, 48, 64, 3, 96, 128, 0, 83498752), (76744448, 76928768, 77113088, 36, 1280, 3, 4, 320, 3, 4, 76691968, 83498752))),
    ('mobilenet-v2', (3, 96, 128), 'bf16'): (54544640, 2223872, 34112, 52, ((10697472, 11877120, 13056768, 9216, 32, 48, 64, 3, 96, 128, 0, 45107456), (38537472, 38629632, 38721792, 36, 1280, 3, 4, 320, 3, 4, 38508032, 45107456))),
    ('efficientnet-b0', (2, 64, 64), 'fp32'): (54398720, 4007548, 42016, 49, ((28730368, 29254656, 29778944, 2048, 32, 32, 32, 3, 64, 64, 0, 50204416), (46383104, 46424064, 46465024, 8, 1280, 2, 2, 320, 2, 2, 46366464, 50204416))),
    ('efficientnet-b0', (2, 64, 64), 'bf16'): (30691584, 4007548, 42016, 49, ((14365184, 14627328, 14889472, 2048, 32, 32, 32, 3, 64, 64, 0, 28594432), (24814080, 24834560, 24855040, 8, 1280, 2, 2, 320, 2, 2, 24802560, 28594432))),
    ('efficientnet-b0', (3, 96, 128), 'fp32'): (124082176, 4007548, 42016, 49, ((29684992, 32044288, 34403584, 9216, 32, 48, 64, 3, 96, 128, 0, 105207808), (97880320, 98064640, 98248960, 36, 1280, 3, 4, 320, 3, 4, 97827840, 105207808))),
    ('efficientnet-b0', (3, 96, 128), 'bf16'): (67201024, 4007548, 42016, 49, ((14842624, 16022272, 17201920, 9216, 32, 48, 64, 3, 96, 128, 0, 57763840), (50620672, 50712832, 50804992, 36, 1280, 3, 4, 320, 3, 4, 50591232, 57763840))),
    ('efficientnet-b7', (2, 64, 64), 'fp32'): (572389632, 63786960, 310720, 163, ((422388736, 422913024, 423437312, 2048, 64, 32, 32, 3, 64, 64, 0, 566098176), (546476544, 546558464, 546640384, 8, 2560, 2, 2, 640, 2, 2, 546443264, 566098176))),
    ('efficientnet-b7', (2, 64, 64), 'bf16'): (322325248, 63786960, 310720, 163, ((211194368, 211456512, 211718656, 2048, 64, 32, 32, 3, 64, 64, 0, 319179520), (299639808, 299680768, 299721728, 8, 2560, 2, 2, 640, 2, 2, 299616768, 319179520))),
    ('efficientnet-b7', (3, 96, 128), 'fp32'): (847353856, 63786960, 310720, 163, ((423343360, 425702656, 428061952, 9216, 64, 48, 64, 3, 96, 128, 0, 819042304), (797800192, 798168832, 798537472, 36, 2560, 3, 4, 640, 3, 4, 797695232, 819042304))),
    ('efficientnet-b7', (3, 96, 128), 'bf16'): (460767232, 63786960, 310720, 163, ((211671808, 212851456, 214031104, 9216, 64, 48, 64, 3, 96, 128, 0, 446611456), (425737984, 425922304, 426106624, 36, 2560, 3, 4, 640, 3, 4, 425679104, 446611456))),
    ('dynamic-cnn/64/l1/p0/k3', (2, 64, 64), 'fp32'): (10994688, 1856, 0, 0, ()),
    ('dynamic-cnn/64/l1/p0/k3', (2, 64, 64), 'bf16'): (7688960, 1856, 0, 0, ()),
    ('dynamic-cnn/64/l1/p0/k3', (3, 96, 128), 'fp32'): (41354496, 1856, 0, 0, ()),
    ('dynamic-cnn/64/l1/p0/k3', (3, 96, 128), 'bf16'): (26561536, 1856, 0, 0, ()),
    ('dynamic-cnn/64/l1/p0/k3/t0', (2, 64, 64), 'fp32'): (13091840, 1856, 0, 0, ()),
    ('dynamic-cnn/64/l1/p0/k3/t0', (2, 64, 64), 'bf16'): (8737536, 1856, 0, 0, ()),
    ('dynamic-cnn/64/l1/p0/k3/t0', (3, 96, 128), 'fp32'): (50791680, 1856, 0, 0, ()),
    ('dynamic-cnn/64/l1/p0/k3/t0', (3, 96, 128), 'bf16'): (31280128, 1856, 0, 0, ()),
    ('dynamic-cnn/64-128/l2/p1/k3', (2, 64, 64), 'fp32'): (26429184, 260544, 0, 0, ()),
    ('dynamic-cnn/64-128/l2/p1/k3', (2, 64, 64), 'bf16'): (18159104, 260544, 0, 0, ()),
    ('dynamic-cnn/64-128/l2/p1/k3', (3, 96, 128), 'fp32'): (148244480, 260544, 0, 0, ()),
    ('dynamic-cnn/64-128/l2/p1/k3', (3, 96, 128), 'bf16'): (114724608, 260544, 0, 0, ()),
    ('dynamic-cnn/64-128-256/l2/p1/k3', (2, 64, 64), 'fp32'): (35670272, 1146304, 0, 0, ()),
    ('dynamic-cnn/64-128-256/l2/p1/k3', (2, 64, 64), 'bf16'): (22943744, 1146304, 0, 0, ()),
    ('dynamic-cnn/64-128-256/l2/p1/k3', (3, 96, 128), 'fp32'): (164203008, 1146304, 0, 0, ()),
    ('dynamic-cnn/64-128-256/l2/p1/k3', (3, 96, 128), 'bf16'): (123015424, 1146304, 0, 0, ()),
}


@pytest.mark.parametrize("key", list(PLAN_PINS), ids=lambda k: "%s-%s-%s" % (k[0], "x".join(map(str, k[1])), k[2]))
def test_plan_carve_is_what_it_was(key):
    arch, shape, dtype = key
    ws_bytes, params, buffers, units, infos = PLAN_PINS[key]
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.mmskin_backbone_create(arch.encode(), *shape, {"fp32": _lib.F32, "bf16": _lib.BF16}[dtype], ctypes.byref(h)))
    try:
        assert lib.mmskin_backbone_workspace_bytes(h) == ws_bytes
        assert lib.mmskin_backbone_param_numel(h) == params
        assert lib.mmskin_backbone_buffer_numel(h) == buffers
        assert lib.mmskin_backbone_num_units(h) == units
        for index, want in zip((0, units - 1), infos):
            info = (ctypes.c_int64 * 12)()
            _lib.check(lib.mmskin_backbone_unit_info(h, index, None, 0, info))
            assert [g for g, w in zip(info, want) if w is not None] == [w for w in want if w is not None], (index, list(info))
    finally:
        lib.mmskin_backbone_destroy(h)
