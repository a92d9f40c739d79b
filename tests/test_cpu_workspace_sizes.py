"""CPU: the sizes the C ABI reports for op-level workspaces and attention scratch buffers (no device needed: every size function is
host arithmetic over the layout struct that the op itself carves, csrc/capi.hip `ws_bytes`).

* mmskin_*_scratch_floats are on the model path (mmskin/ops.py allocates exactly that many floats), so they are pinned to the integers the
  formulas returned before the layouts were written once: any change would move an allocation or an offset.
* mmskin_*_workspace_bytes serve the op-by-op tests.  They are a carve now, so there is no second formula to compare with; what can be
  checked without one: a positive multiple of the carver's 256-byte alignment, not smaller for a larger batch, and not smaller than the
  tensors the op must hold (counted here from the shapes alone, fp32 elements unless the op is bf16-only)."""
import pytest

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


ROWS = (
    # tests/test_gpu_kernels.py CONV_CASES, the two shapes of tests/test_gpu_workspace_bounds.py and the rejected 3-channel shape
    [_conv(*c) for c in [(2, 64, 14, 14, 64, 1, 1, 0), (2, 64, 14, 14, 256, 1, 1, 0), (2, 256, 9, 11, 128, 1, 1, 0), (3, 64, 12, 12, 64, 3, 1, 1),
                         (2, 128, 14, 14, 128, 3, 2, 1), (2, 128, 15, 13, 128, 3, 2, 1), (2, 256, 14, 14, 512, 1, 2, 0), (1, 512, 7, 7, 512, 3, 1, 1),
                         (2, 64, 56, 56, 64, 3, 1, 1), (3, 128, 28, 28, 64, 3, 1, 1), (5, 64, 14, 14, 128, 3, 1, 1), (2, 64, 9, 13, 64, 3, 1, 1),
                         (2, 64, 8, 8, 64, 3, 1, 1), (2, 64, 8, 8, 64, 1, 2, 0), (1, 3, 8, 8, 16, 3, 1, 1)]]
    + [_bn(*c) for c in [(4, 64, 9, 7), (2, 2048, 3, 3), (3, 256, 14, 14), (2, 64, 8, 8)]]
    + [_abn(*c) for c in [(2, 64, 256, 14, 14), (3, 128, 512, 9, 11), (20, 64, 256, 14, 14), (6, 128, 512, 14, 14), (256, 64, 256, 56, 56)]]   # tests/test_gpu_abn.py
    + [_stem(*c) for c in [(2, 32, 32), (3, 50, 70), (3, 224, 224)]]
    + [_dw(*c) for c in sorted({(c.N, c.C, c.H, c.W, c.ksize, c.stride) for c in DW_CASES})]
    + [_bn_act(*c) for c in BN_SHAPES]
    + [_se(*c) for c in SE_SHAPES]
    + [_sd(*c) for c in [(5, 7 * 7 * 64), (4, 256)]]
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
