"""CPU: the reference of the op-level epilogue tests (tests/conv_epilogue_oracle.py) and their case list (tests/conv_epilogue_cases.py), before
any GPU time is spent.

(a) what the sums MEAN: through a small residual block relu(bn3(conv3(y)) + bn_d(conv_d(y0))) followed by a next conv and a skip, the oracle's
    profile-4 / profile-5 outputs are the pieces autograd needs -- dz is the gradient at the BatchNorm output, and the BatchNorm weight and
    bias gradients rebuilt from sum dz, sum dz * x (and sum dz * x2 for the downsample BatchNorm) equal autograd's to 1e-10;
(b) the mask bytes: pack / unpack round trip and byte index (row * C + col) * elem_bytes >> 4;
(c) every case is routed to the instantiation it names (mmskin_conv_route is host arithmetic), and the list covers what it claims."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import conv_epilogue_cases as E
import conv_epilogue_oracle as O
import conv_route_cases as C
from mmskin import _lib


def test_profile_4_and_5_outputs_are_the_batchnorm_backward_autograd_needs():
    g = torch.Generator().manual_seed(3)
    N, Cw, C4, Cn, H, W = 3, 8, 16, 12, 5, 7
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    y, y0 = r(N, Cw, H, W), r(N, Cw, H, W)
    w3, wd, wn = r(C4, Cw, 1, 1) / Cw ** 0.5, r(C4, Cw, 1, 1) / Cw ** 0.5, r(Cn, C4, 3, 3) / (9 * C4) ** 0.5
    g3, b3, gd, bd = (r(C4).requires_grad_(True) for _ in range(4))
    gy, gskip = r(N, Cn, H, W), r(N, C4, H, W)
    x = F.conv2d(y, w3)                                         # raw input of bn3
    x2 = F.conv2d(y0, wd)                                       # raw input of the downsample BatchNorm
    z = F.batch_norm(x, None, None, g3, b3, training=True, eps=1e-5)
    z.retain_grad()
    out = torch.relu(z + F.batch_norm(x2, None, None, gd, bd, training=True, eps=1e-5)).requires_grad_(True)
    out.retain_grad()
    ((F.conv2d(out, wn, padding=1) * gy).sum() + (out * gskip).sum()).backward()
    # the launch: data gradient of the next conv into the block output, the skip gradient as its addend, the mask from the output's bits
    shape = C.conv(N, C4, H, W, Cn, 3, 1, 1)
    bits = O.unpack_bits(O.pack_bits(out.detach() > 0, "fp32"), (N, C4, H, W), "fp32")
    dz = O.dgrad_epilogue(O.conv_dgrad(gy, wn, shape), addend=gskip, keep_bits=bits)
    assert float((dz - z.grad).abs().max()) < 1e-10
    cnt = N * H * W
    for xr, gamma, beta in ((x, g3, b3), (x2, gd, bd)):         # partial = (sum dz, sum dz x); partial_b = (sum dz, sum dz x2)
        s, q = dz.sum((0, 2, 3)), (dz * xr).sum((0, 2, 3))
        mean, var = xr.mean((0, 2, 3)), xr.var((0, 2, 3), unbiased=False)
        invstd = (var + 1e-5).rsqrt()
        assert float((s - beta.grad).abs().max()) < 1e-10
        assert float((invstd * (q - mean * s) - gamma.grad).abs().max()) < 1e-10
    assert cnt == dz[:, 0].numel()
    # the forward order: multiplier, addend, bias, ReLU is train-mode BatchNorm + residual + ReLU with scale / shift as mul / bias
    mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
    scale = g3.detach() * (var + 1e-5).rsqrt()
    res = F.batch_norm(x2, None, None, gd, bd, training=True, eps=1e-5).detach()
    got = O.fwd_epilogue(x, mul=scale, addend=res, bias=b3.detach() - mean * scale, relu=True)
    assert float((got - out.detach()).abs().max()) < 1e-10


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_mask_bytes_round_trip_and_index(dtype):
    g = torch.Generator().manual_seed(4)
    N, Cc, H, W = 2, 24, 3, 5
    keep = torch.rand(N, Cc, H, W, generator=g) > 0.5
    packed = O.pack_bits(keep, dtype)
    eb = O.ELEM_BYTES[dtype]
    assert packed.dtype == torch.uint8 and packed.numel() == O.mask_bytes(N * H * W, Cc, dtype) == N * H * W * Cc * eb // 16
    assert torch.equal(O.unpack_bits(packed, (N, Cc, H, W), dtype), keep)
    rows = O.nhwc_rows(keep)
    for row, col in ((0, 0), (1, 7), (N * H * W - 1, Cc - 1), (17, 13)):
        byte, bit = (row * Cc + col) * eb >> 4, (row * Cc + col) % (16 // eb)
        assert bool((int(packed[byte]) >> bit) & 1) == bool(rows[row, col])
    one = torch.zeros(N, Cc, H, W, dtype=torch.bool)
    one[1, 9, 2, 3] = True                                       # row (1 * 3 + 2) * 5 + 3 = 28, column 9
    p1 = O.pack_bits(one, dtype)
    idx = (28 * Cc + 9) * eb >> 4
    assert int(p1[idx]) == 1 << ((28 * Cc + 9) % (16 // eb)) and int(p1.sum()) == int(p1[idx])


ALL = E.DGRAD_CASES + E.FWD_CASES


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_case_runs_the_instantiation_it_names(case):
    got = C.route(_lib.load(), case.op, case.shape, E.EB[case.dtype], case.flags)
    assert got is not None and got[:6] == case.want, got


def test_case_list_covers_every_128_row_instantiation_of_the_residual_profiles():
    have = {(c.dtype, c.want[3], c.want[4], c.want[5]) for c in ALL if c.want[0] == C.CG_TILE128}
    want = {(dt, bn, nst, epi) for dt in E.DTYPES for bn in (64, 128) for nst in (1, 2) for epi in (1, 2, 4, 5, 7)}
    assert want <= have, sorted(want - have)
    fwd2 = {(c.dtype, c.want[3], c.want[4]) for c in E.FWD_CASES if c.want[5] == 2}   # the forward's light epilogue on its own
    assert fwd2 == {(dt, bn, nst) for dt in E.DTYPES for bn in (64, 128) for nst in (1, 2)}
    assert {(c.dtype, c.want[3]) for c in E.FWD_CASES if c.want[5] == 0} == {(dt, bn) for dt in E.DTYPES for bn in (64, 128)}
    pipe = {c.want[1:3] + (c.want[5],) for tile in C.KNOB_TILES for c in E.pipe_cases(tile)}
    assert pipe == {(bm, step, epi) for bm, step in ((256, 256), (224, 224), (224, 196)) for epi in (2, 4, 5)}


@pytest.mark.parametrize("tile", sorted(C.KNOB_TILES))
def test_pipelined_cases_run_the_pinned_tile(tile):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path[:0] = %r; import conv_epilogue_cases as E, conv_route_cases as C; from mmskin import _lib\n"
            "for c in E.pipe_cases(%r):\n    got = C.route(_lib.load(), c.op, c.shape, C.BF16, c.flags); assert got is not None and got[:6] == c.want, (c, got)\nprint('OK')")
    paths = [os.path.join(root, "tests"), os.path.join(root, "multimodal-model-skin-lesion-classifier_amd")]
    env = dict(os.environ, MMSKIN_CONV_PIPE_FORCE="1", MMSKIN_CONV_PIPE_TILE=tile)
    r = subprocess.run([sys.executable, "-c", code % (paths, tile)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr


def test_statistics_only_pass_never_routes_to_the_all_taps_kernel():
    """conv3x3_c64.hip stores its output tile unconditionally: a launch without an output (MMSKIN_CRF_NO_OUT, which
    mmskin_conv2d_forward_epilogue documents as valid) on a shape that kernel takes must stay on the 128-row tile, whose store is guarded"""
    lib = _lib.load()
    for flags, want in E.NO_OUT_C64_ROUTES:
        assert C.route(lib, C.FWD, E.NO_OUT_C64_SHAPE, C.BF16, flags) == want, (flags, want)
    for N, H in ((32, 56), (256, 56), (64, 12)):
        got = C.route(lib, C.FWD, C.conv(N, 64, H, 56, 64, 3, 1, 1), C.BF16, C.STATS | C.ROWS_FREE | C.NO_OUT)
        assert got is not None and got[0] == C.CG_TILE128, got


def test_refusals_are_arguments_the_route_or_the_entry_rejects():
    """the route-level refusals of E.REFUSALS (the ARG_CHECKs in front of conv_route_dgrad's geometry) are refused by mmskin_conv_route too"""
    lib = _lib.load()
    for name, op, shape, flags, _ in E.REFUSALS:
        if name in ("addend-s2-on-3x3", "fusion-on-in-place-1x1s2"):
            assert C.route(lib, op, shape, C.BF16, flags) is None, name
            assert C.route(lib, op, shape, C.F32, flags) is None, name
