"""-m gpu: every op-level entry point stays inside the workspace its size function reports (csrc/capi.hip: the size IS the null-base
carve of the layout the op uses, with no slack behind it).  Per op family, at the smallest shape that still takes every region of its layout:

1. one buffer of workspace_bytes + 64 KiB, the tail filled with 0xA5; the op runs on the buffer's base; the tail is still all 0xA5;
2. the same call on a workspace of twice the size (filled with another pattern) gives bit-identical outputs: extra room changes nothing,
   and nothing read from the workspace was left over from before the call.

This is a bounds check on a correctly sized buffer; the values themselves are checked by the parity tests of each family."""
import ctypes

import pytest
import torch

from gpu_util import DEV, DT
from densenet_cases import BLOCK_CASES, TRANS_CASES, block_reference, trans_reference
from mbconv_cases import BN_SHAPES, DW_CASES, SE_SHAPES, out_hw, pad64
from mmskin import _lib
from mmskin._lib import call, ptr, stream

pytestmark = pytest.mark.gpu
GUARD = 65536


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).bfloat16().float().to(DEV)


def _new(*shape):
    return torch.empty(*shape, device=DEV)


def conv_case(k, s, p, dtype):
    N, Cin, H, W, Cout = 2, 64, 8, 8, 64
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    g = torch.Generator().manual_seed(k)
    x, w, dy = _rand(g, N, Cin, H, W), _rand(g, Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5), _rand(g, N, Cout, OH, OW)
    shape = (N, Cin, H, W, Cout, k, k, s, p)

    def run(wsp):
        y, dx, dw = _new(N, Cout, OH, OW), _new(N, Cin, H, W), _new(Cout, Cin, k, k)
        call("mmskin_conv2d_forward", ptr(x), ptr(w), ptr(y), *shape, DT[dtype], ptr(wsp), stream())
        call("mmskin_conv2d_backward", ptr(dy), ptr(x), ptr(w), ptr(dx), ptr(dw), *shape, DT[dtype], ptr(wsp), stream())
        return y, dx, dw
    return _lib.load().mmskin_conv2d_workspace_bytes(*shape), run


def dgrad_fused_case():
    N, Cin, H, W, Cout, k, s, p = 2, 64, 8, 8, 64, 3, 1, 1
    g = torch.Generator().manual_seed(5)
    dy, w, xc = _rand(g, N, Cout, H, W), _rand(g, Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5), _rand(g, N, Cin, H, W)
    scale, shift = torch.rand(Cin, generator=g).to(DEV) + 0.5, _rand(g, Cin, scale=0.3)
    shape = (N, Cin, H, W, Cout, k, k, s, p)
    lib = _lib.load()
    rows = lib.mmskin_conv2d_dgrad_fused_rows(*shape)

    def run(wsp):
        dz, part, nw = _new(N, Cin, H, W), torch.zeros(rows, 2, Cin, device=DEV), ctypes.c_int(0)
        call("mmskin_conv2d_dgrad_fused", ptr(dy), ptr(w), ptr(xc), ptr(scale), ptr(shift), ptr(dz), ptr(part), ctypes.addressof(nw), *shape,
             ptr(wsp), stream())
        return dz, part[: nw.value]
    return lib.mmskin_conv2d_workspace_bytes(*shape), run


def dgrad_epilogue_case(dtype):
    import conv_epilogue_oracle as O
    import conv_route_cases as CR
    N, Cin, H, W, Cout, k, s, p = 2, 64, 8, 8, 64, 3, 1, 1
    g = torch.Generator().manual_seed(16)
    dy, w = _rand(g, N, Cout, H, W), _rand(g, Cout, Cin, k, k, scale=(Cout * k * k) ** -0.5)
    addend, mask_y, x, x2 = (_rand(g, N, Cin, H, W) for _ in range(4))
    bits = O.pack_bits(torch.rand(N, Cin, H, W, generator=g) > 0.5, dtype).to(DEV)
    shape = (N, Cin, H, W, Cout, k, k, s, p)
    flags = CR.D_ADDEND | CR.D_MASK_Y | CR.D_MASK_BITS | CR.D_X | CR.D_X2 | CR.D_PARTIAL      # every tensor operand: every region of the layout
    lib = _lib.load()
    rows = lib.mmskin_conv2d_dgrad_fused_rows(*shape)

    def run(wsp):
        dz, part, part_b, nw = _new(N, Cin, H, W), torch.zeros(rows, 2, Cin, device=DEV), torch.zeros(rows, 2, Cin, device=DEV), ctypes.c_int(0)
        call("mmskin_conv2d_dgrad_epilogue", ptr(dy), ptr(w), ptr(addend), ptr(mask_y), ptr(bits), ptr(x), None, None, ptr(x2), ptr(dz), ptr(part), ptr(part_b),
             ctypes.addressof(nw), *shape, flags, DT[dtype], ptr(wsp), stream())
        return dz, part[: nw.value], part_b[: nw.value]
    return lib.mmskin_conv2d_dgrad_epilogue_workspace_bytes(*shape), run


def forward_epilogue_case(dtype):
    import conv_epilogue_oracle as O
    import conv_route_cases as CR
    N, Cin, H, W, Cout, k, s, p = 2, 64, 8, 8, 64, 3, 1, 1
    g = torch.Generator().manual_seed(17)
    x, w, addend = _rand(g, N, Cin, H, W), _rand(g, Cout, Cin, k, k, scale=(Cin * k * k) ** -0.5), _rand(g, N, Cout, H, W)
    mul, bias = torch.rand(Cout, generator=g).to(DEV) + 0.5, _rand(g, Cout, scale=0.3)
    shape = (N, Cin, H, W, Cout, k, k, s, p)
    flags = CR.MUL | CR.BIAS | CR.ADDEND | CR.RELU | CR.MASK_OUT | CR.STATS
    lib = _lib.load()
    rows = lib.mmskin_conv2d_forward_epilogue_stat_rows(*shape)

    def run(wsp):
        y, ssum, ssq, nw = _new(N, Cout, H, W), torch.zeros(rows, Cout, device=DEV), torch.zeros(rows, Cout, device=DEV), ctypes.c_int(0)
        mask = torch.zeros(O.mask_bytes(N * H * W, Cout, dtype) // 4 * 4, dtype=torch.uint8, device=DEV)
        call("mmskin_conv2d_forward_epilogue", ptr(x), ptr(w), ptr(mul), ptr(bias), ptr(addend), ptr(y), ptr(ssum), ptr(ssq), ctypes.addressof(nw), ptr(mask),
             *shape, flags, DT[dtype], ptr(wsp), stream())
        return y, ssum[: nw.value], ssq[: nw.value], mask
    return lib.mmskin_conv2d_forward_epilogue_workspace_bytes(*shape), run


def batchnorm_case(dtype):
    N, C, H, W = 2, 64, 8, 8
    g = torch.Generator().manual_seed(6)
    x, dy = _rand(g, N, C, H, W, scale=2.0), _rand(g, N, C, H, W)
    gamma, beta = torch.rand(C, generator=g).to(DEV) + 0.5, _rand(g, C, scale=0.3)

    def run(wsp):
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        y, sm, si, dx, dg, db = _new(N, C, H, W), _new(C), _new(C), _new(N, C, H, W), _new(C), _new(C)
        call("mmskin_batchnorm_forward", ptr(x), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(y), ptr(sm), ptr(si), N, C, H, W, 1e-5, 0.1, 1,
             DT[dtype], ptr(wsp), stream())
        call("mmskin_batchnorm_backward", ptr(dy), ptr(x), ptr(gamma), ptr(beta), ptr(sm), ptr(si), ptr(dx), ptr(dg), ptr(db), N, C, H, W, 1,
             DT[dtype], ptr(wsp), stream())
        return y, sm, si, rm, rv, dx, dg, db
    return _lib.load().mmskin_batchnorm_workspace_bytes(N, C, H, W), run


def abn_case(entry):
    N, Cw, C4, H, W = 2, 64, 256, 14, 14                     # the smallest case of tests/test_gpu_abn.py
    g = torch.Generator().manual_seed(7)
    y, gr, w = torch.relu(_rand(g, N, Cw, H, W)), _rand(g, N, C4, H, W), _rand(g, C4, Cw, scale=Cw ** -0.5)
    cA, cB, cC = torch.rand(C4, generator=g).to(DEV) + 0.5, _rand(g, C4, scale=0.05), _rand(g, C4, scale=0.02)

    def run(wsp):
        if entry == "mmskin_conv1x1_gram_stats":
            ssum, ssq = _new(C4), _new(C4)
            call(entry, ptr(y), ptr(w), N, Cw, C4, H, W, ptr(ssum), ptr(ssq), ptr(wsp), stream())
            return ssum, ssq
        dy, dw = _new(N, Cw, H, W), _new(C4, Cw)
        call(entry, ptr(gr), ptr(y), ptr(w), ptr(cA), ptr(cB), ptr(cC), N, Cw, C4, H, W, ptr(dy), ptr(dw), ptr(wsp), stream())
        return dy, dw
    return _lib.load().mmskin_abn_workspace_bytes(N, Cw, C4, H, W), run


def stem_case(dtype):
    N, H, W = 2, 32, 32
    g = torch.Generator().manual_seed(8)
    x, w, dy = _rand(g, N, 3, H, W), _rand(g, 64, 3, 7, 7, scale=147 ** -0.5), _rand(g, N, 64, 8, 8)
    gamma, beta = torch.rand(64, generator=g).to(DEV) + 0.5, _rand(g, 64, scale=0.2)

    def run(wsp):
        y, dw, dg, db = _new(N, 64, 8, 8), _new(64, 3, 7, 7), _new(64), _new(64)
        call("mmskin_stem_forward", ptr(x), ptr(w), ptr(gamma), ptr(beta), ptr(y), N, H, W, 1e-5, DT[dtype], ptr(wsp), stream())
        call("mmskin_stem_backward", ptr(dy), ptr(x), ptr(w), ptr(gamma), ptr(beta), ptr(dw), ptr(dg), ptr(db), N, H, W, 1e-5, DT[dtype],
             ptr(wsp), stream())
        return y, dw, dg, db
    return _lib.load().mmskin_stem_workspace_bytes(N, H, W), run


def depthwise_case(dtype):
    c = min(DW_CASES, key=lambda c: (c.N * c.C * c.H * c.W, c.ksize, c.stride))
    OH, OW = out_hw(c.H, c.W, c.ksize, c.stride)
    g = torch.Generator().manual_seed(9)
    x, w, dy = _rand(g, c.N, c.C, c.H, c.W), _rand(g, c.c_valid, 1, c.ksize, c.ksize, scale=0.3), _rand(g, c.N, c.C, OH, OW)
    shape = (c.N, c.C, c.H, c.W, c.ksize, c.stride)

    def run(wsp):
        y, dx, dw = _new(c.N, c.C, OH, OW), _new(c.N, c.C, c.H, c.W), _new(c.c_valid, 1, c.ksize, c.ksize)
        call("mmskin_dwconv2d_forward", ptr(x), ptr(w), ptr(y), *shape, c.c_valid, DT[dtype], ptr(wsp), stream())
        call("mmskin_dwconv2d_backward", ptr(dy), ptr(x), ptr(w), ptr(dx), ptr(dw), *shape, c.c_valid, DT[dtype], ptr(wsp), stream())
        return y, dx, dw
    return _lib.load().mmskin_dwconv2d_workspace_bytes(*shape), run


def batchnorm_act_case(dtype):
    N, C, H, W = min(BN_SHAPES, key=lambda s: s[0] * s[1] * s[2] * s[3])
    g = torch.Generator().manual_seed(10)
    x, res, dy = _rand(g, N, C, H, W), _rand(g, N, C, H, W, scale=0.5), _rand(g, N, C, H, W)
    gamma, beta = torch.full((C,), 3.0, device=DEV), torch.full((C,), 3.0, device=DEV)

    def run(wsp):   # ReLU6 behind a residual: the one combination that takes the residual and the residual-gradient regions too
        rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
        y, sm, si, dx, dres, dg, db = _new(N, C, H, W), _new(C), _new(C), _new(N, C, H, W), _new(N, C, H, W), _new(C), _new(C)
        call("mmskin_batchnorm_act_forward", ptr(x), ptr(res), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(y), ptr(sm), ptr(si), N, C, H, W,
             1e-3, 0.01, 2, DT[dtype], ptr(wsp), stream())
        call("mmskin_batchnorm_act_backward", ptr(dy), ptr(x), ptr(y), ptr(gamma), ptr(beta), ptr(sm), ptr(si), ptr(dx), ptr(dres), ptr(dg),
             ptr(db), N, C, H, W, 2, 1, DT[dtype], ptr(wsp), stream())
        return y, sm, si, rm, rv, dx, dres, dg, db
    return _lib.load().mmskin_batchnorm_act_workspace_bytes(N, C, H, W), run


def se_case(dtype):
    N, C, Csq, HW = min(SE_SHAPES, key=lambda s: s[0] * s[1] * s[3])
    Cp = pad64(C)
    g = torch.Generator().manual_seed(11)
    y = torch.zeros(N, Cp, HW, device=DEV)
    y[:, :C] = _rand(g, N, C, HW)
    dyse = _rand(g, N, Cp, HW)
    w1, b1, w2, b2 = _rand(g, Csq, C, scale=C ** -0.5), _rand(g, Csq, scale=0.3), _rand(g, C, Csq, scale=Csq ** -0.5), _rand(g, C, scale=0.3)

    def run(wsp):
        yse, dyo, dw1, db1, dw2, db2 = _new(N, Cp, HW), _new(N, Cp, HW), _new(Csq, C), _new(Csq), _new(C, Csq), _new(C)
        call("mmskin_se_forward", ptr(y), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(yse), N, C, Cp, Csq, HW, DT[dtype], ptr(wsp), stream())
        call("mmskin_se_backward", ptr(dyse), ptr(y), ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(dyo), ptr(dw1), ptr(db1), ptr(dw2), ptr(db2),
             N, C, Cp, Csq, HW, DT[dtype], ptr(wsp), stream())
        return yse, dyo, dw1, db1, dw2, db2
    return _lib.load().mmskin_se_workspace_bytes(N, Cp, Csq, HW), run


def stochastic_depth_case(dtype):
    N, per = 4, 256
    g = torch.Generator().manual_seed(12)
    branch, res, dy = _rand(g, N, per), _rand(g, N, per), _rand(g, N, per)
    mask = torch.tensor([1.25, 0.0, 1.25, 0.0], device=DEV)

    def run(wsp):
        y, out = _new(N, per), _new(N, per)
        call("mmskin_sd_forward", ptr(branch), ptr(res), ptr(mask), ptr(y), N, per, DT[dtype], ptr(wsp), stream())
        call("mmskin_sd_backward", ptr(dy), ptr(mask), ptr(out), N, per, DT[dtype], ptr(wsp), stream())
        return y, out
    return _lib.load().mmskin_sd_workspace_bytes(N, per), run


def dense_block_case(dtype):
    c = BLOCK_CASES[0]                                        # the row with a padded layer: every region of the layout, two operand parities
    r = block_reference(c)
    x, dcat, params = r["x"].to(DEV), r["dcat"].to(DEV), r["params"].to(DEV)
    ctot = c.C0 + 32 * c.L
    nbuf = sum(2 * (c.C0 + 32 * i) + 256 for i in range(c.L))
    shape = (c.N, c.C0, c.L, c.H, c.W)

    def run(wsp):
        bufs = torch.ones(nbuf, device=DEV)
        cat, table, dx, grads = _new(c.N, ctot, c.H, c.W), _new(2 * ctot), _new(c.N, c.C0, c.H, c.W), _new(params.numel())
        call("mmskin_dense_block_forward", ptr(x), ptr(params), ptr(bufs), ptr(cat), ptr(table), *shape, 1, DT[dtype], ptr(wsp), stream())
        call("mmskin_dense_block_backward", ptr(dcat), ptr(x), ptr(params), ptr(dx), ptr(grads), *shape, DT[dtype], ptr(wsp), stream())
        return cat, table, bufs, dx, grads
    return _lib.load().mmskin_dense_block_workspace_bytes(*shape), run


def dense_transition_case(dtype):
    c = TRANS_CASES[0]                                        # odd map, destination wider than C/2
    r = trans_reference(c)
    x, dnext, params, table = (r[k].to(DEV) for k in ("x", "dnext", "params", "table"))
    shape = (c.N, c.C, c.H, c.W, c.pitch)

    def run(wsp):
        bufs = torch.ones(2 * c.C, device=DEV)
        dst = torch.full((c.N, c.pitch, c.H // 2, c.W // 2), -3.0, device=DEV)
        conv, dx, grads = _new(c.N, c.C // 2, c.H, c.W), _new(c.N, c.C, c.H, c.W), _new(params.numel())
        call("mmskin_dense_transition_forward", ptr(x), ptr(table), ptr(params), ptr(bufs), ptr(dst), ptr(conv), *shape, 1, DT[dtype], ptr(wsp), stream())
        call("mmskin_dense_transition_backward", ptr(dnext), ptr(x), ptr(table), ptr(params), ptr(dx), ptr(grads), None, *shape, DT[dtype], ptr(wsp), stream())
        return dst, conv, bufs, dx, grads
    return _lib.load().mmskin_dense_transition_workspace_bytes(*shape), run


def slice_stats_case(dtype):
    rows, pitch, c0, C = 70, 160, 32, 64
    g = torch.Generator().manual_seed(13)
    x = _rand(g, rows, pitch)

    def run(wsp):
        mean, var = _new(C), _new(C)
        call("mmskin_slice_stats", ptr(x), rows, pitch, c0, C, ptr(mean), ptr(var), DT[dtype], ptr(wsp), stream())
        return mean, var
    return _lib.load().mmskin_slice_stats_workspace_bytes(rows, pitch, c0, C), run


def maxpool_case(dtype):
    N, C, H, W = 1, 64, 7, 5
    g = torch.Generator().manual_seed(14)
    y, dpool = torch.relu(_rand(g, N, C, H, W)), _rand(g, N, C, H // 2, W // 2)

    def run(wsp):
        pooled, dz = _new(N, C, H // 2, W // 2), _new(N, C, H, W)
        idx = torch.empty(N, H // 2, W // 2, C, dtype=torch.uint8, device=DEV)
        call("mmskin_maxpool2_relu_forward", ptr(y), ptr(pooled), ptr(idx), N, C, H, W, DT[dtype], ptr(wsp), stream())
        call("mmskin_maxpool2_relu_backward", ptr(dpool), ptr(y), ptr(dz), N, C, H, W, DT[dtype], ptr(wsp), stream())
        return pooled, dz
    return _lib.load().mmskin_maxpool2_relu_workspace_bytes(N, C, H, W), run


def adaptive_case(dtype):
    N, C, H, W = 1, 24, 10, 9
    g = torch.Generator().manual_seed(15)
    x, dout = _rand(g, N, C, H, W), _rand(g, N, C, 7, 7)

    def run(wsp):
        out, dx = _new(N, C, 7, 7), _new(N, C, H, W)
        call("mmskin_adaptive_avgpool_forward", ptr(x), ptr(out), N, C, H, W, DT[dtype], ptr(wsp), stream())
        call("mmskin_adaptive_avgpool_backward", ptr(dout), ptr(dx), N, C, H, W, DT[dtype], ptr(wsp), stream())
        return out, dx
    return _lib.load().mmskin_adaptive_avgpool_workspace_bytes(N, C, H, W), run


BOTH = ("fp32", "bf16")
CASES = (
    [(f"conv2d_k3s1-{d}", lambda d=d: conv_case(3, 1, 1, d)) for d in BOTH]
    + [(f"conv2d_k1s2-{d}", lambda d=d: conv_case(1, 2, 0, d)) for d in BOTH]
    + [("dgrad_fused-bf16", dgrad_fused_case)]
    + [(f"dgrad_epilogue-{d}", lambda d=d: dgrad_epilogue_case(d)) for d in BOTH]
    + [(f"forward_epilogue-{d}", lambda d=d: forward_epilogue_case(d)) for d in BOTH]
    + [(f"batchnorm-{d}", lambda d=d: batchnorm_case(d)) for d in BOTH]
    + [(f"{e[len('mmskin_'):]}-bf16", lambda e=e: abn_case(e)) for e in ("mmskin_abn_backward", "mmskin_abn_backward_kept_gram", "mmskin_conv1x1_gram_stats")]
    + [(f"stem-{d}", lambda d=d: stem_case(d)) for d in BOTH]
    + [(f"depthwise-{d}", lambda d=d: depthwise_case(d)) for d in BOTH]
    + [(f"batchnorm_act-{d}", lambda d=d: batchnorm_act_case(d)) for d in BOTH]
    + [(f"squeeze_excitation-{d}", lambda d=d: se_case(d)) for d in BOTH]
    + [(f"stochastic_depth-{d}", lambda d=d: stochastic_depth_case(d)) for d in BOTH]
    + [(f"dense_block-{d}", lambda d=d: dense_block_case(d)) for d in BOTH]
    + [(f"dense_transition-{d}", lambda d=d: dense_transition_case(d)) for d in BOTH]
    + [(f"slice_stats-{d}", lambda d=d: slice_stats_case(d)) for d in BOTH]
    + [(f"maxpool2-{d}", lambda d=d: maxpool_case(d)) for d in BOTH]
    + [(f"adaptive_avgpool-{d}", lambda d=d: adaptive_case(d)) for d in BOTH]
)


@pytest.mark.parametrize("build", [c[1] for c in CASES], ids=[c[0] for c in CASES])
def test_op_stays_inside_the_workspace_it_asks_for(build):
    size, run = build()
    assert size > 0
    exact = torch.zeros(size + GUARD, dtype=torch.uint8, device=DEV)
    exact[size:] = 0xA5
    got = [t.clone() for t in run(exact)]
    torch.cuda.synchronize()
    assert bool((exact[size:] == 0xA5).all()), "the op wrote behind the workspace its size function reports"
    roomy = torch.full((2 * size,), 0x5A, dtype=torch.uint8, device=DEV)
    again = run(roomy)
    torch.cuda.synchronize()
    assert len(got) == len(again)
    for i, (a, b) in enumerate(zip(got, again)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"output {i} depends on the room behind the workspace or on its old contents"
