"""CPU: the conv-GEMM route (csrc/conv_gemm.hip conv_gemm_route through mmskin_conv_route; no device needed, the route is host arithmetic).

* every row of tests/conv_route_cases.py: all nine values;
* the table names every instantiation class behind launch_route's switch, or lists it in UNREACHABLE with the reason;
* a transcription of the cascade the launchers ran before there was one route function (pipe_choose + dispatch_conv_gemm + launch_cfg's
  group_m rule + the two outer `takes`) agrees with the export on all nine values over a grid -- except the launches the contract checks
  now refuse for every family, which are enumerated by their flag pattern, and a forward without an output, which no longer goes to the
  all-taps kernel (it always stores);
* no route writes more statistics / partial rows than conv_fwd_stat_rows / conv_dgrad_partial_rows promise;
* the three knobs, each in a child process (they are read once)."""
import itertools
import os
import subprocess
import sys

import pytest

import conv_route_cases as C
import wgrad_plan_cases as W
from mmskin import _lib


def _id(r):
    return "op%d-%s-%s-%x" % (r.op, "x".join(map(str, r.shape)), "bf16" if r.eb == C.BF16 else "fp32", r.flags)


@pytest.mark.parametrize("row", C.ROWS, ids=_id)
def test_route_of_every_table_row(row):
    assert C.route(_lib.load(), row.op, row.shape, row.eb, row.flags) == row.want, row.note


def test_table_names_every_instantiation():
    want = {(eb, C.CG_TILE128, 128, 128, bn, nst, epi) for eb in (C.BF16, C.F32) for bn in (64, 128) for nst in (1, 2) for epi in (0, 1, 2, 3, 4, 5, 7)}
    want |= {(C.BF16, C.CG_TILE128, 128, 128, 128, nst, 6) for nst in (1, 2)}
    want |= {(C.BF16, C.CG_BIG256, 256, 256, 256, 2, epi) for epi in (0, 2, 6)}
    want |= {(C.BF16, C.CG_PIPE, bm, step, 256, 8, epi) for bm, step in ((256, 256), (224, 224), (224, 196)) for epi in (0, 2, 3, 4, 5, 6)}
    assert len({(c[0], c[2]) + c[4:] for c in want}) == 73           # the conv_gemm_kernel instantiations of the library
    have = {(r.eb,) + r.want[:6] for r in C.ROWS if r.want[0] not in (C.CG_C64, C.CG_STEM7)}
    assert want - have == set(C.UNREACHABLE)
    assert have <= want
    assert {r.want[0] for r in C.ROWS} == {C.CG_TILE128, C.CG_BIG256, C.CG_PIPE, C.CG_C64, C.CG_STEM7}


def _child(env, shape, flags):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path[:0] = %r; import conv_route_cases as C; from mmskin import _lib; print(C.route(_lib.load(), 0, %r, 2, %d))"
    paths = [os.path.join(root, "tests"), os.path.join(root, "multimodal-model-skin-lesion-classifier_amd")]
    r = subprocess.run([sys.executable, "-c", code % (paths, shape, flags)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return eval(r.stdout.strip())


def test_knobs_pin_the_pipelined_tile_and_the_tile_order():
    lib = _lib.load()
    assert C.route(lib, C.FWD, C.KNOB_SHAPE, C.BF16)[0] == C.CG_TILE128          # 3 tiles: not the pipelined family without the knob
    for tile, (bm, step, blocks) in C.KNOB_TILES.items():
        got = _child(dict(MMSKIN_CONV_PIPE_FORCE="1", MMSKIN_CONV_PIPE_TILE=tile), C.KNOB_SHAPE, 0)
        assert got == (C.CG_PIPE, bm, step, 256, 8, 0, 0, blocks, 1), (tile, got)
    grouped = C.linear(C.BEIT_M, 1024, 4096)
    assert C.route(lib, C.FWD, grouped, C.BF16, C.BIAS | C.GELU)[6] == 8
    assert _child(dict(MMSKIN_GEMM_GROUP_M="0"), grouped, C.BIAS | C.GELU)[6] == 0


def test_transformer_residual_without_an_fp32_output_is_refused_by_every_family():
    """Before the contract checks stood in front of routing, a K > 8192 Linear with gamma / residual but no out_f32 went to the 256 x 256
    two-stage kernel unchecked (its epilogue 6 writes through out_f32)."""
    lib = _lib.load()
    for shape in (C.linear(14400, 8256, 1024), C.linear(C.BEIT_M, 4096, 1024), C.linear(1024, 1024, 384)):
        assert C.route(lib, C.FWD, shape, C.BF16, C.RESIDUAL | C.BIAS) is None
        assert b"transformer-residual" in lib.mmskin_last_error()
        assert C.route(lib, C.FWD, shape, C.BF16, C.TR) is not None
    assert C.route(lib, C.FWD, C.linear(1024, 1024, 384), C.F32, C.TR) is None            # a bf16-operand feature
    assert C.route(lib, C.FWD, C.linear(1024, 1024, 320), C.BF16, C.TR) is None           # Cout % 128
    assert C.route(lib, C.FWD, C.linear(1024, 1024, 100), C.BF16) is None                 # Cout % 64
    assert C.route(lib, C.FWD, C.linear(1024, 1000, 128), C.F32) is None                  # K % 32


# ---- the cascade as the launchers ran it before conv_gemm_route (transcribed from the parent's conv_gemm.hip, conv3x3_c64.hip, stem7x7.hip)
def _cd(a, b):
    return -(-a // b)


def _old_c64_takes(shape, eb):
    N, Cin, H, W, Cout, k, stride, pad = shape
    return eb == 2 and Cin == 64 and Cout == 64 and k == 3 and stride == 1 and pad == 1 and W == 56 and H % 4 == 0 and H >= 8 and N >= 32


def _old_dispatch(eb, a):
    """a: the ConvGemmArgs fields dispatch_conv_gemm read, operands as booleans, cls = [(rows, ntaps)]"""
    epc, bk = 16 // eb, 128 // eb
    if a["Cout"] % 64 or a["C"] % epc or any((nt * a["C"]) % bk for _, nt in a["cls"]):
        return None
    g = lambda k: a.get(k, 0)
    tr = bool(g("residual"))
    epi = bool(g("addend") or g("mask_y") or g("mask_bits") or g("x") or g("bias") or g("relu") or g("out_f32") or g("mul") or g("mask_out") or tr)
    bn_sel = 128 if a["Cout"] % 128 == 0 else 64
    heavy = bool(g("mask_y") or g("mask_bits") or g("x"))
    prof = 1
    if heavy and not g("mask_y") and not g("relu"):
        if g("x") and not g("addend") and not g("mask_bits") and not g("x2"): prof = 3
        elif not g("bias") and g("x") and g("mask_bits") and not g("scale"): prof = 5 if g("x2") else 4
        elif not g("bias") and not g("x") and not g("x2") and g("mask_bits") and not g("scale"): prof = 7
    ncls, total128 = len(a["cls"]), sum(_cd(r, 128) for r, _ in a["cls"])
    linear = a["IH"] == 1 and a["IW"] == 1 and ncls == 1

    def group_m(total, nblk):
        return 8 if (linear and nblk >= 4 and a["Cout"] * a["wrow"] * eb > (2 << 20) and total >= 16) else 0

    def pipe_choose():
        if (not a["pipe_ok"] or g("in2") or g("addend_sub") or prof == 7 or g("mask_out") or g("mul") or not a["out"] or a["in_bytes"] == 0 or
                a["in_bytes"] > 0xE0000000 or (heavy and prof == 1) or a["Cout"] % 256 or a["C"] % 64 or ncls < 1):
            return None
        if tr and (heavy or g("addend") or g("stat_sum") or not g("out_f32")):
            return None
        ksum = rsum = 0
        for rows, nt in a["cls"]:
            nk = nt * a["C"] // 64
            if nk < 1 or nk > 128:
                return None
            ksum += rows * nk * 64
            rsum += rows
        if rsum <= 0:
            return None
        best, best_tiles, pick = 1e30, 0, None
        for bm, step in ((256, 256), (224, 224), (224, 196)):
            tiles = sum(_cd(rows, step) for rows, _ in a["cls"]) * (a["Cout"] // 256)
            cost = _cd(tiles, 256) * bm
            if cost < best:
                best, best_tiles, pick = cost, tiles, (bm, step)
        mink = 768 if linear else 1024
        return pick if (ksum / rsum >= mink and best_tiles >= 192) else None

    if eb == 2:
        pc = pipe_choose()
        if pc:
            total, nblk = sum(_cd(r, pc[1]) for r, _ in a["cls"]), a["Cout"] // 256
            e = 6 if tr else (0 if not epi else (2 if not heavy else prof))
            return (C.CG_PIPE, pc[0], pc[1], 256, 8, e, group_m(total, nblk), total, nblk)
        if (a["out"] and not g("mask_out") and not g("mul") and a["wrow"] >= 2048 and ncls == 1 and not heavy and not g("stat_sum") and not g("addend") and
                a["Cout"] % 256 == 0 and g("relu") != 2 and a["cls"][0][1] == 1 and a["Sy"] == 1 and a["Sx"] == 1 and a["OS"] == 1):
            mb, nb = _cd(a["cls"][0][0], 256), a["Cout"] // 256
            if mb * nb >= 224:
                return (C.CG_BIG256, 256, 256, 256, 2, 0 if not epi else (6 if tr else 2), group_m(mb, nb), mb, nb)
    one = total128 * (a["Cout"] // bn_sel) > (800 if (heavy and prof == 1) else 640)
    nst = 1 if one else 2
    if tr:
        if heavy or g("addend") or g("stat_sum") or not g("out_f32") or a["Cout"] % 128 or eb != 2:
            return None
        return (C.CG_TILE128, 128, 128, 128, nst, 6, group_m(total128, a["Cout"] // 128), total128, a["Cout"] // 128)
    e = 0 if not epi else (2 if not heavy else prof)
    return (C.CG_TILE128, 128, 128, bn_sel, nst, e, group_m(total128, a["Cout"] // bn_sel), total128, a["Cout"] // bn_sel)


def _old_route(op, shape, eb, flags, c64_needs_out=False):
    N, Cin, H, W, Cout, k, stride, pad = shape
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    f = lambda bit: bool(flags & bit)
    if op == C.STEM:
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        Hp, Wp = max(2 * OH + 8, H + 6), (max(2 * OW + 8, W + 6) + 1) // 2 * 2
        if eb == 2 and OW == 112 and OH % 4 == 0 and Hp >= 2 * OH + 5 and Wp >= 2 * OW + 8 and 13 * Wp * 8 <= 7 * 256 * 16 and 13 * Wp * 8 + 7 * 4096 + 4 * 16 * 144 <= 80 * 1024:
            return (C.CG_STEM7, 0, 0, 0, 0, 0, 0, N * (OH // 4), 1)
        return _old_dispatch(eb, dict(Cout=64, C=32, wrow=256, IH=Hp, IW=Wp // 2, Sy=2, Sx=1, OS=1, cls=[(N * OH * OW, 8)], in_bytes=0, pipe_ok=0, out=1, stat_sum=f(C.STATS)))
    if op == C.FIRST:
        OH, OW = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
        return _old_dispatch(eb, dict(Cout=64, C=32, wrow=128, IH=H + 2, IW=(W + 5) // 2 * 2, Sy=stride, Sx=stride, OS=1, cls=[(N * OH * OW, 4)], in_bytes=0, pipe_ok=0,
                                      out=1, stat_sum=f(C.STATS), bias=f(C.BIAS), addend=f(C.ADDEND), relu=int(f(C.RELU))))
    if op == C.FWD:
        fuse = bool(flags & 0x3fc)
        rows_ok = not f(C.STATS) or f(C.ROWS_FREE)
        if not fuse and rows_ok and not (c64_needs_out and f(C.NO_OUT)) and _old_c64_takes(shape, eb):
            return (C.CG_C64, 0, 0, 0, 0, 0, 0, N, 1)
        return _old_dispatch(eb, dict(Cout=Cout, C=Cin, wrow=k * k * Cin, IH=H, IW=W, Sy=stride, Sx=stride, OS=1, cls=[(N * OH * OW, k * k)], in_bytes=N * H * W * Cin * eb,
                                      pipe_ok=rows_ok, out=not f(C.NO_OUT), stat_sum=f(C.STATS), bias=f(C.BIAS), addend=f(C.ADDEND), relu=2 if f(C.GELU) else int(f(C.RELU)),
                                      out_f32=f(C.OUT_F32), residual=f(C.RESIDUAL), mask_out=f(C.MASK_OUT), mul=f(C.MUL)))
    fuse = bool(flags & 0xffc)
    addend, in_place = f(C.D_ADDEND), f(C.D_ADDEND) and f(C.D_ADDEND_IS_DIN)
    prof3 = f(C.D_X) and f(C.D_SCALE_SHIFT) and not f(C.D_MASK_Y) and not f(C.D_MASK_BITS) and not f(C.D_X2) and f(C.D_PARTIAL)
    if stride not in (1, 2):
        return None
    if not addend and (not fuse or prof3) and _old_c64_takes(shape, eb):
        return (C.CG_C64, 0, 0, 0, 0, 0, 0, N, 1)
    s1x1 = k == 1 and stride == 1 and pad == 0
    if fuse and in_place and stride != 1 and k == 1:
        return None
    if f(C.D_ADDEND_S2) and not (addend and not in_place and s1x1):
        return None
    Cg, k2 = Cout, 0
    if f(C.D_IN2):
        k2, sh = flags >> 16, 0
        if k2 <= 0:
            return None
        while (k2 << sh) < Cout: sh += 1
        if not (s1x1 and (k2 << sh) == Cout and k2 % (128 // eb) == 0 and Cout % (128 // eb) == 0):
            return None
        Cg = Cout + k2
    cls = []
    for ph in range(stride):
        for pw in range(stride):
            a_dim, b_dim = (H - ph + stride - 1) // stride, (W - pw + stride - 1) // stride
            nt = sum(1 for r in range(k) for q in range(k) if (ph + pad - r) % stride == 0 and (pw + pad - q) % stride == 0)
            if a_dim <= 0 or b_dim <= 0 or (nt == 0 and (in_place or (not addend and not fuse))):
                continue
            cls.append((N * a_dim * b_dim, nt))
    cls.sort(key=lambda c: -c[1])
    return _old_dispatch(eb, dict(Cout=Cin, C=Cg, wrow=Cg if k2 else k * k * Cout, IH=OH, IW=OW, Sy=1, Sx=1, OS=stride, cls=cls, in_bytes=N * OH * OW * Cout * eb, pipe_ok=1, out=1,
                                  addend=addend, stat_sum=f(C.D_PARTIAL), mask_y=f(C.D_MASK_Y), mask_bits=f(C.D_MASK_BITS), x=f(C.D_X), scale=f(C.D_SCALE_SHIFT), x2=f(C.D_X2),
                                  bias=f(C.D_BIAS), in2=f(C.D_IN2), addend_sub=f(C.D_ADDEND_S2)))


FWD_FLAGS = [0, C.STATS, C.TRAIN, C.BIAS | C.RELU, C.BIAS | C.GELU, C.BIAS | C.OUT_F32, C.TR, C.RESIDUAL | C.BIAS, C.RESIDUAL | C.OUT_F32 | C.ADDEND,
             C.MUL | C.BIAS | C.ADDEND | C.RELU | C.MASK_OUT, C.STATS | C.ROWS_FREE | C.NO_OUT, C.ADDEND]
DGRAD_FLAGS = [0, C.D_ADDEND, C.D_ADDEND | C.D_ADDEND_IS_DIN, C.D_EMPTY] + [C.EPI_FLAGS[e] for e in (1, 3, 4, 5, 7)] + [C.EPI_FLAGS[3] | C.D_BIAS, C.EPI_FLAGS[4] | C.D_BIAS]


def _grid():
    pts = []
    widths = (64, 128, 192, 256, 512, 1024)
    for Cin, Cout, k, stride, S, N in itertools.product(widths, widths, (1, 3), (1, 2), (7, 14, 28, 56), (8, 256)):
        pts += [(C.FWD, (N, Cin, S, S, Cout, k, stride, k // 2), fl) for fl in (0, C.TRAIN, C.BIAS | C.RELU)]
        pts += [(C.DGRAD, (N, Cin, S, S, Cout, k, stride, k // 2), fl) for fl in (0, C.EPI_FLAGS[3], C.EPI_FLAGS[4], C.EPI_FLAGS[1])]
    for M, K, N in itertools.product((197, 1576, 4096, 14400, 32768, 50432, 65536), (64, 704, 768, 1024, 2048, 3072, 4096, 8192, 8256, 16384), (64, 128, 384, 768, 1024, 3072, 4096)):
        pts += [(C.FWD, C.linear(M, K, N), fl) for fl in FWD_FLAGS]
        pts += [(C.DGRAD, C.linear(M, N, K), fl) for fl in (0, C.EPI_FLAGS[3], C.D_IN2 | C.D_BIAS | ((K // 4) << 16), C.D_ADDEND | C.D_ADDEND_S2)]
    lib = _lib.load()
    for arch in W.ARCHS:
        for N, S in ((256, 224), (8, 64)):
            for s in sorted(set(W.plan_conv_units(lib, arch, N, S, S))):
                if s[1] == 3:
                    op = C.STEM if s[5] == 7 else C.FIRST
                    pts += [(op, s, fl) for fl in (0, C.STATS)]
                else:
                    pts += [(C.FWD, s, fl) for fl in FWD_FLAGS] + [(C.DGRAD, s, fl) for fl in DGRAD_FLAGS]
    return pts


def test_route_agrees_with_the_cascade_it_replaced_and_keeps_the_row_bounds():
    lib = _lib.load()
    pts = _grid()
    assert len(pts) >= 5000, len(pts)
    refused = rerouted = families = 0
    seen = set()
    for op, shape, flags in pts:
        N, Cin, H, W_, Cout, k, stride, pad = shape
        for eb in (C.BF16, C.F32):
            got, old = C.route(lib, op, shape, eb, flags), _old_route(op, shape, eb, flags)
            # the one intended difference: the transformer-residual contract (an fp32 output) now holds for the 256 x 256 two-stage family too
            if op == C.FWD and flags & C.RESIDUAL and not flags & C.OUT_F32 and old is not None and old[0] == C.CG_BIG256:
                assert got is None, (op, shape, eb, hex(flags), got)
                refused += 1
                continue
            # the other: the cascade sent a forward WITHOUT an output to the all-taps kernel, which stores its tile unconditionally (a store through
            # a null pointer); the route keeps such a launch on the rest of the cascade
            if op == C.FWD and flags & C.NO_OUT and old is not None and old[0] == C.CG_C64:
                old = _old_route(op, shape, eb, flags, c64_needs_out=True)
                assert old[0] == C.CG_TILE128, old
                rerouted += 1
            assert got == old, (op, shape, eb, hex(flags), got, old)
            if got is None:
                continue
            seen.add(got[0])
            if op == C.DGRAD:
                assert got[7] <= _cd(N * H * W_, 128) + stride * stride, (shape, got)          # conv_dgrad_partial_rows
            else:
                assert got[7] <= _cd(N * ((H + 2 * pad - k) // stride + 1) * ((W_ + 2 * pad - k) // stride + 1), 128), (shape, got)   # conv_fwd_stat_rows / stem_conv_stat_rows
    assert refused > 0 and rerouted > 0 and seen == {C.CG_TILE128, C.CG_BIG256, C.CG_PIPE, C.CG_C64, C.CG_STEM7}


def test_table_rows_keep_the_row_bounds_and_agree_with_the_cascade():
    lib = _lib.load()
    for r in C.ROWS:
        N, Cin, H, W_, Cout, k, stride, pad = r.shape
        assert _old_route(r.op, r.shape, r.eb, r.flags) == r.want, r
        if r.op == C.DGRAD:
            assert r.want[7] <= _cd(N * H * W_, 128) + stride * stride          # conv_dgrad_partial_rows
        else:
            assert r.want[7] <= _cd(N * ((H + 2 * pad - k) // stride + 1) * ((W_ + 2 * pad - k) // stride + 1), 128)   # conv_fwd_stat_rows / stem_conv_stat_rows
