"""The table of tests/mbconv_cases.py checked without a GPU: every row runs through F.conv2d(groups = C) in fp64, every row's note is
turned into an assertion on the launch geometry recomputed from csrc/ops.hip (dww_strips, dww_rows_plan), and the depthwise units of the
real MobileNet-V2 / EfficientNet plans at 224 and 225 (plan creation launches nothing) must all fall in a class the table holds."""
import ctypes

import pytest

from mbconv_cases import (DW_CASES, DWW_LANES, EPC, KS, dw_class, dw_id, dw_reference, dww_rows_plan, out_hw, pad64, rows_kernel,
                          tapped_plan)
from mmskin import _lib
from mmskin.backbone import _Plan


@pytest.mark.parametrize("case", DW_CASES, ids=dw_id)
def test_case_is_a_valid_depthwise_convolution(case):
    c = case
    assert c.N >= 2 and c.C % 64 == 0 and 1 <= c.c_valid <= c.C and pad64(c.c_valid) == c.C and (c.ksize, c.stride) in KS
    r = dw_reference(c)
    OH, OW = out_hw(c.H, c.W, c.ksize, c.stride)
    assert tuple(r["y"].shape) == (c.N, c.C, OH, OW) and tuple(r["dx"].shape) == (c.N, c.C, c.H, c.W)
    assert tuple(r["dw"].shape) == (c.c_valid, 1, c.ksize, c.ksize)
    assert float(r["y"][:, : c.c_valid].abs().max()) > 0 and float(r["dw"].abs().max()) > 0
    if c.c_valid < c.C:   # the padding carries data in, and the reference carries none out
        assert float(r["x"][:, c.c_valid:].abs().min()) > 0 and float(r["dy"][:, c.c_valid:].abs().min()) > 0
        assert float(r["y"][:, c.c_valid:].abs().max()) == 0 and float(r["dx"][:, c.c_valid:].abs().max()) == 0
    assert 4 * max(r["x"].numel(), r["dy"].numel()) <= 9 << 20, "a case moves a few megabytes at the most"


def _rows(c, dtype):
    return dww_rows_plan(c.N, c.H, c.C // EPC[dtype])


EDGE = {
    "parities": lambda c: c.H % 2 == 1 and c.W % 2 == 0 and c.H != c.W and c.H >= 5 and c.W >= 5,
    "even": lambda c: c.H % 2 == 0 and c.W % 2 == 0 and c.H >= 5,
    "odd": lambda c: c.H % 2 == 1 and c.W % 2 == 1 and c.H >= 5,
    "small": lambda c: c.H < 3 and c.W < 5 and c.H * c.W > 1,
    "one": lambda c: c.H == 1 and c.W == 1,
    "cw24": lambda c: c.C == c.c_valid and _rows(c, "fp32")["CW"] == 24 and _rows(c, "fp32")["lanes"] == 10 and _rows(c, "fp32")["gy"] == 2
    and _rows(c, "bf16")["CW"] == 24 and _rows(c, "bf16")["gy"] == 1,
    "ragged_cblock": lambda c: all(_rows(c, d)["CW"] == 32 and _rows(c, d)["gy"] > 1 and (c.C // EPC[d]) % 32 != 0 for d in EPC),
    "padded": lambda c: c.c_valid < c.C and c.c_valid % 8 == 0,
    "strips2": lambda c: tapped_plan(c) == (2, 1262, 2523) and 1262 % DWW_LANES != 0 and not rows_kernel(c),
    "rpl2_fp32": lambda c: rows_kernel(c) and _rows(c, "fp32") == dict(CW=24, gy=2, lanes=10, rpl=2, nb=134, NR=2664)
    and 133 * 20 < 2664 < 134 * 20,     # the last block starts inside the tensor and ends past it: the `row >= NR` break
    "rpl2_bf16": lambda c: rows_kernel(c) and _rows(c, "bf16")["rpl"] == 2 and _rows(c, "bf16")["gy"] == 1
    and _rows(c, "bf16")["nb"] * _rows(c, "bf16")["lanes"] * 2 > c.N * c.H,
}


@pytest.mark.parametrize("case", DW_CASES, ids=dw_id)
def test_case_reaches_the_edge_its_note_claims(case):
    assert EDGE[case.edge](case), case.note
    # the basic cases stay single-strip / one row per lane, so the multi-strip rows are the only ones that can reach those paths
    if case.edge not in ("strips2", "rpl2_fp32", "rpl2_bf16"):
        assert tapped_plan(case)[0] == 1 and _rows(case, "fp32")["rpl"] == 1 and _rows(case, "bf16")["rpl"] == 1


def test_table_holds_every_required_row():
    rows = {(c.N, c.C, c.c_valid, c.H, c.W, c.ksize, c.stride) for c in DW_CASES}
    assert len(rows) == len(DW_CASES), "duplicate row"
    for k, s in KS:
        for H, W in ((7, 10), (8, 8), (2, 3), (1, 1)):
            assert (2, 64, 64, H, W, k, s) in rows
        for C, cv in ((192, 192), (320, 320), (192, 144)):
            assert any(r[1:3] == (C, cv) and r[5:] == (k, s) for r in rows)
    for r in ((3, 64, 64, 57, 57, 3, 2), (3, 64, 64, 58, 58, 5, 2), (24, 192, 192, 111, 3, 3, 1)):
        assert r in rows
    assert any(c.edge == "rpl2_bf16" for c in DW_CASES)
    # each weight-gradient kernel meets a case where the window is larger than the image, in both strides where it has them
    assert any(rows_kernel(c) and c.H < 3 for c in DW_CASES) and any(not rows_kernel(c) and c.H < c.ksize for c in DW_CASES)


def _depthwise_units(arch, size):
    """(name, ksize, stride, H, W, c_valid) of every depthwise unit of the plan, from unit_info and tensor_info"""
    lib = _lib.load()
    plan = _Plan(arch, 2, size, size, _lib.F32, None)
    shapes = {name: shape for name, _, _, shape in plan.tensor_table(0)}
    out = []
    n = lib.mmskin_backbone_num_units(plan.handle)
    assert n > 0
    for i in range(n):
        name = ctypes.create_string_buffer(128)
        info = (ctypes.c_int64 * 12)()
        _lib.call("mmskin_backbone_unit_info", plan.handle, i, name, 128, info)
        shape = shapes[name.value.decode()]
        rows, cout, OH, OW, cin, H, W = info[3:10]
        assert rows == 2 * OH * OW
        if len(shape) == 4 and shape[1] == 1 and shape[2] >= 3:
            k = shape[2]
            assert shape == (cout, 1, k, k) and cin == cout
            strides = [s for s in (1, 2) if out_hw(H, W, k, s) == (OH, OW)]
            assert len(strides) == 1, (name.value, H, W, OH, OW)
            out.append((name.value.decode(), k, strides[0], H, W, cout))
    return out


@pytest.mark.parametrize("size", [224, 225])
@pytest.mark.parametrize("arch,n_dw", [("mobilenet-v2", 17), ("efficientnet-b0", 16), ("efficientnet-b7", 55)])
def test_every_depthwise_unit_of_the_plans_has_its_class_in_the_table(arch, n_dw, size):
    have = {dw_class(c.ksize, c.stride, c.H, c.W, c.c_valid < c.C) for c in DW_CASES}
    units = _depthwise_units(arch, size)
    assert len(units) == n_dw   # torchvision: one depthwise conv per InvertedResidual / MBConv block
    for name, k, s, H, W, cv in units:
        assert dw_class(k, s, H, W, cv % 64 != 0) in have, (arch, size, name, k, s, H, W, cv)
