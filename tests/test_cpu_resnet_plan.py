"""What the ResNet plan decides at creation (mmskin_backbone_unit_flags; no GPU): which units take the algebraic BatchNorm backward, the
two-pass forward with or without kept Gram statistics, and the compact stride-2 downsample gradient.

(i)   Implications between the flags and the unit's shape that the executor relies on, for every unit of resnet-18 / resnet-50 in both
      dtypes at three shapes.
(ii)  fp32 plans and resnet-18 take none of the algebraic forms.
(iii) At the production shape (resnet-50, bf16, 256 x 224 x 224) the set of units carrying each flag, and at every shape the workspace
      size, equal tests/golden/resnet_plan.json: recorded from commit e79992f with this export alone added, before the backward was
      rewritten as steps and the choices moved into build_plan."""
import ctypes
import json
import os

import pytest

from mmskin import _lib

FLAGS = {"ABN": 1, "FWD2P": 2, "GRAM": 4, "DS": 8, "DS_COMPACT": 16, "LAST_BLOCK": 32}   # MMSKIN_UNIT_* of mmskin.h
SHAPES = [(4, 64, 64), (3, 90, 70), (256, 224, 224)]
CASES = [(a, d, s) for a in ("resnet-18", "resnet-50") for d in ("fp32", "bf16") for s in SHAPES]
DT = {"fp32": _lib.F32, "bf16": _lib.BF16}

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resnet_plan.json")) as _f:
    GOLDEN = json.load(_f)


def key(arch, dtype, shape):
    return f"{arch}/{dtype}/{shape[0]}x{shape[1]}x{shape[2]}"


def abn_accepts(C4, Cw):
    """csrc/conv.h, from the limits documented there: abn_prep Cw in {64, 128, 256}, C4 <= 1024, C4 % (4 * (256 / Cw)) == 0;
    abn_wgrad_finalize Cw <= 256; the data gradient's second operand C4 = Cw * 2^j."""
    if Cw not in (64, 128, 256) or not 0 < C4 <= 1024 or C4 % (4 * (256 // Cw)) or C4 % Cw:
        return False
    ratio = C4 // Cw
    return ratio & (ratio - 1) == 0


class PlanView:
    """Units of a plan: name -> dict(flags, Cout, Cin, H, W, OH, OW, kh, kw), and the workspace size."""

    def __init__(self, arch, dtype, shape):
        lib = _lib.load()
        h = ctypes.c_void_p()
        _lib.check(lib.mmskin_backbone_create(arch.encode(), *shape, DT[dtype], ctypes.byref(h)))
        try:
            self.workspace_bytes = lib.mmskin_backbone_workspace_bytes(h)
            kernel = {}
            for i in range(lib.mmskin_backbone_num_tensors(h, 0)):
                name = ctypes.create_string_buffer(128)
                ndim, shape4 = ctypes.c_int(), (ctypes.c_int64 * 4)()
                _lib.check(lib.mmskin_backbone_tensor_info(h, 0, i, name, 128, None, None, ctypes.byref(ndim), shape4))
                if ndim.value == 4:
                    kernel[name.value.decode()] = (shape4[2], shape4[3])
            self.units = {}
            for i in range(lib.mmskin_backbone_num_units(h)):
                name = ctypes.create_string_buffer(128)
                info, flags = (ctypes.c_int64 * 12)(), ctypes.c_int(-1)
                _lib.check(lib.mmskin_backbone_unit_info(h, i, name, 128, info))
                _lib.check(lib.mmskin_backbone_unit_flags(h, i, ctypes.byref(flags)))
                nm = name.value.decode()
                self.units[nm] = dict(flags=flags.value, Cout=info[4], OH=info[5], OW=info[6], Cin=info[7], H=info[8], W=info[9],
                                      kh=kernel[nm][0], kw=kernel[nm][1])
        finally:
            lib.mmskin_backbone_destroy(h)

    def names_with(self, flag):
        return sorted(n for n, u in self.units.items() if u["flags"] & FLAGS[flag])


_views = {}


def view(arch, dtype, shape):
    k = key(arch, dtype, shape)
    if k not in _views:
        _views[k] = PlanView(arch, dtype, shape)
    return _views[k]


def block_of(name):
    return ".".join(name.split(".")[:2])   # "layer2.0.conv3.weight" -> "layer2.0"


def is_1x1(u):
    return u["kh"] == 1 and u["kw"] == 1


def stride_of_1x1(u):
    """stride of an unpadded 1x1 convolution from its input and output extents (the plans use 1 and 2 only)"""
    for s in (1, 2):
        if u["OH"] == (u["H"] - 1) // s + 1 and u["OW"] == (u["W"] - 1) // s + 1:
            return s
    raise AssertionError(u)


@pytest.mark.parametrize("arch,dtype,shape", CASES, ids=[key(*c) for c in CASES])
def test_flag_implications_hold_for_every_unit(arch, dtype, shape):
    v = view(arch, dtype, shape)
    last_block = block_of(list(v.units)[-1])
    assert len(v.units) == {"resnet-18": 20, "resnet-50": 53}[arch]
    for name, u in v.units.items():
        f = {k: bool(u["flags"] & b) for k, b in FLAGS.items()}
        assert u["flags"] < 64, (name, u["flags"])
        assert f["DS"] == (".downsample." in name), name
        assert f["LAST_BLOCK"] == (block_of(name) == last_block), name
        if f["FWD2P"]:
            assert f["ABN"] and not f["DS"] and not f["LAST_BLOCK"], (name, f)
            assert block_of(name) + ".downsample.0.weight" not in v.units, name
        if f["GRAM"]:
            assert f["FWD2P"], (name, f)
        if f["ABN"]:
            assert dtype == "bf16" and arch == "resnet-50", name
            assert is_1x1(u) and stride_of_1x1(u) == 1 and u["Cin"] <= 128 and abn_accepts(u["Cout"], u["Cin"]), (name, u)
        if f["DS_COMPACT"]:
            assert f["DS"] and is_1x1(u) and stride_of_1x1(u) == 2 and block_of(name) != "layer1.0", (name, u)
    if dtype == "fp32" or arch == "resnet-18":
        assert not any(u["flags"] & (FLAGS["ABN"] | FLAGS["FWD2P"] | FLAGS["GRAM"]) for u in v.units.values())


def test_production_plan_selects_what_it_did_before():
    arch, dtype, shape = "resnet-50", "bf16", (256, 224, 224)
    assert key(arch, dtype, shape) == GOLDEN["production_case"]
    v = view(arch, dtype, shape)
    for flag in FLAGS:
        assert v.names_with(flag) == sorted(GOLDEN["production_flags"][flag]), flag
    assert all(GOLDEN["production_flags"][flag] for flag in FLAGS)   # every decision is exercised by the production plan


@pytest.mark.parametrize("arch,dtype,shape", CASES, ids=[key(*c) for c in CASES])
def test_workspace_bytes_unchanged(arch, dtype, shape):
    assert view(arch, dtype, shape).workspace_bytes == GOLDEN["workspace_bytes"][key(arch, dtype, shape)]


def test_unit_flags_errors():
    lib = _lib.load()
    h, f = ctypes.c_void_p(), ctypes.c_int()
    _lib.check(lib.mmskin_backbone_create(b"resnet-18", 2, 64, 64, _lib.F32, ctypes.byref(h)))
    try:
        assert lib.mmskin_backbone_unit_flags(h, lib.mmskin_backbone_num_units(h), ctypes.byref(f)) == 1   # MMSKIN_ERR_ARG
        assert lib.mmskin_backbone_unit_flags(h, -1, ctypes.byref(f)) == 1
        assert lib.mmskin_backbone_unit_flags(h, 0, None) == 1
    finally:
        lib.mmskin_backbone_destroy(h)
    for arch in (b"vgg16-features", b"mobilenet-v2"):   # a plan without units; a plan with units of another kind
        _lib.check(lib.mmskin_backbone_create(arch, 2, 64, 64, _lib.F32, ctypes.byref(h)))
        try:
            assert lib.mmskin_backbone_unit_flags(h, 0, ctypes.byref(f)) == 3, arch   # MMSKIN_ERR_UNSUPPORTED
        finally:
            lib.mmskin_backbone_destroy(h)
