"""CPU: the 3-channel 3x3 first conv's geometry (csrc/conv.h FirstGeom) seen through the exports that need no device -- the weight-gradient
plan and the conv-GEMM route of its virtual form, and the image sizes at which the four plans that start with it are created or refused.
Values: tests/first_conv_cases.py."""
import ctypes

import pytest

import conv_route_cases as R
import first_conv_cases as C
import wgrad_plan_cases as W
from mmskin import _lib

ERR_ARG = 1


@pytest.mark.parametrize("key", list(C.PINS), ids=lambda k: "%s-s%d-%s" % ("x".join(map(str, k[0])), k[1], "bf16" if k[2] == 2 else "fp32"))
def test_wgrad_plan_and_route_of_the_virtual_form(key):
    (N, H, Wd), stride, eb = key
    shape = (N, 3, H, Wd, 64, 3, stride, 1)
    lib = _lib.load()
    assert (W.plan(lib, shape, eb), R.route(lib, R.FIRST, shape, eb)) == C.PINS[key]


@pytest.mark.parametrize("arch,H,Wd,created", C.LIMITS, ids=["%s-%dx%d" % r[:3] for r in C.LIMITS])
def test_plans_stop_at_a_240_x_240_first_conv_output(arch, H, Wd, created):
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.mmskin_backbone_create(arch.encode(), 1, H, Wd, _lib.BF16, ctypes.byref(h))
    if created:
        assert rc == 0 and h.value, lib.mmskin_last_error()
        lib.mmskin_backbone_destroy(h)
    else:
        assert rc == ERR_ARG and not h.value
        assert b"too large for the weight-gradient kernel" in lib.mmskin_last_error()
