"""Back-to-back training steps of the ResNet plan: the second of two steps enqueued with no synchronize between them equals a step
run alone, bit for bit (features, flat gradient arena, BatchNorm running statistics).

The kernels are deterministic (slab reductions, no atomics), so the comparison cannot fail by chance.  What it catches is a hand-off
between the main stream and the weight-gradient stream that is missing or guards the wrong buffer: with work of the previous step
still in flight, a gradient buffer rewritten before the side-stream launch reading it has finished changes a weight gradient.

resnet-50 bf16 at N=4, 64 x 64 (the shape of test_gpu_plan_profile.py) runs every block form: mmskin_backbone_unit_flags reports units
with the algebraic BatchNorm backward, with the two-pass forward and with kept Gram statistics at that shape, asserted below, so no
larger shape is needed.  resnet-50 fp32 and resnet-18 bf16 take the ordinary paths and the basic block."""
import ctypes

import pytest
import torch

from gpu_util import DEV
from mmskin import _lib
from mmskin._lib import call
from oracle.detinit import det_init_, det_tensor

pytestmark = pytest.mark.gpu

N, HW = 4, 64
ABN, FWD2P, GRAM = 1, 2, 4   # MMSKIN_UNIT_* of mmskin.h
CASES = [("resnet-50", "bf16"), ("resnet-50", "fp32"), ("resnet-18", "bf16")]


def unit_flag_counts(plan):
    n = ctypes.c_int()
    counts = {ABN: 0, FWD2P: 0, GRAM: 0}
    for i in range(_lib.load().mmskin_backbone_num_units(plan.handle)):
        call("mmskin_backbone_unit_flags", plan.handle, i, ctypes.byref(n))
        for bit in counts:
            counts[bit] += bool(n.value & bit)
    return counts


def enqueue_step(m, x, w, buffers0):
    """One training step from buffers0, enqueued only: restore (a device copy on the same stream), forward, backward."""
    with torch.no_grad():
        m._flat_b.copy_(buffers0)
    for p in m.parameters():
        p.grad = None
    f = m(x)
    (f * w).sum().backward()
    return f.detach(), m.last_flat_grad, m._flat_b.detach().clone()


@pytest.mark.parametrize("arch,dtype", CASES, ids=["-".join(c) for c in CASES])
def test_second_of_two_unsynchronized_steps_equals_a_step_alone(arch, dtype):
    from mmskin.backbone import HipResNet
    m = det_init_(HipResNet(arch, compute_dtype=dtype)).to(DEV).train()
    x = det_tensor("backward.img", (N, 3, HW, HW)).to(DEV)
    w = det_tensor("backward.w", (N, m.num_features)).to(DEV)
    counts = unit_flag_counts(m._plan_for(N, HW, HW, x.device))
    if (arch, dtype) == ("resnet-50", "bf16"):
        assert all(c >= 1 for c in counts.values()), counts   # all three algebraic forms run at this shape
    else:
        assert not any(counts.values()), counts
    buffers0 = m._flat_b.detach().clone()

    solo = enqueue_step(m, x, w, buffers0)
    torch.cuda.synchronize()
    solo = tuple(t.clone() for t in solo)
    assert all(torch.isfinite(t).all() for t in solo)
    assert not torch.equal(solo[2], buffers0)   # the step did update the running statistics

    first = enqueue_step(m, x, w, buffers0)
    second = enqueue_step(m, x, w, buffers0)
    torch.cuda.synchronize()
    for name, got, want in zip(("features", "gradients", "buffers"), second, solo):
        assert torch.equal(got, want), (name, float((got - want).abs().max()))
    for name, got, want in zip(("features", "gradients", "buffers"), first, solo):
        assert torch.equal(got, want), ("first step", name, float((got - want).abs().max()))
