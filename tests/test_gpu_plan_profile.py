"""The profiled path of the plan executors (mmskin_backbone_profile_enable: single stream, one event pair per launch group; what
bench.py's live roofline reads) against the normal path (weight gradients on the side stream), one training step per plan.

(i)  Both paths enqueue the same kernels with the same arguments, and the kernels are deterministic (slab reductions, no atomics), so
     features, the flat gradient arena and the BatchNorm running statistics are bit-identical.
(ii) The profiler's per-class totals are host arithmetic over the plan's shapes (sums of small-integer products, exact in a double):
     FLOPs, bytes and event pairs per class are pinned to the values of commit a9b9008, before the BatchNorm-backward chain, the stem
     and the side-stream hand-off were each written once.  Classes: conv fwd, dgrad, wgrad, BN fwd, BN bwd, stage, stem/misc."""
import ctypes

import pytest
import torch

from gpu_util import DEV
from mmskin._lib import call
from oracle.detinit import det_init_, det_tensor

pytestmark = pytest.mark.gpu

N, HW = 4, 64   # every stage's map is >= 2x2: every block type, both ResNet block-0 forms and DenseNet's three transitions run

CASES = [("resnet-50", "bf16"), ("resnet-50", "fp32"), ("resnet-18", "bf16"), ("densenet169", "bf16"), ("densenet169", "fp32"),
         ("mobilenet-v2", "bf16"), ("efficientnet-b0", "bf16")]

# (flops7, bytes7, launches7) of one training forward + backward
EXPECTED = {
    ('resnet-50', 'bf16'): ([2669150208.0, 2592079872.0, 2669150208.0, 0.0, 0.0, 0.0, 0.0],
        [62966144.0, 74366976.0, 60489728.0, 10059776.0, 12861440.0, 0.0, 0.0],
        [53, 52, 53, 101, 53, 1, 2]),
    ('resnet-50', 'fp32'): ([2669150208.0, 2592079872.0, 2669150208.0, 0.0, 0.0, 0.0, 0.0],
        [122262272.0, 148733952.0, 120979456.0, 30212096.0, 44597248.0, 0.0, 0.0],
        [53, 52, 53, 101, 53, 1, 2]),
    ('resnet-18', 'bf16'): ([1184366592.0, 1107296256.0, 1184366592.0, 0.0, 0.0, 0.0, 0.0],
        [25381248.0, 26902528.0, 24739840.0, 2457600.0, 5193728.0, 0.0, 0.0],
        [20, 19, 20, 36, 20, 1, 2]),
    ('densenet169', 'bf16'): ([2241331200.0, 2164260864.0, 2241331200.0, 0.0, 0.0, 0.0, 0.0],
        [48875904.0, 60456960.0, 48234496.0, 25931776.0, 38547456.0, 0.0, 0.0],
        [168, 167, 168, 505, 255, 1, 10]),
    ('densenet169', 'fp32'): ([2241331200.0, 2164260864.0, 2241331200.0, 0.0, 0.0, 0.0, 0.0],
        [97751808.0, 120913920.0, 96468992.0, 51863552.0, 77094912.0, 0.0, 0.0],
        [168, 167, 168, 505, 255, 1, 10]),
    ('mobilenet-v2', 'bf16'): ([388386816.0, 381308928.0, 388386816.0, 0.0, 0.0, 0.0, 0.0],
        [17333632.0, 11855872.0, 11589632.0, 14528512.0, 36925440.0, 0.0, 0.0],
        [52, 51, 52, 173, 52, 19, 1]),
    ('efficientnet-b0', 'bf16'): ([450074624.0, 442996736.0, 450074624.0, 0.0, 0.0, 0.0, 0.0],
        [19475840.0, 13873152.0, 13625344.0, 19210240.0, 41975808.0, 0.0, 0.0],
        [49, 48, 49, 188, 74, 66, 1]),
}


def build(arch, dtype):
    from mmskin import backbone as B
    cls = {"resnet-50": B.HipResNet, "resnet-18": B.HipResNet, "densenet169": B.HipDenseNet, "mobilenet-v2": B.HipMobileNetV2,
           "efficientnet-b0": B.HipEfficientNet}[arch]
    return det_init_(cls(arch, compute_dtype=dtype)).to(DEV)


def train_step(m, x, w, buffers0, profile):
    """One training step from the same state; returns (features, flat gradients, BatchNorm buffers[, profiler totals])."""
    plan = m._plan_for(x.shape[0], x.shape[2], x.shape[3], x.device)
    with torch.no_grad():
        m._flat_b.copy_(buffers0)
    for p in m.parameters():
        p.grad = None
    m.train()
    torch.manual_seed(0)   # EfficientNet draws its stochastic-depth masks from torch's generator
    prof = None
    if profile:
        call("mmskin_backbone_profile_enable", plan.handle, 1)
    try:
        f = m(x)
        (f * w).sum().backward()
        torch.cuda.synchronize()
        if profile:
            ms, fl, by = ((ctypes.c_double * 7)() for _ in range(3))
            ln = (ctypes.c_int64 * 7)()
            call("mmskin_backbone_profile_read", plan.handle, ms, fl, by, ln)
            prof = (list(fl), list(by), list(ln))
    finally:
        if profile:
            call("mmskin_backbone_profile_enable", plan.handle, 0)
    out = (f.detach().clone(), m.last_flat_grad.clone(), m._flat_b.detach().clone())
    return out + (prof,) if profile else out


def inputs(m):
    return det_tensor("profile.img", (N, 3, HW, HW)).to(DEV), det_tensor("profile.w", (N, m.num_features)).to(DEV)


@pytest.mark.parametrize("arch,dtype", CASES, ids=["-".join(c) for c in CASES])
def test_profiled_step_equals_side_stream_step_and_counts_what_it_did(arch, dtype):
    m = build(arch, dtype)
    x, w = inputs(m)
    buffers0 = m._flat_b.detach().clone()
    side = train_step(m, x, w, buffers0, False)
    f, g, b, prof = train_step(m, x, w, buffers0, True)
    print(arch, dtype, prof)
    assert all(torch.isfinite(t).all() for t in (f, g, b))
    for name, got, want in zip(("features", "gradients", "buffers"), (f, g, b), side):
        assert torch.equal(got, want), (name, float((got - want).abs().max()))
    assert not torch.equal(b, buffers0)   # the step did update the running statistics
    flops, nbytes, launches = EXPECTED[(arch, dtype)]
    assert prof[0] == flops, ("flops", prof[0])
    assert prof[1] == nbytes, ("bytes", prof[1])
    assert prof[2] == launches, ("launches", prof[2])
