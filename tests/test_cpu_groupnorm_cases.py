"""No GPU: the inputs of tests/groupnorm_cases.py have the properties tests/test_gpu_groupnorm_ops.py relies on, and the op-level entry
points of csrc/groupnorm.hip size and refuse on the host."""
import pytest
import torch
import torch.nn.functional as F

import groupnorm_cases as G
from mmskin import _lib

ALL = [(s, False) for s in G.SMALL_SHAPES + [G.LARGE_SHAPE]] + [(G.CONDITIONING_SHAPE, True)]


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("shape,conditioning", ALL, ids=lambda v: G.case_id(v) if isinstance(v, tuple) else str(v))
def test_inputs_keep_every_decision_off_a_rounding(shape, conditioning, pool):
    y, gamma, beta, gout = G.inputs(shape, pool, conditioning)
    for t in (y, gamma, beta, gout):
        assert torch.equal(t, G.rb(t)), "bf16-representable"
    r64 = G.references(shape, pool, conditioning)[0]
    assert float(r64["pre"].abs().min()) >= G.MARGIN
    near_zero, near_tie = G.excluded(r64, pool)
    assert float(near_zero.float().mean()) <= G.EXCLUDED_CAP, float(near_zero.float().mean())
    if pool:
        assert float(G.deciding_gap(r64["pre"].clamp_min(0)).min()) >= G.MARGIN
        assert float(near_tie.float().mean()) <= G.EXCLUDED_CAP, float(near_tie.float().mean())
        assert int(r64["tap"].min()) >= 0 and int(r64["tap"].max()) <= 3
        z = r64["pre"].clamp_min(0)
        assert torch.equal(G.window_taps(z).gather(-1, r64["tap"].unsqueeze(-1)).squeeze(-1), F.max_pool2d(z, 2))
    if conditioning:
        grp = y.double().reshape(shape[0], G.GROUPS, -1)
        assert float((grp.mean(-1) - 50).abs().max()) < 0.5 and float((grp.std(-1) - 1).abs().max()) < 0.3


def test_an_all_zero_window_takes_tap_0_in_the_reference():
    z = torch.zeros(1, 1, 2, 2, dtype=torch.float64)
    _, flat = F.max_pool2d(z, 2, return_indices=True)
    assert int(flat) == 0


def test_workspace_sizes_and_host_side_refusals():
    lib = _lib.load()
    for (N, C, H, W) in G.SMALL_SHAPES:
        for pool in (0, 1):
            es, rows, orows = 4, N * H * W, N * (H // 2 if pool else H) * (W // 2 if pool else W)
            assert lib.mmskin_groupnorm8_relu_workspace_bytes(N, C, H, W, 8, pool) >= es * C * (2 * rows + 2 * orows) + pool * orows * C
    for args, code in (((1, 96, 4, 4, 8, 0), 3), ((1, 64, 4, 4, 4, 0), 3), ((1, 2048, 4, 4, 8, 0), 3), ((1, 64, 1, 4, 8, 1), 1), ((0, 64, 4, 4, 8, 0), 1)):
        assert lib.mmskin_groupnorm8_relu_workspace_bytes(*args) == -1
        assert lib.mmskin_groupnorm8_relu_forward(None, None, None, None, None, None, None, *args, 1e-5, 0, None, None) == code
        assert lib.mmskin_groupnorm8_relu_backward(None, None, None, None, None, None, None, *args, 1e-5, 1, None, None) == code
        assert lib.mmskin_last_error()
