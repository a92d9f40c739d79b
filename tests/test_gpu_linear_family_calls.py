"""-m gpu: the launch trace of the Linear family of mmskin/ops.py (linear, linear_gelu, mlp, star_relu, gelu, gelu_tanh, dw7_star) is
pinned.  ops.call is replaced by a recorder that forwards to the real one and notes, per call, the entry-point name, the positions
of the None arguments and the plain-integer arguments (the stream is a c_void_p and so are all pointers: no pointer value is ever
recorded).  Each case runs forward + backward once and must reproduce the literal in EXPECTED, which was recorded from the wrappers as
they stood BEFORE MlpFn / StarMlpFn and the two keep-or-plain Linear forwards were folded (MMSKIN_PRINT_TRACES=1 prints the traces
instead of only comparing them) -- the fold may not change which entry points run, in which order, with which sizes, or which pointer
arguments are null.  Every case first asks the library for the route of its GEMM shapes (mmskin_linear_route), so a change of the route
predicates cannot quietly move a case off the branch it was chosen for.

Shapes: (64, 64, 64) fp32 mode = LIN_SMALL, (2048, 64, 64) bf16 mode = LIN_BIG_BF16, (2048, 96, 96) bf16 mode = LIN_PADDED_BF16 -- the
smallest of each route; the MLP cases use hidden width 4 x, which keeps both of their GEMMs on the route of the case."""
import os

import pytest
import torch

from gpu_util import DEV, linear_mode
from linear_route_cases import BIG_BF16, BIG_F32, PADDED, SMALL
from mmskin import _lib, ops

pytestmark = pytest.mark.gpu


def leaf(*shape, grad=True, scale=1.0, seed=0):
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(1000 * seed + sum(shape))) * scale
    return t.to(DEV).requires_grad_(grad)


def linear_case(M, K, N, variant):
    def fn():
        x = leaf(M, K, seed=1)
        w = leaf(N, K, grad=variant != "w_frozen", scale=K ** -0.5, seed=2)
        b = None if variant == "no_bias" else leaf(N, seed=3)
        res = leaf(M, N, seed=4) if variant == "residual" else None
        return ops.linear(x, w, b, relu=variant == "relu", residual=res), dict(x=x, w=w, b=b, res=res)
    return fn


def linear_gelu_case(M, K, N, variant):
    def fn():
        x, w, b = leaf(M, K, seed=1), leaf(N, K, grad=variant != "w_frozen", scale=K ** -0.5, seed=2), leaf(N, seed=3)
        return ops.linear_gelu(x, w, b), dict(x=x, w=w, b=b)
    return fn


def mlp_case(M, K, Hd, act, residual, x_grad=True):
    def fn():
        x = leaf(M, K, grad=x_grad, seed=1)
        w1, b1 = leaf(Hd, K, scale=K ** -0.5, seed=2), leaf(Hd, seed=3)
        w2, b2 = leaf(K, Hd, scale=Hd ** -0.5, seed=4), leaf(K, seed=5)
        res = leaf(M, K, seed=6) if residual else None
        s, sb = None, None
        if act == "star":      # timm StarReLU: one-element scale and bias
            s = torch.full((1,), 0.8944, device=DEV, requires_grad=True)
            sb = torch.full((1,), -0.4472, device=DEV, requires_grad=True)
        y = ops.mlp(x, w1, b1, w2, b2, residual=res, star_relu=None if s is None else (s, sb))
        return y, dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, res=res, s=s, sb=sb)
    return fn


def elementwise_case(name):
    def fn():
        z = leaf(3, 37, seed=1)
        if name == "star_relu":
            s, b = leaf(1, seed=2), leaf(1, seed=3)
            return ops.star_relu(z, s, b), dict(z=z, s=s, b=b)
        return getattr(ops, name)(z), dict(z=z)
    return fn


def dw7_star_case(grad_s, grad_b):
    def fn():
        z, w = leaf(1, 7, 7, 8, seed=1), leaf(8, 1, 7, 7, seed=2)
        s, b = leaf(1, grad=grad_s, seed=3), leaf(1, grad=grad_b, seed=4)
        return ops.dw7_star(z, w, s, b), dict(z=z, w=w, s=s, b=b)
    return fn


def _cases():
    """(id, operand mode, [(M, K, N, route) of every GEMM of the case], fn)"""
    cases = []
    routes = (("small", "fp32", 64, 64, 64, SMALL), ("big_bf16", "bf16", 2048, 64, 64, BIG_BF16), ("padded", "bf16", 2048, 96, 96, PADDED))
    for rname, mode, M, K, N, route in routes:
        for variant in ("all", "relu", "residual", "w_frozen", "no_bias"):
            cases.append((f"linear-{rname}-{variant}", mode, [(M, K, N, route)], linear_case(M, K, N, variant)))
        for variant in ("all", "w_frozen"):
            cases.append((f"linear_gelu-{rname}-{variant}", mode, [(M, K, N, route)], linear_gelu_case(M, K, N, variant)))
    for act in ("gelu", "star"):
        for kind, mode, M, K, route in (("fused", "bf16", 2048, 64, BIG_BF16), ("fused", "bf16", 2048, 96, PADDED),
                                        ("fallback", "bf16", 64, 64, SMALL), ("fallback", "fp32", 2048, 64, BIG_F32)):
            gemms = [(M, K, 4 * K, route), (M, 4 * K, K, route)]
            for residual in (False, True):
                cid = f"mlp-{act}-{kind}-{mode}-{M}x{K}-{'res' if residual else 'nores'}"
                cases.append((cid, mode, gemms, mlp_case(M, K, 4 * K, act, residual)))
        cases.append((f"mlp-{act}-fused-bf16-2048x64-res-x_frozen", "bf16", [(2048, 64, 256, BIG_BF16), (2048, 256, 64, BIG_BF16)],
                      mlp_case(2048, 64, 256, act, True, x_grad=False)))
    # StarReLU with a hidden width that is no multiple of 4: the fused Function is not offered whatever the route (it is LIN_SMALL here)
    cases.append(("mlp-star-hidden262-bf16-2048x65-nores", "bf16", [(2048, 65, 262, SMALL), (2048, 262, 65, SMALL)],
                  mlp_case(2048, 65, 4 * 65 + 2, "star", False)))
    for name in ("star_relu", "gelu", "gelu_tanh"):
        cases.append((name, "fp32", [], elementwise_case(name)))
    cases.append(("dw7_star-grad_s_only", "fp32", [], dw7_star_case(True, False)))
    cases.append(("dw7_star-grad_b_only", "fp32", [], dw7_star_case(False, True)))
    return cases


CASES = _cases()
FUSED_MLP = [c for c in CASES if c[0].startswith("mlp-") and "-fused-" in c[0]]


def run_case(case, monkeypatch, before_backward=None):
    """forward + backward of one case under its operand mode with ops.call recorded -> (trace, output, leaves)"""
    cid, mode, gemms, fn = case
    trace = []
    real = ops.call

    def recorder(name, *args):
        trace.append((name, tuple(i for i, a in enumerate(args) if a is None), tuple(a for a in args if type(a) is int)))
        return real(name, *args)

    with linear_mode(mode):
        for M, K, N, route in gemms:
            got = _lib.load().mmskin_linear_route(M, K, N)
            assert got == route, f"{cid}: ({M}, {K}, {N}) in {mode} mode takes route {got}, the case was written for route {route}"
        with monkeypatch.context() as m:
            m.setattr(ops, "call", recorder)
            y, leaves = fn()
            if before_backward is not None:
                before_backward(y)
            y.backward(leaf(*y.shape, grad=False, seed=9))
        torch.cuda.synchronize()
    return trace, y, leaves


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_launch_trace(case, monkeypatch):
    trace, y, leaves = run_case(case, monkeypatch)
    if os.environ.get("MMSKIN_PRINT_TRACES"):
        print(f"\nTRACE {case[0]!r}: {trace!r},")
    for name, t in leaves.items():
        if t is not None and t.requires_grad:
            assert t.grad is not None and t.grad.shape == t.shape, f"{case[0]}: no gradient of shape {tuple(t.shape)} for {name}"
    assert trace == EXPECTED[case[0]]


@pytest.mark.parametrize("case", FUSED_MLP, ids=[c[0] for c in FUSED_MLP])
def test_fused_mlp_backward_returns_ten_values(case, monkeypatch):
    """The one MLP Function takes (x, w1, b1, w2, b2, s, sb, res, p1, p2), so its backward hands back exactly ten values; those for
    s / sb are None with GELU and tensors of s.shape with StarReLU, where they arrive as .grad of the two leaves."""
    returned = []

    def spy_on_backward(y):
        cls = type(y.grad_fn)._forward_cls
        real = cls.backward

        def backward(ctx, *grads):
            returned.append(real(ctx, *grads))
            return returned[-1]
        monkeypatch.setattr(cls, "backward", staticmethod(backward))

    trace, y, leaves = run_case(case, monkeypatch, spy_on_backward)
    assert any(name == "mmskin_linear_forward_x16" for name, _, _ in trace), "not the fused Function"
    assert len(returned) == 1 and len(returned[0]) == 10
    ds, dsb = returned[0][5:7]
    s, sb = leaves["s"], leaves["sb"]
    if "-star-" in case[0]:
        assert ds.shape == s.shape and dsb.shape == s.shape
        assert s.grad is not None and s.grad.shape == s.shape and sb.grad is not None and sb.grad.shape == s.shape
    else:
        assert s is None and sb is None and ds is None and dsb is None


# recorded from the wrappers before the fold (see the module docstring); (entry point, positions of None arguments, integer arguments)
EXPECTED = {
    'linear-small-all': [
        ('mmskin_linear_forward', (), (64, 64, 64, 0)),
        ('mmskin_linear_backward', (3, 4), (64, 64, 64)),
    ],
    'linear-small-relu': [
        ('mmskin_linear_forward', (), (64, 64, 64, 1)),
        ('mmskin_linear_backward', (), (64, 64, 64)),
    ],
    'linear-small-residual': [
        ('mmskin_linear_forward', (), (64, 64, 64, 0)),
        ('mmskin_add', (), (4096, 4096)),
        ('mmskin_linear_backward', (3, 4), (64, 64, 64)),
    ],
    'linear-small-w_frozen': [
        ('mmskin_linear_forward', (), (64, 64, 64, 0)),
        ('mmskin_linear_backward', (1, 3, 4, 6), (64, 64, 64)),
    ],
    'linear-small-no_bias': [
        ('mmskin_linear_forward', (2,), (64, 64, 64, 0)),
        ('mmskin_linear_backward', (3, 4, 7), (64, 64, 64)),
    ],
    'linear_gelu-small-all': [
        ('mmskin_linear_forward', (), (64, 64, 64, 0)),
        ('mmskin_gelu_forward', (), (4096,)),
        ('mmskin_linear_gelu_backward', (), (64, 64, 64)),
    ],
    'linear_gelu-small-w_frozen': [
        ('mmskin_linear_forward', (), (64, 64, 64, 0)),
        ('mmskin_gelu_forward', (), (4096,)),
        ('mmskin_linear_gelu_backward', (1, 6), (64, 64, 64)),
    ],
    'linear-big_bf16-all': [
        ('mmskin_linear_forward_keep', (3,), (2048, 64, 64, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 64, 64)),
    ],
    'linear-big_bf16-relu': [
        ('mmskin_linear_forward_keep', (3,), (2048, 64, 64, 1)),
        ('mmskin_linear_backward_keep', (4,), (2048, 64, 64)),
    ],
    'linear-big_bf16-residual': [
        ('mmskin_linear_forward_keep', (), (2048, 64, 64, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 64, 64)),
    ],
    'linear-big_bf16-w_frozen': [
        ('mmskin_linear_forward', (), (2048, 64, 64, 0)),
        ('mmskin_linear_backward', (1, 3, 4, 6), (2048, 64, 64)),
    ],
    'linear-big_bf16-no_bias': [
        ('mmskin_linear_forward_keep', (2, 3), (2048, 64, 64, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5, 8), (2048, 64, 64)),
    ],
    'linear_gelu-big_bf16-all': [
        ('mmskin_linear_forward_keep', (3,), (2048, 64, 64, 0)),
        ('mmskin_gelu_forward', (), (131072,)),
        ('mmskin_linear_backward_keep', (3, 5), (2048, 64, 64)),
    ],
    'linear_gelu-big_bf16-w_frozen': [
        ('mmskin_linear_forward', (), (2048, 64, 64, 0)),
        ('mmskin_gelu_forward', (), (131072,)),
        ('mmskin_linear_gelu_backward', (1, 4, 6), (2048, 64, 64)),
    ],
    'linear-padded-all': [
        ('mmskin_linear_forward_keep', (3,), (2048, 96, 96, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 96, 96)),
    ],
    'linear-padded-relu': [
        ('mmskin_linear_forward_keep', (3,), (2048, 96, 96, 1)),
        ('mmskin_linear_backward_keep', (4,), (2048, 96, 96)),
    ],
    'linear-padded-residual': [
        ('mmskin_linear_forward_keep', (), (2048, 96, 96, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 96, 96)),
    ],
    'linear-padded-w_frozen': [
        ('mmskin_linear_forward', (), (2048, 96, 96, 0)),
        ('mmskin_linear_backward', (1, 3, 4, 6), (2048, 96, 96)),
    ],
    'linear-padded-no_bias': [
        ('mmskin_linear_forward_keep', (2, 3), (2048, 96, 96, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5, 8), (2048, 96, 96)),
    ],
    'linear_gelu-padded-all': [
        ('mmskin_linear_forward_keep', (3,), (2048, 96, 96, 0)),
        ('mmskin_gelu_forward', (), (196608,)),
        ('mmskin_linear_backward_keep', (3, 5), (2048, 96, 96)),
    ],
    'linear_gelu-padded-w_frozen': [
        ('mmskin_linear_forward', (), (2048, 96, 96, 0)),
        ('mmskin_gelu_forward', (), (196608,)),
        ('mmskin_linear_gelu_backward', (1, 4, 6), (2048, 96, 96)),
    ],
    'mlp-gelu-fused-bf16-2048x64-nores': [
        ('mmskin_linear_forward_keep', (3,), (2048, 64, 256, 0)),
        ('mmskin_gelu_forward_bf16', (), (2048, 256, 256)),
        ('mmskin_linear_forward_x16', (3,), (2048, 256, 64, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 256, 64)),
        ('mmskin_linear_backward_keep', (3, 5), (2048, 64, 256)),
    ],
    'mlp-gelu-fused-bf16-2048x64-res': [
        ('mmskin_linear_forward_keep', (3,), (2048, 64, 256, 0)),
        ('mmskin_gelu_forward_bf16', (), (2048, 256, 256)),
        ('mmskin_linear_forward_x16', (), (2048, 256, 64, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 256, 64)),
        ('mmskin_linear_backward_keep', (3, 5), (2048, 64, 256)),
    ],
    'mlp-gelu-fused-bf16-2048x96-nores': [
        ('mmskin_linear_forward_keep', (3,), (2048, 96, 384, 0)),
        ('mmskin_gelu_forward_bf16', (), (2048, 384, 384)),
        ('mmskin_linear_forward_x16', (3,), (2048, 384, 96, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 384, 96)),
        ('mmskin_linear_backward_keep', (3, 5), (2048, 96, 384)),
    ],
    'mlp-gelu-fused-bf16-2048x96-res': [
        ('mmskin_linear_forward_keep', (3,), (2048, 96, 384, 0)),
        ('mmskin_gelu_forward_bf16', (), (2048, 384, 384)),
        ('mmskin_linear_forward_x16', (), (2048, 384, 96, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 384, 96)),
        ('mmskin_linear_backward_keep', (3, 5), (2048, 96, 384)),
    ],
    'mlp-gelu-fallback-bf16-64x64-nores': [
        ('mmskin_linear_forward', (), (64, 64, 256, 0)),
        ('mmskin_gelu_forward', (), (16384,)),
        ('mmskin_linear_forward', (), (64, 256, 64, 0)),
        ('mmskin_linear_backward', (3, 4), (64, 256, 64)),
        ('mmskin_linear_gelu_backward', (), (64, 64, 256)),
    ],
    'mlp-gelu-fallback-bf16-64x64-res': [
        ('mmskin_linear_forward', (), (64, 64, 256, 0)),
        ('mmskin_gelu_forward', (), (16384,)),
        ('mmskin_linear_forward', (), (64, 256, 64, 0)),
        ('mmskin_add', (), (4096, 4096)),
        ('mmskin_linear_backward', (3, 4), (64, 256, 64)),
        ('mmskin_linear_gelu_backward', (), (64, 64, 256)),
    ],
    'mlp-gelu-fallback-fp32-2048x64-nores': [
        ('mmskin_linear_forward', (), (2048, 64, 256, 0)),
        ('mmskin_gelu_forward', (), (524288,)),
        ('mmskin_linear_forward', (), (2048, 256, 64, 0)),
        ('mmskin_linear_backward', (3, 4), (2048, 256, 64)),
        ('mmskin_linear_gelu_backward', (), (2048, 64, 256)),
    ],
    'mlp-gelu-fallback-fp32-2048x64-res': [
        ('mmskin_linear_forward', (), (2048, 64, 256, 0)),
        ('mmskin_gelu_forward', (), (524288,)),
        ('mmskin_linear_forward', (), (2048, 256, 64, 0)),
        ('mmskin_add', (), (131072, 131072)),
        ('mmskin_linear_backward', (3, 4), (2048, 256, 64)),
        ('mmskin_linear_gelu_backward', (), (2048, 64, 256)),
    ],
    'mlp-gelu-fused-bf16-2048x64-res-x_frozen': [
        ('mmskin_linear_forward_keep', (3,), (2048, 64, 256, 0)),
        ('mmskin_gelu_forward_bf16', (), (2048, 256, 256)),
        ('mmskin_linear_forward_x16', (), (2048, 256, 64, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 256, 64)),
        ('mmskin_linear_backward_keep', (3, 5, 6), (2048, 64, 256)),
    ],
    'mlp-star-fused-bf16-2048x64-nores': [
        ('mmskin_linear_forward_keep', (3,), (2048, 64, 256, 0)),
        ('mmskin_star_relu_forward_bf16', (), (2048, 256, 256)),
        ('mmskin_linear_forward_x16', (3,), (2048, 256, 64, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 256, 64)),
        ('mmskin_linear_star_relu_backward_keep', (), (2048, 64, 256)),
    ],
    'mlp-star-fused-bf16-2048x64-res': [
        ('mmskin_linear_forward_keep', (3,), (2048, 64, 256, 0)),
        ('mmskin_star_relu_forward_bf16', (), (2048, 256, 256)),
        ('mmskin_linear_forward_x16', (), (2048, 256, 64, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 256, 64)),
        ('mmskin_linear_star_relu_backward_keep', (), (2048, 64, 256)),
    ],
    'mlp-star-fused-bf16-2048x96-nores': [
        ('mmskin_linear_forward_keep', (3,), (2048, 96, 384, 0)),
        ('mmskin_star_relu_forward_bf16', (), (2048, 384, 384)),
        ('mmskin_linear_forward_x16', (3,), (2048, 384, 96, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 384, 96)),
        ('mmskin_linear_star_relu_backward_keep', (), (2048, 96, 384)),
    ],
    'mlp-star-fused-bf16-2048x96-res': [
        ('mmskin_linear_forward_keep', (3,), (2048, 96, 384, 0)),
        ('mmskin_star_relu_forward_bf16', (), (2048, 384, 384)),
        ('mmskin_linear_forward_x16', (), (2048, 384, 96, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 384, 96)),
        ('mmskin_linear_star_relu_backward_keep', (), (2048, 96, 384)),
    ],
    'mlp-star-fallback-bf16-64x64-nores': [
        ('mmskin_linear_forward', (), (64, 64, 256, 0)),
        ('mmskin_star_relu_forward', (), (16384,)),
        ('mmskin_linear_forward', (), (64, 256, 64, 0)),
        ('mmskin_linear_backward', (3, 4), (64, 256, 64)),
        ('mmskin_star_relu_backward', (), (16384,)),
        ('mmskin_linear_backward', (3, 4), (64, 64, 256)),
    ],
    'mlp-star-fallback-bf16-64x64-res': [
        ('mmskin_linear_forward', (), (64, 64, 256, 0)),
        ('mmskin_star_relu_forward', (), (16384,)),
        ('mmskin_linear_forward', (), (64, 256, 64, 0)),
        ('mmskin_add', (), (4096, 4096)),
        ('mmskin_linear_backward', (3, 4), (64, 256, 64)),
        ('mmskin_star_relu_backward', (), (16384,)),
        ('mmskin_linear_backward', (3, 4), (64, 64, 256)),
    ],
    'mlp-star-fallback-fp32-2048x64-nores': [
        ('mmskin_linear_forward', (), (2048, 64, 256, 0)),
        ('mmskin_star_relu_forward', (), (524288,)),
        ('mmskin_linear_forward', (), (2048, 256, 64, 0)),
        ('mmskin_linear_backward', (3, 4), (2048, 256, 64)),
        ('mmskin_star_relu_backward', (), (524288,)),
        ('mmskin_linear_backward', (3, 4), (2048, 64, 256)),
    ],
    'mlp-star-fallback-fp32-2048x64-res': [
        ('mmskin_linear_forward', (), (2048, 64, 256, 0)),
        ('mmskin_star_relu_forward', (), (524288,)),
        ('mmskin_linear_forward', (), (2048, 256, 64, 0)),
        ('mmskin_add', (), (131072, 131072)),
        ('mmskin_linear_backward', (3, 4), (2048, 256, 64)),
        ('mmskin_star_relu_backward', (), (524288,)),
        ('mmskin_linear_backward', (3, 4), (2048, 64, 256)),
    ],
    'mlp-star-fused-bf16-2048x64-res-x_frozen': [
        ('mmskin_linear_forward_keep', (3,), (2048, 64, 256, 0)),
        ('mmskin_star_relu_forward_bf16', (), (2048, 256, 256)),
        ('mmskin_linear_forward_x16', (), (2048, 256, 64, 0)),
        ('mmskin_linear_backward_keep', (3, 4, 5), (2048, 256, 64)),
        ('mmskin_linear_star_relu_backward_keep', (6,), (2048, 64, 256)),
    ],
    'mlp-star-hidden262-bf16-2048x65-nores': [
        ('mmskin_linear_forward', (), (2048, 65, 262, 0)),
        ('mmskin_star_relu_forward', (), (536576,)),
        ('mmskin_linear_forward', (), (2048, 262, 65, 0)),
        ('mmskin_linear_backward', (3, 4), (2048, 262, 65)),
        ('mmskin_star_relu_backward', (), (536576,)),
        ('mmskin_linear_backward', (3, 4), (2048, 65, 262)),
    ],
    'star_relu': [
        ('mmskin_star_relu_forward', (), (111,)),
        ('mmskin_star_relu_backward', (), (111,)),
    ],
    'gelu': [
        ('mmskin_gelu_forward', (), (111,)),
        ('mmskin_gelu_backward', (), (111,)),
    ],
    'gelu_tanh': [
        ('mmskin_gelu_tanh_forward', (), (111,)),
        ('mmskin_gelu_tanh_backward', (), (111,)),
    ],
    'dw7_star-grad_s_only': [
        ('mmskin_dw7_star_forward', (), (1, 7, 7, 8)),
        ('mmskin_dw7_star_backward', (), (1, 7, 7, 8)),
    ],
    'dw7_star-grad_b_only': [
        ('mmskin_dw7_star_forward', (), (1, 7, 7, 8)),
        ('mmskin_dw7_star_backward', (), (1, 7, 7, 8)),
    ],
}
