"""-m gpu: every route of csrc/linear.hip (linear_path: LIN_SMALL / LIN_BIG_F32 / LIN_BIG_BF16 / LIN_PADDED_BF16) at the shapes where the
route, or a kernel choice inside it, changes -- against torch on the CPU in float64 on the same inputs.  Every case first asks the
library which route it takes (mmskin_linear_route), so a change of the predicates cannot quietly move a case elsewhere.

Error metric: gpu_util.rel_err (worst element over the rms of the fp64 reference) unless a bound says 'l2' (relative L2 norm, the
metric of the existing test the bound comes from).  Bounds:
  LIN_SMALL        2e-5 rel_err   (test_gpu_kernels.test_linear)
  LIN_BIG_F32      2e-4 rel_err   (the exact-f32 conv kernels in test_gpu_kernels.test_conv_forward_backward)
  LIN_BIG_BF16     y: 2e-2 rel_err (test_gpu_flash_attention.test_flash_bf16_tensors_and_lane_ops, y32) and 1e-2 l2
                   (test_gpu_kernels.test_linear_bf16_operand_mode) -- the GEMM epilogue hands y over rounded to bf16, so its worst
                   element is half a bf16 ulp of the largest |y| (measured 1.0e-2 .. 1.6e-2 of the rms) while its l2 error is ~1e-3;
                   dW / db: 1e-2 (test_linear_bf16_operand_mode; that test bounds the relative L2 norm, here the same figure bounds
                   rel_err, which is never smaller than it).  dx: 1e-2 l2 (the same test) -- the dgrad GEMM also hands dx over
                   rounded to bf16, and no existing test bounds its worst element, so that bound is twice the rel_err of
                   tests/bf16_emulation.py's dx (bf16(bf16(g) bf16(w)) in CPU fp32) against fp64 on the same inputs, computed per
                   case.  Measured emulation figures, no activation / ReLU: (2048, 64, 64) 1.46e-2 / 1.10e-2, (2049, 64, 128)
                   1.09e-2 / 1.47e-2, (2500, 192, 64) 1.36e-2 / 1.78e-2, (4120, 128, 320) 9.9e-3 / 1.41e-2, (20992, 512, 512)
                   1.56e-2 / 1.09e-2; the kernel's figures were the same to three digits.
  LIN_PADDED_BF16  2.5e-2 y, 2e-2 dx, 2e-2 dW, 1e-4 db rel_err (test_gpu_flash_attention.test_linear_bf16_padded_widths)
  GELU on the two bf16 routes: 2e-2 l2 on all four (test_gpu_davit_ops.test_linear_gelu_backward_in_one_call)
In bf16 mode x, w and dy are bf16-representable, so operand rounding is not part of the error.  With ReLU the gradient reference uses
the mask y > 0 of the output under test (as test_linear_bf16_padded_widths does), and every element where that mask differs from the
fp64 one must have a pre-activation within the route's y bound of zero.

Calls that go to the C ABI directly write into NaN-filled outputs with 64 sentinel elements behind them: a dropped tail leaves a NaN,
an overrun changes a sentinel -- neither of which a torch.empty output would show."""
import itertools

import pytest
import torch

import conv_route_cases as CR
from gpu_util import DEV, linear_mode, rel_err
from linear_route_cases import BIG_BF16, BIG_F32, PADDED, ROUTE_CASES, SMALL, case_id, make_inputs, reference
from mmskin import _lib, ops
from mmskin._lib import call, ptr, stream

pytestmark = pytest.mark.gpu

ACTS = ("none", "relu", "gelu")
Y, DX, DW, DB = range(4)
NAMES = ("y", "dx", "dW", "db")


def bounds(route, act):
    """(metric, (y, dx, dW, db)) -- see the module docstring for where each figure comes from"""
    if route == SMALL:
        return "max", (2e-5,) * 4
    if route == BIG_F32:
        return "max", (2e-4,) * 4
    if act == "gelu":
        return "l2", (2e-2,) * 4
    if route == BIG_BF16:   # dx: l2; its rel_err bound comes from the emulation (emulated_dx_bound)
        return "max", (2e-2, 1e-2, 1e-2, 1e-2)
    return "max", (2.5e-2, 2e-2, 2e-2, 1e-4)


def check_y(label, got, want, route, act):
    """y against its route's bound(s): LIN_BIG_BF16 without GELU carries an l2 bound next to the rel_err one"""
    metric, tol = bounds(route, act)
    check(f"{label} y", got, want, metric, tol[Y])
    if route == BIG_BF16 and act != "gelu":
        check(f"{label} y", got, want, "l2", 1e-2)


def emulated_dx_bound(w, g, want_dx):
    """2 x the rel_err of the bf16-operand emulation's dx for the gradient g (fp32, CPU) against the fp64 dx"""
    from bf16_emulation import _Bf16Linear
    xe = torch.zeros(g.shape[0], w.shape[1], requires_grad=True)
    _Bf16Linear.apply(xe, w, None).backward(g)
    return 2.0 * rel_err(xe.grad, want_dx)


def l2_err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm()) / (float(want.norm()) + 1e-30)


def check(label, got, want, metric, tol):
    """prints the figure, then asserts it.  A reference that is zero everywhere (a ReLU that passes nothing at M = 1) must be met exactly."""
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{label}: non-finite values"
    if float(want.abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0, label
        return
    err = rel_err(got, want) if metric == "max" else l2_err(got, want)
    print(f"{label}: {metric} {err:.3e} (bound {tol:.1e})")
    assert err < tol, f"{label}: {metric} error {err:.3e} >= {tol:.1e}"


def assert_route(M, K, N, route):
    got = _lib.load().mmskin_linear_route(M, K, N)
    assert got == route, f"({M}, {K}, {N}) in {ops.get_linear_dtype()} mode takes route {got}, the case was written for route {route}"
    if route in (BIG_F32, BIG_BF16):
        # ... and the conv-GEMM family behind it: these shapes stay on the 128-row tile with the light epilogue (bias; bf16 operands store
        # fp32), below the pipelined / 256 x 256 thresholds that tests/conv_route_cases.py pins (K < 768 or fewer than 192 tiles of 256
        # columns); two LDS stages up to 640 workgroups, one above (only 20992 x 512 x 512: 164 x 4 = 656)
        eb, flags = (CR.F32, CR.BIAS) if route == BIG_F32 else (CR.BF16, CR.BIAS | CR.OUT_F32)
        bn = 128 if N % 128 == 0 else 64
        conv = CR.route(_lib.load(), CR.FWD, CR.linear(M, K, N), eb, flags)
        assert conv[:6] == (CR.CG_TILE128, 128, 128, bn, 1 if -(-M // 128) * (N // bn) > 640 else 2, 2), conv


def run_linear(x, w, b, dy, act, grads=(True, True, True)):
    """ops.linear / ops.linear_gelu forward + backward on the GPU; returns (y, dx, dW, db) on the CPU, None where no gradient was asked"""
    xd = x.to(DEV).requires_grad_(grads[0])
    wd = w.to(DEV).requires_grad_(grads[1])
    bd = None if b is None else b.to(DEV).requires_grad_(grads[2])
    y = ops.linear_gelu(xd, wd, bd) if act == "gelu" else ops.linear(xd, wd, bd, act == "relu")
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.detach().cpu()
    return cpu(y), cpu(xd.grad), cpu(wd.grad), cpu(None if bd is None else bd.grad)


def check_against_fp64(label, outs, x, w, b, dy, act, route):
    metric, tol = bounds(route, act)
    mask = (outs[Y] > 0) if act == "relu" else None
    z, *want = reference(x, w, b, dy, act, mask)
    if act == "relu":   # a sign the kernel and fp64 disagree on must belong to a pre-activation that is zero to within the y bound
        flipped = mask != (z > 0)
        if bool(flipped.any()):
            lim = tol[Y] * float(z.pow(2).mean().sqrt())
            assert float(z[flipped].abs().max()) <= lim, f"{label}: ReLU mask differs from fp64 where |z| > {lim:.2e}"
    check_y(label, outs[Y], want[Y].float(), route, act)
    for i in (DX, DW, DB):
        if outs[i] is None:
            continue
        if i == DX and route == BIG_BF16 and act != "gelu":
            g = dy * mask.float() if act == "relu" else dy
            check(f"{label} dx", outs[DX], want[DX].float(), "l2", tol[DX])
            check(f"{label} dx", outs[DX], want[DX].float(), "max", emulated_dx_bound(w, g, want[DX]))
            continue
        check(f"{label} {NAMES[i]}", outs[i], want[i].float(), metric, tol[i])


# ---------------------------------------------------------------------------------------------------------------- a. route matrix
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", ROUTE_CASES, ids=case_id)
def test_route_matrix(case, act):
    """y, dx, dW, db of every row of the route table, for no activation, fused ReLU and Linear -> GELU; run twice: the reductions of
    linear.hip (split-K slices, column-sum partial rows, weight-gradient slabs) are summed in a fixed order, so the results are equal
    bit for bit."""
    mode, M, K, N, route = case
    x, w, b, dy = make_inputs(mode, M, K, N)
    with linear_mode(mode):
        assert_route(M, K, N, route)
        outs = run_linear(x, w, b, dy, act)
        again = run_linear(x, w, b, dy, act)
    check_against_fp64(f"{case_id(case)} {act}", outs, x, w, b, dy, act, route)
    for i in range(4):
        assert torch.equal(outs[i], again[i]), f"{NAMES[i]} differs between two runs of the same call"


# ---------------------------------------------------------------------------------------------------------------- C ABI with sentinels
GUARD = 64
GUARD_VALUE = -12352.0   # bf16-representable, far from anything a test computes


class Guarded:
    """an output of n elements, NaN-filled, with GUARD sentinel elements behind it"""

    def __init__(self, n, dtype=torch.float32):
        self.n = n
        self.buf = torch.full((n + GUARD,), float("nan"), dtype=dtype, device=DEV)
        self.buf[n:] = GUARD_VALUE
        self.out = self.buf[:n]

    def result(self, label, shape):
        torch.cuda.synchronize()
        host = self.buf.cpu()
        assert bool((host[self.n:] == GUARD_VALUE).all()), f"{label}: wrote past its {self.n} elements"
        nan = torch.isnan(host[:self.n])
        assert not bool(nan.any()), f"{label}: {int(nan.sum())} of {self.n} elements never written (first at {int(nan.nonzero()[0])})"
        return host[:self.n].reshape(shape)


# ---------------------------------------------------------------------------------------------------------------- b. split-K on / off
@pytest.mark.parametrize("bias,relu", [(False, 0), (True, 0), (False, 1)])
def test_forward_split_k_on_and_off(bias, relu):
    """gemm_f32: K >= 4096 && tiles < 256 && !bias && !relu.  (8, 5000, 40) has 2 output tiles: without bias the forward runs 10 K
    slices into scratch + split_reduce_kernel; a bias or a ReLU turns that off and one workgroup per tile walks all 5000."""
    M, K, N = 8, 5000, 40
    x, w, b, _ = make_inputs("fp32", M, K, N)
    with linear_mode("fp32"):
        assert_route(M, K, N, SMALL)
        y = Guarded(M * N)
        xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV) if bias else None
        call("mmskin_linear_forward", ptr(xd), ptr(wd), ptr(bd), ptr(y.out), M, K, N, relu, stream())
        got = y.result("linear_forward", (M, N))
    _, want = reference(x, w, b if bias else None, None, "relu" if relu else "none")
    check(f"split-K forward bias={bias} relu={relu}", got, want.float(), "max", 2e-5)


def test_dx_split_k():
    """gemm_f32 from linear_backward_impl's dx: (4096, 32, 4100) contracts over N = 4100 >= 4096 with 128 output tiles -> 4 K slices"""
    M, K, N = 4096, 32, 4100
    x, w, b, dy = make_inputs("fp32", M, K, N)
    with linear_mode("fp32"):
        assert_route(M, K, N, SMALL)
        dx = Guarded(M * K)
        dyd, wd = dy.to(DEV), w.to(DEV)
        call("mmskin_linear_backward", ptr(dyd), None, ptr(wd), None, None, ptr(dx.out), None, None, M, K, N, stream())
        got = dx.result("linear_backward dx", (M, K))
    check("split-K dx", got, (dy.double() @ w.double()).float(), "max", 2e-5)


# ---------------------------------------------------------------------------------------------------------------- c. partial gradients
PARTIAL_SHAPES = [
    ("fp32", 33, 130, 31, SMALL),      # linear_bwd_small_kernel: n_dx / n_dw / n_db block ranges, each of which may be empty
    ("fp32", 4100, 36, 30, SMALL),     # separate gemm_f32 launches + colsum
    ("fp32", 2049, 64, 128, BIG_F32),
    ("bf16", 2049, 64, 128, BIG_BF16),   # need_w False: no kept bf16 operand; db None: cvt_operand instead of colsum4
    ("bf16", 2048, 64, 72, PADDED),
]
GRAD_SETS = [(gx, gw, gb, True) for gx, gw, gb in itertools.product((False, True), repeat=3) if gx or gw or gb] + \
            [(gx, gw, False, False) for gx, gw in itertools.product((False, True), repeat=2) if gx or gw]


@pytest.mark.parametrize("act", ["none", "gelu"])
@pytest.mark.parametrize("case", PARTIAL_SHAPES, ids=case_id)
def test_partial_gradients(case, act):
    """every subset of requires_grad over (x, w, b), and b = None: the values asked for, None for the rest"""
    mode, M, K, N, route = case
    x, w, b, dy = make_inputs(mode, M, K, N)
    with linear_mode(mode):
        assert_route(M, K, N, route)
        for gx, gw, gb, has_b in GRAD_SETS:
            bb = b if has_b else None
            outs = run_linear(x, w, bb, dy, act, (gx, gw, gb))
            label = f"{case_id(case)} {act} grads x={gx} w={gw} b={gb if has_b else 'absent'}"
            for i, asked in ((DX, gx), (DW, gw), (DB, gb and has_b)):
                assert (outs[i] is not None) == asked, f"{label}: {NAMES[i]} {'missing' if asked else 'present'}"
            check_against_fp64(label, outs, x, w, bb, dy, act, route)


# ---------------------------------------------------------------------------------------------------------------- d. forward_ex
def bf16_ulp(v):
    """spacing of bf16 (8 significant bits) at |v|"""
    return torch.pow(2.0, torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 7)


EX_SHAPES = [
    (2048, 64, 64, BIG_BF16),     # linear_big_bf16_ex: bf16 tensors straight in and out of the GEMM
    (2048, 64, 72, PADDED),       # not LIN_BIG_BF16 -> the fallback, whose fp32 entry point takes the padded route
    (96, 64, 40, SMALL),          # the fallback shape test_flash_bf16_tensors_and_lane_ops has: M*K and M*N multiples of 4
    (3, 5, 7, SMALL),             # M*K = 15, M*N = 21: both flat conversions end in a tail
    (5, 768, 6, SMALL),           # M*K % 4 == 0, M*N = 30: the output conversion's tail only
    (7, 9, 3, SMALL),             # M*K = 63, M*N = 21
    (1, 3, 1, SMALL),             # fewer than 4 elements either way: no whole chunk at all
]


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("y_bf16", [False, True])
@pytest.mark.parametrize("x_bf16", [False, True])
@pytest.mark.parametrize("shape", EX_SHAPES, ids=lambda s: "x".join(map(str, s[:3])))
def test_forward_ex_dtype_pairs(shape, x_bf16, y_bf16, act):
    """mmskin_linear_forward_ex with fp32 / bf16 tensors at either end, bf16-operand mode.  An fp32 result meets the route's bound; a
    bf16 result is, element by element, within one bf16 ulp of the fp64 value plus the route's bound (of the reference rms)."""
    M, K, N, route = shape
    x, w, b, _ = make_inputs("bf16", M, K, N)
    name = "gelu" if act == 2 else "none"
    metric, tol = bounds(route, name)
    with linear_mode("bf16"):
        assert_route(M, K, N, route)
        xd = x.to(DEV).bfloat16() if x_bf16 else x.to(DEV)
        wd, bd = w.to(DEV), b.to(DEV)
        y = Guarded(M * N, torch.bfloat16 if y_bf16 else torch.float32)
        call("mmskin_linear_forward_ex", ptr(xd), int(x_bf16), ptr(wd), ptr(bd), ptr(y.out), int(y_bf16), M, K, N, act, stream())
        got = y.result(f"linear_forward_ex x_bf16={x_bf16} y_bf16={y_bf16}", (M, N)).double()
    _, want = reference(x, w, b, None, name)
    label = f"forward_ex {M}x{K}x{N} x_bf16={x_bf16} y_bf16={y_bf16} act={act}"
    if not y_bf16:
        check_y(label, got, want, route, name)
        return
    rms = float(want.pow(2).mean().sqrt())
    excess = ((got - want).abs() - bf16_ulp(want) - tol[Y] * rms).max()
    print(f"{label}: worst |error| - (ulp + bound) = {float(excess):.3e}")
    assert float(excess) <= 0.0, f"{label}: an element is {float(excess):.3e} past one bf16 ulp + {tol[Y]:.1e} of the rms"


# ---------------------------------------------------------------------------------------------------------------- e. bmm
@pytest.mark.parametrize("Dh", [8, 64, 80])
@pytest.mark.parametrize("L", [1, 31, 33, 129, 160, 257])
@pytest.mark.parametrize("batch", [1, 3, 24])
def test_bmm_attention_stride_patterns(batch, L, Dh):
    """mmskin_bmm with the six calls of ops.LongAttentionFn (QK^T, PV, and the four gradient products: three of gemm_f32_kernel's
    four A_KC / B_KC instantiations), plus the fourth instantiation (A walked along rows, B along k) -- against torch.bmm in fp64.
    batch == 1 takes gemm_f32 without blockIdx.z."""
    g = torch.Generator().manual_seed(batch * 1000 + L * 10 + Dh)
    q, k, v, dO = (torch.randn(batch, L, Dh, generator=g) for _ in range(4))
    p, ds = (torch.randn(batch, L, L, generator=g) for _ in range(2))
    T = lambda t: t.double().transpose(1, 2)
    LD, LL = L * Dh, L * L
    # (name, a, b, M, N, K, sam, sak, sab, sbn, sbk, sbb, ldc, scb, reference)
    calls = [
        ("scores = q k^T", q, k, L, L, Dh, Dh, 1, LD, Dh, 1, LD, L, LL, q.double() @ T(k)),
        ("o = p v", p, v, L, Dh, L, L, 1, LL, 1, Dh, LD, Dh, LD, p.double() @ v.double()),
        ("dv = p^T dO", p, dO, L, Dh, L, 1, L, LL, 1, Dh, LD, Dh, LD, T(p) @ dO.double()),
        ("dp = dO v^T", dO, v, L, L, Dh, Dh, 1, LD, Dh, 1, LD, L, LL, dO.double() @ T(v)),
        ("dq = ds k", ds, k, L, Dh, L, L, 1, LL, 1, Dh, LD, Dh, LD, ds.double() @ k.double()),
        ("dk = ds^T q", ds, q, L, Dh, L, 1, L, LL, 1, Dh, LD, Dh, LD, T(ds) @ q.double()),
        ("p^T p^T (A rows-first, B k-first)", p, ds, L, L, L, 1, L, LL, L, 1, LL, L, LL, T(p) @ T(ds)),
    ]
    for name, a, b, M, N, K, sam, sak, sab, sbn, sbk, sbb, ldc, scb, want in calls:
        c = Guarded(batch * M * N)
        ad, bd = a.to(DEV), b.to(DEV)
        ops._bmm(ad, bd, c.out, batch, M, N, K, sam, sak, sab, sbn, sbk, sbb, ldc, scb)
        got = c.result(f"bmm {name}", (batch, M, N))
        check(f"bmm batch={batch} L={L} Dh={Dh} {name}", got, want.float(), "max", 2e-5)


def test_bmm_single_batch_split_k():
    """batch == 1 goes through gemm_f32's split-K test like any Linear: K = 4100 with one output tile"""
    g = torch.Generator().manual_seed(9)
    M, N, K = 20, 24, 4100
    a, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    c = Guarded(M * N)
    ad, bd = a.to(DEV), b.to(DEV)
    ops._bmm(ad, bd, c.out, 1, M, N, K, K, 1, 0, K, 1, 0, N, 0)
    check("bmm batch=1 split-K", c.result("bmm", (M, N)), (a.double() @ b.double().T).float(), "max", 2e-5)


# ---------------------------------------------------------------------------------------------------------------- f. colsum
@pytest.mark.parametrize("M,N", [
    (2047, 30),     # colsum: M >= 2048 fails -> one colsum_kernel row group (G = 1)
    (2048, 30),     # colsum: N % 4 != 0 -> colsum_kernel over G = 8 row groups + split_reduce_kernel
    (40000, 6),     # colsum: G capped at 128 (M / 256 = 156), 313 rows per group, the last group ragged
    (2048, 96),     # colsum4_plan: CW = 24 chunk columns, 10 row lanes, 16 idle threads per block
    (5003, 100),    # colsum4_plan: CW = 25, ragged last row block
    (2048, 4),      # colsum4_plan: CW = 1, 256 row lanes
    (2048, 132),    # colsum4_plan: ncol4 = 33 > 32 -> two column groups, the second with one live chunk column (added)
])
def test_colsum(M, N):
    x = torch.randn(M, N, generator=torch.Generator().manual_seed(M + N))
    out = Guarded(N)
    xd = x.to(DEV)
    call("mmskin_colsum", ptr(xd), ptr(out.out), M, N, stream())
    check(f"colsum {M}x{N}", out.result("colsum", (N,)), x.double().sum(0).float(), "max", 2e-5)


# ---------------------------------------------------------------------------------------------------------------- g. scratch regrowth
def test_scratch_regrowth_keeps_small_results():
    """head_scratch starts at 8 MB and is freed and reallocated when a call needs more.  Small calls that use it (a split-K forward, a
    padded bf16 Linear forward + backward) give the same bits before and after (20992, 512, 512) in bf16 mode, whose operands alone
    are over 8 MB -- and that large call is itself right."""
    xs, ws, _, _ = make_inputs("fp32", 8, 5000, 40)
    xp, wp, bp, dyp = make_inputs("bf16", 2048, 64, 72)

    def small():
        with linear_mode("fp32"):
            assert_route(8, 5000, 40, SMALL)
            with torch.no_grad():
                ysplit = ops.linear(xs.to(DEV), ws.to(DEV)).cpu()
        with linear_mode("bf16"):
            assert_route(2048, 64, 72, PADDED)
            return (ysplit,) + run_linear(xp, wp, bp, dyp, "none")

    before = small()
    M, K, N = 20992, 512, 512
    x, w, b, dy = make_inputs("bf16", M, K, N)
    with linear_mode("bf16"):
        assert_route(M, K, N, BIG_BF16)
        big = run_linear(x, w, b, dy, "none")
    after = small()
    for i, (p, q) in enumerate(zip(before, after)):
        assert torch.equal(p, q), f"small result {i} changed after the scratch buffer grew"
    check_against_fp64("20992x512x512 bf16", big, x, w, b, dy, "none", BIG_BF16)
    check_against_fp64("2048x64x72 bf16", before[1:], xp, wp, bp, dyp, "none", PADDED)


# ---------------------------------------------------------------------------------------------------------------- residual epilogue
@pytest.mark.parametrize("case", [
    ("bf16", 2049, 64, 128, BIG_BF16),   # linear_forward_impl: res && N % 128 == 0 -> the residual rides the GEMM epilogue
    ("bf16", 2500, 192, 64, BIG_BF16),   # linear_forward_impl: N % 128 != 0 -> add4_inplace_kernel after the GEMM
    ("bf16", 2048, 64, 72, PADDED),      # bf16_unpad_bias_act_kernel adds the residual while un-padding
], ids=case_id)
def test_fused_residual(case):
    """y = residual + x w^T + b through ops.linear(residual=...): value, the Linear's gradients, and d(residual) = dy exactly"""
    mode, M, K, N, route = case
    x, w, b, dy = make_inputs(mode, M, K, N)
    res = torch.randn(M, N, generator=torch.Generator().manual_seed(M + N))
    with linear_mode(mode):
        assert_route(M, K, N, route)
        xd, wd, bd, rd = (t.to(DEV).requires_grad_(True) for t in (x, w, b, res))
        y = ops.linear(xd, wd, bd, residual=rd)
        y.backward(dy.to(DEV))
        torch.cuda.synchronize()
    metric, tol = bounds(route, "none")
    _, y0, dx, dw, db = reference(x, w, b, dy, "none")
    # the y bound is a figure for x w^T + b, so the residual is taken off again (in fp64) instead of entering the scale
    check_y(f"{case_id(case)} residual (y - res)", y.detach().cpu().double() - res.double(), y0, route, "none")
    if route == BIG_BF16:
        check(f"{case_id(case)} residual dx", xd.grad.cpu(), dx.float(), "l2", tol[DX])
        check(f"{case_id(case)} residual dx", xd.grad.cpu(), dx.float(), "max", emulated_dx_bound(w, dy, dx))
    else:
        check(f"{case_id(case)} residual dx", xd.grad.cpu(), dx.float(), metric, tol[DX])
    check(f"{case_id(case)} residual dW", wd.grad.cpu(), dw.float(), metric, tol[DW])
    check(f"{case_id(case)} residual db", bd.grad.cpu(), db.float(), metric, tol[DB])
    assert torch.equal(rd.grad.cpu(), dy), "d(residual) is dy"
