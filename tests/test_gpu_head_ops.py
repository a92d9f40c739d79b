"""-m gpu: the fusion-head and encoder-glue kernels of csrc/head.hip, op by op, against plain PyTorch in fp64 on the CPU (autograd for the
backward) -- the element-wise gates / GELUs / add / LayerScale / StarReLU / concat, dropout, token mean, the MD-Net fusion pool, the
custom-CNN pooling and direct conv, the embedding gather, and the row softmax and mixed-output LayerNorm entries that have no wrapper.

Sizes.  Every element-wise entry launches at most 4096 blocks of 256 threads and strides over the rest, so N_BIG = 4097 * 256 + 3 is the
smallest size at which a thread takes a second trip of its loop (and it is a multiple of neither 4, 64 nor 256); 1 / 255 / 257 sit around
one block.  The per-plane kernels get planes below, at and off a multiple of the 64-lane wave and plane counts off a multiple of 4.

Tolerances are the head-operator bounds of test_gpu_kernels.py on rel_err = max|got - want| / rms(want): 2e-5 for element-wise fp32
ops, 1e-4 for anything with a reduction (summation order differs).  Gathers, copies and masks are compared bit for bit.  Every case
appends its measured errors to the parity report that the conv tests write (test_gpu_abn.REPORT)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import DEV, rel_err
from mmskin import _lib, ops
from mmskin._lib import call, ptr, stream
from test_gpu_abn import REPORT   # one report file for all parity tests

pytestmark = pytest.mark.gpu

EW_TOL, RED_TOL = 2e-5, 1e-4
N_BIG = 4097 * 256 + 3
EW_SIZES = [1, 255, 257, N_BIG]
F32_MIN = torch.finfo(torch.float32).min


def _report(test, case, errs):
    rec = dict(test="head_ops." + test, case=case, **errs)
    print(rec)
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(json.dumps(rec) + "\n")
    return rec


def _check(test, case, pairs):
    """pairs: name -> (got, want, tol).  Measures every pair, writes the record, then asserts shape, finiteness and the bound (tol None:
    the figure is recorded only)."""
    errs = {k: rel_err(g, w) for k, (g, w, _) in pairs.items()}
    rec = _report(test, case, errs)
    for k, (g, w, tol) in pairs.items():
        assert tuple(g.shape) == tuple(w.shape), (k, g.shape, w.shape)
        assert bool(torch.isfinite(g).all()), (k, "not finite", rec)
        assert tol is None or errs[k] < tol, (k, errs[k], tol, rec)


def _run(fn, ref_fn, inputs, dy):
    """fn on the device in fp32 and ref_fn on the CPU in fp64 on the same inputs, both backward with dy: (y, y_ref, grads, ref grads)."""
    ref_in = [t.double().requires_grad_(True) for t in inputs]
    yr = ref_fn(*ref_in)
    yr.backward(dy.double())
    dev_in = [t.to(DEV).requires_grad_(True) for t in inputs]
    yd = fn(*dev_in)
    yd.backward(dy.to(DEV))
    torch.cuda.synchronize()
    return yd.detach().cpu(), yr.detach(), [d.grad.cpu() for d in dev_in], [r.grad for r in ref_in]


def _put(t, vals):
    """the edge values at the front of t when it has room for them"""
    if t.numel() >= len(vals):
        t.view(-1)[:len(vals)] = torch.tensor(vals, dtype=t.dtype)
    return t


# ------------------------------------------------------------------------------- 1. element-wise family
SAT = [30.0, -30.0, 100.0, -100.0]     # positions 0..3 of the gate pre-activation: fp32 sigmoid is exactly 1 at +30 / +100, exactly 0 at -100


@pytest.mark.parametrize("n", EW_SIZES)
def test_sigmoid_gate(n):
    g = torch.Generator().manual_seed(100 + n)
    z, v, dy = _put(torch.randn(n, generator=g) * 2, SAT), torch.randn(n, generator=g), torch.randn(n, generator=g)
    y, yr, (dz, dv), (dzr, dvr) = _run(ops.sigmoid_gate, lambda z, v: torch.sigmoid(z) * v, [z, v], dy)
    _check("sigmoid_gate", [n], dict(y=(y, yr, EW_TOL), dz=(dz, dzr, EW_TOL), dv=(dv, dvr, EW_TOL)))
    if n >= len(SAT):
        one, zero = [0, 2], [3]
        assert torch.equal(y[one], v[one]) and torch.equal(dv[one], dy[one]) and bool((y[zero] == 0).all() and (dv[zero] == 0).all())
        assert bool((dz[[0, 2, 3]] == 0).all())


@pytest.mark.parametrize("n", EW_SIZES)
def test_gated_mix(n):
    g = torch.Generator().manual_seed(200 + n)
    z = _put(torch.randn(n, generator=g) * 2, SAT)
    a, q, dy = (torch.randn(n, generator=g) for _ in range(3))
    ref = lambda z, a, q: torch.sigmoid(z) * a + (1 - torch.sigmoid(z)) * q
    y, yr, (dz, da, dq), (dzr, dar, dqr) = _run(ops.gated_mix, ref, [z, a, q], dy)
    _check("gated_mix", [n], dict(y=(y, yr, EW_TOL), dz=(dz, dzr, EW_TOL), da=(da, dar, EW_TOL), dq=(dq, dqr, EW_TOL)))
    if n >= len(SAT):
        one, zero = [0, 2], [3]
        assert torch.equal(y[one], a[one]) and torch.equal(da[one], dy[one]) and bool((dq[one] == 0).all())
        assert torch.equal(y[zero], q[zero]) and torch.equal(dq[zero], dy[zero]) and bool((da[zero] == 0).all())
        assert bool((dz[[0, 2, 3]] == 0).all())


@pytest.mark.parametrize("n", EW_SIZES)
def test_metablock_gate(n):
    """sigmoid(tanh(V t1) + t2): t2 carries the saturating values, and V t1 = +-100 at positions 4, 5 saturates the tanh (1 - u^2 = 0)."""
    g = torch.Generator().manual_seed(300 + n)
    V, t1, t2, dy = (torch.randn(n, generator=g) for _ in range(4))
    _put(t2, SAT)
    if n >= 6:
        V[4], V[5], t1[4], t1[5] = 100.0, -100.0, 1.0, 1.0
    ref = lambda V, t1, t2: torch.sigmoid(torch.tanh(V * t1) + t2)
    y, yr, (dV, d1, d2), (dVr, d1r, d2r) = _run(ops.metablock_gate, ref, [V, t1, t2], dy)
    _check("metablock_gate", [n], dict(y=(y, yr, EW_TOL), dV=(dV, dVr, EW_TOL), dt1=(d1, d1r, EW_TOL), dt2=(d2, d2r, EW_TOL)))
    if n >= 6:
        assert bool((y[[0, 2]] == 1).all() and (y[3] == 0))
        for d in (dV, d1, d2):
            assert bool((d[[0, 2, 3]] == 0).all())
        assert bool((dV[[4, 5]] == 0).all() and (d1[[4, 5]] == 0).all())     # through the saturated tanh


GELU_EDGES = [0.0, 10.0, -10.0, 40.0, -40.0, 6.0, -6.0]


@pytest.mark.parametrize("n", EW_SIZES)
@pytest.mark.parametrize("flavour", ["gelu", "gelu_tanh"])
def test_gelu(flavour, n):
    """x in [-6, 6] plus {0, +-10, +-40}.  The far tails are +-40: there the derivative is exactly 1 / 0 in fp32 for both flavours (at -10
    the exact erf derivative is -7.7e-22, not 0, and is compared with the reference like every other point).  The backward of
    ops.gelu is mmskin_gelu_backward."""
    g = torch.Generator().manual_seed(400 + n)
    x, dy = _put(torch.rand(n, generator=g) * 12 - 6, GELU_EDGES), torch.randn(n, generator=g)
    fn, ref = (ops.gelu, F.gelu) if flavour == "gelu" else (ops.gelu_tanh, lambda t: F.gelu(t, approximate="tanh"))
    y, yr, (dx,), (dxr,) = _run(fn, ref, [x], dy)
    _check(flavour, [n], dict(y=(y, yr, EW_TOL), dx=(dx, dxr, EW_TOL)))
    if n >= len(GELU_EDGES):
        assert bool(dx[3] == dy[3]) and bool(dx[4] == 0) and bool(y[3] == 40) and bool(y[4] == 0) and bool(y[0] == 0)


@pytest.mark.parametrize("n", EW_SIZES)
def test_add_same_shape(n):
    g = torch.Generator().manual_seed(500 + n)
    a, b, dy = (torch.randn(n, generator=g) for _ in range(3))
    y, yr, (da, db), (dar, dbr) = _run(ops.add, lambda a, b: a + b, [a, b], dy)
    _check("add", [n, n], dict(y=(y, yr, EW_TOL), da=(da, dar, EW_TOL), db=(db, dbr, EW_TOL)))


@pytest.mark.parametrize("ashape,bshape", [((3, 197, 40), (197, 40)), ((N_BIG,), (1,))])
def test_add_broadcast(ashape, bshape):
    """b broadcast over a's leading dimension (position embeddings); nb = 1 is the degenerate stride.  db is a sum over that dimension."""
    g = torch.Generator().manual_seed(510 + len(ashape))
    a, b, dy = torch.randn(ashape, generator=g), torch.randn(bshape, generator=g), torch.randn(ashape, generator=g)
    y, yr, (da, db), (dar, dbr) = _run(ops.add, lambda a, b: a + b, [a, b], dy)
    _check("add_broadcast", [list(ashape), list(bshape)], dict(y=(y, yr, EW_TOL), da=(da, dar, EW_TOL), db=(db, dbr, RED_TOL)))


# C = 1 / 40 / 768 and the LayerScale width 384 with 2731 rows (> 4096 * 256 elements).  768 = 3 * 256, so no row count keeps that total off
# a multiple of 256: 7 rows give an odd number of blocks; the other totals (257, 1480, 1 048 704 + ... ) are off it.
@pytest.mark.parametrize("rows,C", [(257, 1), (37, 40), (7, 768), (2731, 384)])
def test_scale_add(rows, C):
    """x + gamma[c] b.  db = dy gamma[c] is mmskin_scale_mul per channel; dgamma = colsum(dy b) is its element-wise mode + mmskin_colsum."""
    g = torch.Generator().manual_seed(600 + C)
    x, b, dy = (torch.randn(rows, C, generator=g) for _ in range(3))
    gamma = torch.randn(C, generator=g) * 0.5
    y, yr, (dx, db, dg), (dxr, dbr, dgr) = _run(ops.scale_add, lambda x, b, gamma: x + gamma * b, [x, b, gamma], dy)
    _check("scale_add", [rows, C], dict(y=(y, yr, EW_TOL), dx=(dx, dxr, EW_TOL), db=(db, dbr, EW_TOL), dgamma=(dg, dgr, RED_TOL)))


@pytest.mark.parametrize("n", EW_SIZES)
def test_star_relu(n):
    """s relu(z)^2 + b; (ds, db) is a two-stage sum over at most 1024 blocks, so N_BIG runs the capped grid."""
    g = torch.Generator().manual_seed(700 + n)
    z, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    s, b = torch.tensor([0.8931]), torch.tensor([-0.17])
    y, yr, (dz, ds, db), (dzr, dsr, dbr) = _run(ops.star_relu, lambda z, s, b: s * torch.relu(z) ** 2 + b, [z, s, b], dy)
    _check("star_relu", [n], dict(y=(y, yr, EW_TOL), dz=(dz, dzr, EW_TOL), dsb=(torch.cat([ds, db]), torch.cat([dsr, dbr]), RED_TOL)))


@pytest.mark.parametrize("M,Na,Nb", [(1, 1, 1), (6, 10, 7), (4099, 200, 57)])
def test_concat2_bit_exact(M, Na, Nb):
    g = torch.Generator().manual_seed(800 + M)
    a, b, dy = torch.randn(M, Na, generator=g), torch.randn(M, Nb, generator=g), torch.randn(M, Na + Nb, generator=g)
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    y = ops.concat2(ad, bd)
    y.backward(dy.to(DEV))
    _report("concat2", [M, Na, Nb], dict(y=rel_err(y, torch.cat([a, b], 1)), da=rel_err(ad.grad, dy[:, :Na]), db=rel_err(bd.grad, dy[:, Na:])))
    assert torch.equal(y.detach().cpu(), torch.cat([a, b], 1))
    assert torch.equal(ad.grad.cpu(), dy[:, :Na]) and torch.equal(bd.grad.cpu(), dy[:, Na:])


# ------------------------------------------------------------------------------- 2. dropout
def _drop_mask(n, p, seed, offset):
    """the keep mask of DropoutFn(seed, offset) over n elements, read off an all-ones input"""
    y = ops.DropoutFn.apply(torch.ones(n, device=DEV), p, seed, offset)
    torch.cuda.synchronize()
    return (y != 0).cpu()


def generator_mask(n, p, seed, offset):
    """The counter-based generator the library documents (csrc/common.h): element i keeps iff (h >> 40) / 2^24 >= p with
    h = mix64(mix64(seed) ^ (offset + i)), mix64 the splitmix64 finaliser -- evaluated on the host in wrapping 64-bit arithmetic."""
    def mix64(x):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))
    with np.errstate(over="ignore"):
        ctr = np.full(n, offset, dtype=np.uint64) + np.arange(n, dtype=np.uint64)
        h = mix64(mix64(np.full(1, seed, dtype=np.uint64)) ^ ctr)
    u = (h >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return torch.from_numpy(u >= np.float32(p))


def test_dropout_determinism_and_counter_continuity():
    n, p, seed, off = 5000, 0.3, 1234, 77
    m = _drop_mask(n, p, seed, off)
    assert torch.equal(m, _drop_mask(n, p, seed, off))                 # same (seed, offset): same mask
    assert not torch.equal(m, _drop_mask(n, p, seed + 1, off))         # another seed: another mask
    assert torch.equal(_drop_mask(n - 1, p, seed, off + 1), m[1:])     # element i of a call is counter offset + i
    _report("dropout_continuity", [n, p], dict(keep=float(m.float().mean())))


@pytest.mark.parametrize("n,seed,offset", [(5000, 1234, 77), (N_BIG, 99, (1 << 33) + 5)])
def test_dropout_mask_is_the_documented_generator(n, seed, offset):
    """Bit for bit the mask of the documented generator, also on a second loop trip and with a counter above 2^32."""
    m = _drop_mask(n, 0.3, seed, offset)
    want = generator_mask(n, 0.3, seed, offset)
    _report("dropout_generator", [n, seed, offset], dict(mismatches=int((m != want).sum())))
    assert torch.equal(m, want)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_keep_rate(p):
    """|keep - (1 - p)| < 5 sigma, sigma = sqrt(p (1 - p) / n), at N_BIG for a fixed seed: a condition, not a measurement."""
    n = N_BIG
    keep = float(_drop_mask(n, p, 2024, 0).double().mean())
    sigma = (p * (1 - p) / n) ** 0.5
    _report("dropout_keep_rate", [n, p], dict(keep=keep, deviation_in_sigma=abs(keep - (1 - p)) / sigma))
    assert abs(keep - (1 - p)) < 5 * sigma, (keep, sigma)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n", [257, N_BIG])
def test_dropout_forward_backward_exact(n, p):
    """y = x mask / (1 - p) and dx = dy mask / (1 - p), exactly: one fp32 product with the fp32 quotient 1 / (1 - p)."""
    g = torch.Generator().manual_seed(900 + n)
    x, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    seed, off = 31337, 1000
    mask = _drop_mask(n, p, seed, off)
    scale = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32))
    xd = x.to(DEV).requires_grad_(True)
    y = ops.DropoutFn.apply(xd, p, seed, off)
    y.backward(dy.to(DEV))
    zero = torch.zeros(())
    want_y, want_dx = torch.where(mask, x * scale, zero), torch.where(mask, dy * scale, zero)
    _report("dropout_exact", [n, p], dict(y=rel_err(y, want_y), dx=rel_err(xd.grad, want_dx)))
    assert torch.equal(y.detach().cpu(), want_y) and torch.equal(xd.grad.cpu(), want_dx)


def test_dropout_edge_probabilities():
    g = torch.Generator().manual_seed(950)
    x, dy = torch.randn(1000, generator=g), torch.randn(1000, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    y = ops.DropoutFn.apply(xd, 1.0, 5, 0)                # p = 1: everything dropped, and no 1 / 0 anywhere
    y.backward(dy.to(DEV))
    assert bool((y == 0).all()) and bool((xd.grad == 0).all())
    assert ops.dropout(xd, 0.0, True) is xd                # p = 0: the input itself
    _report("dropout_edges", [1000], dict(y_absmax=float(y.detach().abs().max()), dx_absmax=float(xd.grad.abs().max())))


# ------------------------------------------------------------------------------- 3. reductions and per-plane kernels
@pytest.mark.parametrize("B,L,E,start", [(2, 1, 8, 0), (3, 2, 8, 1), (5, 197, 40, 1), (4, 49, 512, 0), (3, 50, 350, 1)])
def test_token_mean(B, L, E, start):
    g = torch.Generator().manual_seed(1000 + L + E)
    x, dy = torch.randn(B, L, E, generator=g), torch.randn(B, E, generator=g)
    y, yr, (dx,), (dxr,) = _run(lambda x: ops.token_mean(x, start), lambda x: x[:, start:].mean(1), [x], dy)
    _check("token_mean", [B, L, E, start], dict(y=(y, yr, RED_TOL), dx=(dx, dxr, EW_TOL)))
    assert bool((dx[:, :start] == 0).all())


def _mdnet_ref(f, z, t1, t2):
    e = lambda t: t[:, :, None, None]
    return (torch.sigmoid(e(z)) * f + torch.sigmoid(torch.tanh(f * e(t1)) + e(t2))).mean((2, 3))


@pytest.mark.parametrize("feat_grad", [True, False])
@pytest.mark.parametrize("N,C,H,W", [(1, 1, 1, 1), (2, 3, 7, 7), (3, 5, 8, 8), (2, 6, 9, 15)])
def test_mdnet_fuse(N, C, H, W, feat_grad):
    """One wave per plane: HW = 1 / 49 (< 64), 64, 135 (off a multiple of 64); N C = 1 / 6 / 15 leave idle waves in the last block.
    Without a gradient for feat the backward kernel gets dfeat = nullptr."""
    g = torch.Generator().manual_seed(1100 + H * W)
    f = torch.randn(N, C, H, W, generator=g)
    z, t1, t2, dy = (torch.randn(N, C, generator=g) for _ in range(4))
    ref = [t.double().requires_grad_(True) for t in (f, z, t1, t2)]
    yr = _mdnet_ref(*ref)
    yr.backward(dy.double())
    dev = [t.to(DEV).requires_grad_(i > 0 or feat_grad) for i, t in enumerate((f, z, t1, t2))]
    y = ops.mdnet_fuse(*dev)
    y.backward(dy.to(DEV))
    pairs = dict(y=(y.detach().cpu(), yr.detach(), RED_TOL))
    for name, d, r in zip(("dfeat", "dz", "dt1", "dt2"), dev, ref):
        if d.grad is not None:
            pairs[name] = (d.grad.cpu(), r.grad, EW_TOL if name == "dfeat" else RED_TOL)
    assert (dev[0].grad is not None) == feat_grad
    _check("mdnet_fuse", [N, C, H, W, int(feat_grad)], pairs)


def _pool_ref(x, k):
    return F.max_pool2d(x, k).mean((2, 3))


def _windows(x, k):
    N, C, H, W = x.shape
    PH, PW = H // k, W // k
    return x[:, :, :PH * k, :PW * k].reshape(N, C, PH, k, PW, k).permute(0, 1, 2, 4, 3, 5).reshape(N, C, PH, PW, k * k)


@pytest.mark.parametrize("N,C,H,W,k", [(2, 3, 8, 8, 2), (1, 5, 9, 11, 2), (2, 2, 20, 20, 3), (1, 1, 2, 2, 2)])
def test_pool_gap(N, C, H, W, k):
    """MaxPool2d(k) (floor mode: 9 x 11 and 20 x 20 / 3 leave pixels outside every window) + global mean; PH PW = 16 / 20 / 36 / 1.
    The kernel's own dx: dy / (PH PW) at each window's argmax, exactly 0 everywhere else."""
    g = torch.Generator().manual_seed(1200 + H + k)
    x, dy = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, generator=g)
    top2 = _windows(x, k).topk(2, dim=-1).values
    assert bool((top2[..., 0] > top2[..., 1]).all())            # continuous inputs: no ties, the argmax is unique
    y, yr, (dx,), (dxr,) = _run(lambda x: ops.pool_gap(x, k), lambda x: _pool_ref(x, k), [x], dy)
    _check("pool_gap", [N, C, H, W, k], dict(y=(y, yr, RED_TOL), dx=(dx, dxr, EW_TOL)))
    assert torch.equal(dx != 0, dxr != 0)


def test_pool_gap_ties_go_to_the_first_element():
    """A constant plane: every window is a four-way tie, and the first element in row-major order takes the gradient, as in torch."""
    N, C, H, W, k = 2, 3, 9, 11, 2
    PH, PW = H // k, W // k
    g = torch.Generator().manual_seed(1250)
    x, dy = torch.full((N, C, H, W), 1.5), torch.randn(N, C, generator=g)
    y, yr, (dx,), (dxr,) = _run(lambda x: ops.pool_gap(x, k), lambda x: _pool_ref(x, k), [x], dy)
    want = torch.zeros(N, C, H, W, dtype=torch.float64)
    want[:, :, 0:PH * k:k, 0:PW * k:k] = (dy.double() / (PH * PW))[:, :, None, None]
    assert rel_err(dxr, want) < 1e-12 and torch.equal(dxr != 0, want != 0)     # torch itself sends the gradient there
    _check("pool_gap_ties", [N, C, H, W, k], dict(y=(y, yr, RED_TOL), dx=(dx, dxr, EW_TOL)))
    assert torch.equal(dx != 0, want != 0)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("N,Cin,H,W,Cout,k,stride,pad", [(3, 3, 32, 32, 16, 3, 2, 1), (2, 3, 9, 11, 5, 3, 1, 0), (1, 1, 5, 5, 1, 5, 1, 2),
                                                         (2, 2, 7, 7, 3, 1, 2, 0)])
def test_direct_conv2d(N, Cin, H, W, Cout, k, stride, pad, relu, bias):
    g = torch.Generator().manual_seed(1300 + H + Cout + k)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.3 if bias else None
    wr = w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if bias else None
    yr = F.conv2d(x.double(), wr, br, stride=stride, padding=pad)
    if relu:
        yr = F.relu(yr)
    dy = torch.randn(yr.shape, generator=g)
    yr.backward(dy.double())
    wd = w.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True) if bias else None
    y = ops.direct_conv2d(x.to(DEV), wd, bd, stride, pad, relu)
    y.backward(dy.to(DEV))
    pairs = dict(y=(y.detach().cpu(), yr.detach(), RED_TOL), dw=(wd.grad.cpu(), wr.grad, RED_TOL))
    if bias:
        pairs["db"] = (bd.grad.cpu(), br.grad, RED_TOL)
    _check("direct_conv2d", [N, Cin, H, W, Cout, k, stride, pad, int(relu), int(bias)], pairs)


def _embedding_ref(table, ids):
    card = table.shape[1]
    return torch.stack([table[c][ids[:, c].clamp(0, card - 1)] for c in range(table.shape[0])], dim=1)


def _embedding_case(ncols, card, E, B, ids, g):
    table, dy = torch.randn(ncols, card, E, generator=g), torch.randn(B, ncols, E, generator=g)
    tr = table.double().requires_grad_(True)
    ref = _embedding_ref(tr, ids)
    ref.backward(dy.double())
    grads = []
    for _ in range(2):
        td = table.to(DEV).requires_grad_(True)
        out = ops.embedding(td, ids.to(DEV))
        out.backward(dy.to(DEV))
        grads.append(td.grad.cpu())
    return out.detach().cpu(), ref.detach(), grads, tr.grad


@pytest.mark.parametrize("ncols,card,E,B", [(1, 1, 1, 1), (5, 10, 8, 9), (3, 7, 33, 300)])
def test_embedding(ncols, card, E, B):
    """The gather is a copy (bit-exact); the table gradient sums the batch rows that share an id in a fixed order (300 rows over 7 ids),
    so two runs agree bit for bit."""
    g = torch.Generator().manual_seed(1400 + B)
    ids = torch.randint(0, card, (B, ncols), generator=g)
    out, ref, grads, want = _embedding_case(ncols, card, E, B, ids, g)
    _check("embedding", [ncols, card, E, B], dict(out=(out, ref, EW_TOL), dtable=(grads[0], want, RED_TOL)))
    assert torch.equal(out.double(), ref) and torch.equal(grads[0], grads[1])


def test_embedding_out_of_range_ids_are_clamped_in_both_directions():
    """ids below 0 and above card - 1 read the clamped row, so that row must receive their gradient (embedding_bwd_kernel clamps as the
    forward does; it matched the raw id before and dropped them)."""
    ncols, card, E, B = 5, 10, 8, 9
    g = torch.Generator().manual_seed(1450)
    ids = torch.randint(0, card, (B, ncols), generator=g)
    ids[0, 0], ids[1, 0], ids[2, 3], ids[8, 4], ids[4, 2], ids[5, 2] = -1, card + 2, card + 2, -1, -(1 << 40), 1 << 40
    out, ref, grads, want = _embedding_case(ncols, card, E, B, ids, g)
    _check("embedding_clamped", [ncols, card, E, B], dict(out=(out, ref, EW_TOL), dtable=(grads[0], want, RED_TOL)))
    assert torch.equal(out.double(), ref)


# ------------------------------------------------------------------------------- 4. entries with no wrapper of their own
SOFTMAX_SCALE = float(torch.tensor(32 ** -0.5, dtype=torch.float32))     # what the C ABI's float parameter receives


def softmax_reference(x, scale, mask, bias, causal):
    """softmax over keys of x scale + mask[b, key] + bias[h, query, key], keys above the diagonal excluded under causal (fp64)"""
    s = x * scale
    if mask is not None:
        s = s + mask.double()[:, None, None, :]
    if bias is not None:
        s = s + bias.double()[None]
    if causal:
        L = x.shape[-1]
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), float("-inf"))
    return torch.softmax(s, dim=-1)


def softmax_mask(B, L, g):
    """additive key mask [B, L]: the last batch row fully masked with the fp32 minimum, the others with about a third of the keys masked"""
    m = torch.where(torch.rand(B, L, generator=g) < 0.3, F32_MIN, 0.0)
    m[:, 0] = 0.0
    m[B - 1] = F32_MIN
    return m


@pytest.mark.parametrize("variant", ["plain", "mask", "bias", "mask_bias", "causal"])
@pytest.mark.parametrize("B,H,L", [(1, 1, 1), (2, 3, 63), (2, 2, 65), (1, 5, 130)])
def test_softmax_entries(B, H, L, variant):
    """mmskin_softmax_forward / _backward without the GEMMs around them: one wave per row, four rows per block (B H L = 1, 378, 260, 650
    rows leave the r >= rows guard live in three of four shapes), L below, across and twice across the 64 lanes."""
    g = torch.Generator().manual_seed(1500 + L + len(variant))
    x, dy = torch.randn(B, H, L, L, generator=g) * 3, torch.randn(B, H, L, L, generator=g)
    mask = softmax_mask(B, L, g) if "mask" in variant else None
    bias = torch.randn(H, L, L, generator=g) if "bias" in variant else None
    causal = variant == "causal"
    xr = x.double().requires_grad_(True)
    yr = softmax_reference(xr, SOFTMAX_SCALE, mask, bias, causal)
    yr.backward(dy.double())
    assert float((yr.detach().sum(-1) - 1).abs().max()) < 1e-12
    dev = lambda t: None if t is None else t.to(DEV)
    xd, dyd, md, bd = dev(x), dev(dy), dev(mask), dev(bias)
    y, dx = torch.empty_like(xd), torch.empty_like(xd)
    rows = B * H * L
    call("mmskin_softmax_forward", ptr(xd), ptr(md), ptr(bd), ptr(y), rows, L, H * L, SOFTMAX_SCALE, int(causal), stream())
    call("mmskin_softmax_backward", ptr(dyd), ptr(y), ptr(dx), rows, L, SOFTMAX_SCALE, stream())
    torch.cuda.synchronize()
    y, dx = y.cpu(), dx.cpu()
    _check("softmax", [B, H, L, variant], dict(y=(y, yr.detach(), RED_TOL), dx=(dx, xr.grad, RED_TOL)))
    if mask is not None:      # the fully masked batch row: uniform over the keys, as torch gives
        assert float((y[B - 1].double() * L - 1).abs().max()) < 2e-7
    if causal:
        upper = torch.ones(L, L, dtype=torch.bool).triu(1)
        assert bool((y[..., upper] == 0).all()) and bool((dx[..., upper] == 0).all())
        assert float((y.double().sum(-1) - 1).abs().max()) < 1e-6


@pytest.mark.parametrize("M,N", [(4, 64), (5, 32), (9, 2048), (4099, 96)])
def test_layernorm_mixed_outputs(M, N):
    """ops.layernorm(out_dtype=bfloat16, keep_f32=True) -> mmskin_layernorm_forward_mixed: the fp32 output against fp64 F.layer_norm, and
    the bf16 output bit for bit the fp32 one rounded to bf16 -- layernorm_fwd_rows_kernel forms both from the same register.  The bf16-only
    call (no fp32 pointer) gives the same bf16 tensor; a LayerNorm without bias takes the b == nullptr branch."""
    g = torch.Generator().manual_seed(1600 + M + N)
    x = torch.randn(M, N, generator=g) * 3 + 1
    w, b = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    y32, y16 = ops.layernorm(xd, wd, bd, 1e-5, out_dtype=torch.bfloat16, keep_f32=True)
    only16 = ops.layernorm(xd, wd, bd, 1e-5, out_dtype=torch.bfloat16)
    n32, n16 = ops.layernorm(xd, wd, None, 1e-5, out_dtype=torch.bfloat16, keep_f32=True)
    torch.cuda.synchronize()
    assert y32.dtype == torch.float32 and y16.dtype == only16.dtype == n16.dtype == torch.bfloat16
    want = F.layer_norm(x.double(), (N,), w.double(), b.double(), 1e-5)
    want_nb = F.layer_norm(x.double(), (N,), w.double(), None, 1e-5)
    _check("layernorm_mixed", [M, N], dict(y32=(y32.cpu(), want, EW_TOL), y32_no_bias=(n32.cpu(), want_nb, EW_TOL),
                                           y16=(y16.float().cpu(), want, None)))     # bf16: recorded only, the exact check is below
    assert torch.equal(y16, y32.bfloat16()) and torch.equal(only16, y16) and torch.equal(n16, n32.bfloat16())


def test_layernorm_mixed_refuses_widths_off_a_multiple_of_four():
    """N = 85: the entry itself refuses, and ops.layernorm sends the width to the general kernel instead (fp32 result for both outputs)."""
    M, N = 7, 85
    g = torch.Generator().manual_seed(1685)
    x, w, b = torch.randn(M, N, generator=g) * 3 + 1, torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    y32, y16 = torch.empty_like(xd), torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(_lib.MMSkinError):
        call("mmskin_layernorm_forward_mixed", ptr(xd), ptr(wd), ptr(bd), ptr(y32), ptr(y16), M, N, 1e-5, stream())
    ya, yb = ops.layernorm(xd, wd, bd, 1e-5, out_dtype=torch.bfloat16, keep_f32=True)
    want = F.layer_norm(x.double(), (N,), w.double(), b.double(), 1e-5)
    _check("layernorm_mixed_n85", [M, N], dict(y=(ya.cpu(), want, EW_TOL)))
    assert yb is ya and ya.dtype == torch.float32
