"""Cases and CPU references for the op-level DenseNet / VGG tests (tests/test_gpu_densenet_ops.py, tests/test_gpu_vgg_ops.py), checked on
the CPU by tests/test_cpu_densenet_cases.py.  Every row names the edge it exists for; the shapes are the smallest at which that edge exists,
not the workload's.

References are plain torch in fp64.  Inputs, weights and upstream gradients are bf16-representable (rb), so operands are exact in both
element types.  dense_block_deferred / transition_chain restate the plan's chain (csrc/densenet.hip) with a rounding hook `rnd`:
  rnd = identity : the algebraic rewrite alone ("every consumer adds cA*g + cB*x + cC" summed as coefficients and applied once); the CPU
                   test proves it equal to autograd through torch.cat;
  rnd = rb64     : the bf16 EMULATION -- fp64 arithmetic, rounded to bf16 exactly where the plan stores a T: t, a, u, the 32-channel slice of
                   cat, sB, sU, sA, sZ and each read-modify-write of dcat.  Statistics and BatchNorm-backward sums are taken on the values AS
                   STORED, in the conv epilogues too: conv_gemm.hip stages the accumulators in LDS in the element type, and its epilogue
                   sums what it read back from there (the masked gradient is rounded before it is summed, "like the stand-alone reduce
                   kernel")."""
from collections import namedtuple

import torch
import torch.nn.functional as F

from mbconv_cases import EPC, rb

GROWTH, BOTTLE, EPS, MOM = 32, 128, 1e-5, 0.1
DENSE_DEPTHS = (6, 12, 32, 32)
BN_SINGLE_STAGE_ROWS = 512            # bn.hip: more partial rows than this take the finalize entries' two-stage path


def pad64(c):
    return (c + 63) // 64 * 64


def rb64(t):
    """fp64 value rounded to bf16 (through fp32: both roundings are to nearest even and fp32 keeps 16 more bits than bf16 -- a double
    rounding differs only on ties of measure zero for the emulation's purpose)"""
    return t.float().bfloat16().double()


# ------------------------------------------------------------------ tables
BlockCase = namedtuple("BlockCase", "N C0 L H W edge")
BLOCK_CASES = [
    BlockCase(2, 64, 3, 7, 5, "Cin 64/96/128: one layer has padded channels (Cp = 128 > Cin = 96); rows = 70, a multiple of no tile"),
    BlockCase(3, 128, 2, 1, 1, "rows = 3: three samples per channel"),
    BlockCase(2, 64, 6, 14, 14, "block 1's real depth: six consumers of the block input"),
    BlockCase(1, 256, 2, 3, 3, "block-4-like width: Cin = 288 padded to 320"),
]
TransCase = namedtuple("TransCase", "C N H W pitch edge")
TRANS_CASES = [
    TransCase(128, 2, 7, 7, 64 + 32 * 2, "odd map, pooled to 3x3"),
    TransCase(128, 1, 5, 8, 64 + 32 * 2, "one dimension odd"),
    TransCase(256, 2, 4, 4, 128, "pitch equal to C/2"),
]
SliceCase = namedtuple("SliceCase", "rows C pitch c0 dtype edge")
SLICE_CASES = [
    SliceCase(70, 64, 160, 32, "fp32", "small: at most two partial rows, the last row block short, slice in the middle of a row"),
    SliceCase(70, 64, 160, 32, "bf16", "small: at most two partial rows, the last row block short, slice in the middle of a row"),
    SliceCase(65536 + 70, 32, 64, 32, "fp32", "two-stage finalize: more than 512 partial rows, last row block short"),
    SliceCase(131072 + 70, 32, 64, 32, "bf16", "two-stage finalize: more than 512 partial rows, last row block short"),
    SliceCase(128 * 100 + 5, 32, 64, 0, "fp32", "64 < partial rows <= 512: single launch, all 16 row lanes busy"),
]
MAXPOOL_CASES = [(2, 64, 6, 6), (1, 64, 7, 5), (2, 64, 2, 2)]                                   # N, C, H, W
ADAPTIVE_CASES = [(2, 64, 2, 2), (2, 64, 3, 3), (2, 64, 7, 7), (2, 64, 10, 10), (1, 64, 9, 12), (2, 64, 14, 14), (2, 24, 10, 10),
                  (1, 6, 10, 9)]            # C = 24: a multiple of 8 only; C = 6: of neither chunk width (4 fp32, 8 bf16)


def block_id(c):
    return f"n{c.N}-c{c.C0}-l{c.L}-{c.H}x{c.W}"


def trans_id(c):
    return f"c{c.C}-n{c.N}-{c.H}x{c.W}-p{c.pitch}"


def slice_id(c):
    return f"r{c.rows}-c{c.C}-p{c.pitch}-o{c.c0}-{c.dtype}"


def col_geom(rows, C, epc):
    """col_geom of ops_internal.h -> (RL row lanes, RB rows per block, gx row blocks = partial rows)"""
    cpr = C // epc
    cw = 256 if cpr >= 256 else cpr
    rl = 256 // cw
    rbk = max((rows + 1023) // 1024, rl * 4)
    rbk = (rbk + rl - 1) // rl * rl
    return rl, rbk, (rows + rbk - 1) // rbk


def block_classes(C0, L):
    return {("padded" if (C0 + GROWTH * i) % 64 else "unpadded") for i in range(L)}


def densenet_geometry(size):
    """(blocks, transitions) of DensePlan at a size x size input: blocks (C0, L, H, W), transitions (C, H, W)"""
    h = (size + 6 - 7) // 2 + 1
    h = (h + 2 - 3) // 2 + 1
    c, blocks, trans = 64, [], []
    for bi, depth in enumerate(DENSE_DEPTHS):
        blocks.append((c, depth, h, h))
        c += GROWTH * depth
        if bi < 3:
            trans.append((c, h, h))
            c //= 2
            h //= 2
    return blocks, trans


# ------------------------------------------------------------------ dense block
def block_param_slices(C0, L):
    """per layer: name -> (offset, shape) into the flat parameter vector (torchvision order), and the total"""
    out, off = [], 0
    for i in range(L):
        cin, d = C0 + GROWTH * i, {}
        for name, shape in (("g1", (cin,)), ("b1", (cin,)), ("w1", (BOTTLE, cin, 1, 1)), ("g2", (BOTTLE,)), ("b2", (BOTTLE,)), ("w2", (GROWTH, BOTTLE, 3, 3))):
            n = 1
            for s in shape:
                n *= s
            d[name] = (off, shape)
            off += n
        out.append(d)
    return out, off


def block_buffer_slices(C0, L):
    out, off = [], 0
    for i in range(L):
        cin, d = C0 + GROWTH * i, {}
        for name, n in (("rm1", cin), ("rv1", cin), ("rm2", BOTTLE), ("rv2", BOTTLE)):
            d[name] = (off, (n,))
            off += n
        out.append(d)
    return out, off


def unflatten(flat, slices):
    return [{k: flat[o:o + int(torch.tensor(s).prod())].reshape(s) for k, (o, s) in d.items()} for d in slices]


def flatten(layers, slices, total, dtype=torch.float64):
    flat = torch.zeros(total, dtype=dtype)
    for d, sl in zip(layers, slices):
        for k, (o, s) in sl.items():
            flat[o:o + d[k].numel()] = d[k].reshape(-1).to(dtype)
    return flat


def block_inputs(c):
    """bf16-representable x, dcat and flat parameters (fp32, CPU).  gamma around 1, beta around 0.2 so about half of every ReLU is open."""
    g = torch.Generator().manual_seed(1000 * c.C0 + 100 * c.L + 10 * c.H + c.W)
    ctot = c.C0 + GROWTH * c.L
    x = rb(torch.randn(c.N, c.C0, c.H, c.W, generator=g))
    dcat = rb(torch.randn(c.N, ctot, c.H, c.W, generator=g))
    slices, total = block_param_slices(c.C0, c.L)
    layers = []
    for i in range(c.L):
        cin = c.C0 + GROWTH * i
        layers.append(dict(g1=rb(1 + 0.3 * torch.randn(cin, generator=g)), b1=rb(0.2 + 0.2 * torch.randn(cin, generator=g)),
                           w1=rb(torch.randn(BOTTLE, cin, 1, 1, generator=g) * cin ** -0.5),
                           g2=rb(1 + 0.3 * torch.randn(BOTTLE, generator=g)), b2=rb(0.2 + 0.2 * torch.randn(BOTTLE, generator=g)),
                           w2=rb(torch.randn(GROWTH, BOTTLE, 3, 3, generator=g) * (9 * BOTTLE) ** -0.5)))
    return x, dcat, flatten(layers, slices, total, torch.float32)


def _stats(t):
    return t.mean((0, 2, 3)), t.var((0, 2, 3), unbiased=False)


def _v(t):
    return t.reshape(1, -1, 1, 1)


def block_autograd(c, x, dcat, params, training=True, buffers=None):
    """fp64 torch: torchvision's _DenseLayer chain through torch.cat.  training: (cat, table, running buffers after one step, dx, grads);
    eval (buffers given): cat alone"""
    slices, total = block_param_slices(c.C0, c.L)
    bsl, btotal = block_buffer_slices(c.C0, c.L)
    p = params.double().clone().requires_grad_(training)
    layers = unflatten(p, slices)
    xd = x.double().clone().requires_grad_(training)
    bufs = unflatten(buffers.double(), bsl) if buffers is not None else None
    cat = xd
    new_buf = []
    n = c.N * c.H * c.W
    for i, l in enumerate(layers):
        if training:
            m1, v1 = _stats(cat.detach())
            h = F.batch_norm(cat, None, None, l["g1"], l["b1"], True, 0.0, EPS)
        else:
            h = F.batch_norm(cat, bufs[i]["rm1"], bufs[i]["rv1"], l["g1"], l["b1"], False, 0.0, EPS)
        a = F.conv2d(F.relu(h), l["w1"])
        if training:
            m2, v2 = _stats(a.detach())
            h2 = F.batch_norm(a, None, None, l["g2"], l["b2"], True, 0.0, EPS)
            unb = n / (n - 1) if n > 1 else 1.0
            new_buf.append(dict(rm1=MOM * m1, rv1=(1 - MOM) + MOM * v1 * unb, rm2=MOM * m2, rv2=(1 - MOM) + MOM * v2 * unb))
        else:
            h2 = F.batch_norm(a, bufs[i]["rm2"], bufs[i]["rv2"], l["g2"], l["b2"], False, 0.0, EPS)
        cat = torch.cat([cat, F.conv2d(F.relu(h2), l["w2"], padding=1)], 1)
    if not training:
        return cat.detach()
    cat.backward(dcat.double())
    mean, var = _stats(cat.detach())
    return dict(cat=cat.detach(), table=torch.cat([mean, var]), buffers=flatten(new_buf, bsl, btotal), dx=xd.grad, grads=p.grad.detach())


def _conv_bwd(g, inp, w, pad):
    inp, w = inp.detach().requires_grad_(True), w.detach().requires_grad_(True)
    return torch.autograd.grad(F.conv2d(inp, w, padding=pad), (inp, w), g)


def _bn_bwd_coef(dz, x, mean, invstd, gamma):
    """dgamma, dbeta and the coefficients of dx = cA*dz + cB*x + cC (bn_bwd_finalize)"""
    n = dz.numel() / dz.shape[1]
    s1, s2 = dz.sum((0, 2, 3)), (dz * x).sum((0, 2, 3))
    dgamma = (s2 - mean * s1) * invstd
    cA = gamma * invstd
    cB = -gamma * invstd ** 2 * dgamma / n
    cC = -cA * s1 / n - cB * mean
    return dgamma, s1, cA, cB, cC


def block_deferred(c, x, dcat, params, rnd=lambda t: t):
    """the plan's chain (dense_block_forward / dense_block_backward of csrc/densenet.hip) in fp64 with `rnd` at every store of a T"""
    slices, total = block_param_slices(c.C0, c.L)
    layers = unflatten(params.double(), slices)
    ctot = c.C0 + GROWTH * c.L
    cat = torch.zeros(c.N, ctot, c.H, c.W, dtype=torch.float64)
    cat[:, :c.C0] = rnd(x.double())
    mean, var = torch.zeros(ctot, dtype=torch.float64), torch.zeros(ctot, dtype=torch.float64)
    mean[:c.C0], var[:c.C0] = _stats(cat[:, :c.C0])                # slice_stats re-reads the stored input slice
    saved = []
    for i, l in enumerate(layers):
        cin = c.C0 + GROWTH * i
        is1 = 1 / torch.sqrt(var[:cin] + EPS)
        sc1 = l["g1"] * is1
        sh1 = l["b1"] - mean[:cin] * sc1
        t = rnd(F.relu(cat[:, :cin] * _v(sc1) + _v(sh1)))
        a = rnd(F.conv2d(t, l["w1"]))
        m2, v2 = _stats(a)                                          # conv epilogue: statistics of the value as stored
        is2 = 1 / torch.sqrt(v2 + EPS)
        sc2 = l["g2"] * is2
        sh2 = l["b2"] - m2 * sc2
        u = rnd(F.relu(a * _v(sc2) + _v(sh2)))
        o = rnd(F.conv2d(u, l["w2"], padding=1))
        mean[cin:cin + GROWTH], var[cin:cin + GROWTH] = _stats(o)
        cat[:, cin:cin + GROWTH] = o
        saved.append(dict(t=t, a=a, u=u, m1=mean[:cin].clone(), is1=is1, sc1=sc1, sh1=sh1, m2=m2, is2=is2, sc2=sc2, sh2=sh2))
    # backward: one gradient buffer, the x / constant terms of every consumer summed as coefficients
    d = rnd(dcat.double()).clone()
    sB, sC = torch.zeros(ctot, dtype=torch.float64), torch.zeros(ctot, dtype=torch.float64)
    grads = [None] * c.L
    for i in reversed(range(c.L)):
        l, s = layers[i], saved[i]
        cin = c.C0 + GROWTH * i
        sl = slice(cin, cin + GROWTH)
        g = rnd(d[:, sl] + _v(sB[sl]) * cat[:, sl] + _v(sC[sl]))                       # slice_pack_deferred
        du, dw2 = _conv_bwd(g, s["u"], l["w2"], 1)
        dz2 = rnd(du * (s["a"] * _v(s["sc2"]) + _v(s["sh2"]) > 0))                     # sU; the epilogue sums the value as stored
        dg2, db2, cA, cB, cC = _bn_bwd_coef(dz2, s["a"], s["m2"], s["is2"], l["g2"])
        sA = rnd(_v(cA) * dz2 + _v(cB) * s["a"] + _v(cC))                              # bn_bwd_apply -> sA
        dt, dw1 = _conv_bwd(sA, s["t"], l["w1"], 0)
        dz1 = rnd(dt * (cat[:, :cin] * _v(s["sc1"]) + _v(s["sh1"]) > 0))               # sZ; sums of the value as stored
        dg1, db1, cA1, cB1, cC1 = _bn_bwd_coef(dz1, cat[:, :cin], s["m1"], s["is1"], l["g1"])
        sB[:cin] += cB1                                                                # bn_bwd_finalize(accumulate_bc)
        sC[:cin] += cC1
        d[:, :cin] = rnd(d[:, :cin] + _v(cA1) * dz1)                                   # slice_accumulate_scaled
        grads[i] = dict(g1=dg1, b1=db1, w1=dw1, g2=dg2, b2=db2, w2=dw2)
    d[:, :c.C0] = rnd(d[:, :c.C0] + _v(sB[:c.C0]) * cat[:, :c.C0] + _v(sC[:c.C0]))    # slice_affine_inplace
    return dict(cat=cat, table=torch.cat([mean, var]), dx=d[:, :c.C0].clone(), grads=flatten(grads, slices, total))


def block_eval_chain(c, x, params, buffers, rnd=lambda t: t):
    """the plan's eval-mode forward with `rnd` at every store of a T: running statistics, norm2's scale folded into conv1's STAGED weights
    (rounded to the element type), its shift and the ReLU in conv1's epilogue, which reads the accumulators back in the element type"""
    layers = unflatten(params.double(), block_param_slices(c.C0, c.L)[0])
    bufs = unflatten(buffers.double(), block_buffer_slices(c.C0, c.L)[0])
    cat = torch.zeros(c.N, c.C0 + GROWTH * c.L, c.H, c.W, dtype=torch.float64)
    cat[:, :c.C0] = rnd(x.double())
    for i, (l, b) in enumerate(zip(layers, bufs)):
        cin = c.C0 + GROWTH * i
        sc1 = l["g1"] / torch.sqrt(b["rv1"] + EPS)
        t = rnd(F.relu(cat[:, :cin] * _v(sc1) + _v(l["b1"] - b["rm1"] * sc1)))
        sc2 = l["g2"] / torch.sqrt(b["rv2"] + EPS)
        u = rnd(F.relu(rnd(F.conv2d(t, rnd(l["w1"] * sc2.reshape(-1, 1, 1, 1)))) + _v(l["b2"] - b["rm2"] * sc2)))
        cat[:, cin:cin + GROWTH] = rnd(F.conv2d(u, l["w2"], padding=1))
    return cat


_BLOCK_CACHE = {}


def block_reference(c):
    """inputs, fp64 truth and bf16 emulation of one case; computed once and shared (callers must not modify the tensors)"""
    if c not in _BLOCK_CACHE:
        x, dcat, params = block_inputs(c)
        _BLOCK_CACHE[c] = dict(x=x, dcat=dcat, params=params, ref=block_autograd(c, x, dcat, params), emu=block_deferred(c, x, dcat, params, rb64))
    return _BLOCK_CACHE[c]


def eval_buffers(c):
    g = torch.Generator().manual_seed(7 + c.C0 + c.L)
    bsl, btotal = block_buffer_slices(c.C0, c.L)
    flat = torch.zeros(btotal)
    for d in bsl:
        for k, (o, s) in d.items():
            flat[o:o + s[0]] = (0.2 * torch.randn(s[0], generator=g)) if k.startswith("rm") else (0.5 + torch.rand(s[0], generator=g))
    return flat


# ------------------------------------------------------------------ transition
def trans_inputs(c):
    g = torch.Generator().manual_seed(100 * c.C + 10 * c.H + c.W)
    x = rb(torch.randn(c.N, c.C, c.H, c.W, generator=g))
    dnext = rb(torch.randn(c.N, c.pitch, c.H // 2, c.W // 2, generator=g))
    params = torch.cat([rb(1 + 0.3 * torch.randn(c.C, generator=g)), rb(0.2 + 0.2 * torch.randn(c.C, generator=g)),
                        rb(torch.randn(c.C // 2 * c.C, generator=g) * c.C ** -0.5)])
    mean, var = _stats(x.double())
    return x, dnext, params, torch.cat([mean, var]).float()


def trans_chain(c, x, dnext, params, table, rnd=lambda t: t):
    """dense_transition_forward / _backward in fp64 with `rnd` at every store of a T (tt, the conv output, the pooled rows; the pooled
    gradient sC, sZ, dx).  rnd = identity is the fp64 truth: checked against autograd by the CPU test."""
    C, h = c.C, c.C // 2
    p = params.double()
    g, b, w = p[:C], p[C:2 * C], p[2 * C:].reshape(h, C, 1, 1)
    mean, var = table.double()[:C], table.double()[C:]
    xd = x.double()
    invstd = 1 / torch.sqrt(var + EPS)
    sc = g * invstd
    sh = b - mean * sc
    tt = rnd(F.relu(xd * _v(sc) + _v(sh)))
    conv = rnd(F.conv2d(tt, w))
    pooled = rnd(F.avg_pool2d(conv, 2))
    dconv = torch.zeros_like(conv)
    PH, PW = c.H // 2, c.W // 2
    dconv[:, :, :2 * PH, :2 * PW] = rnd(0.25 * dnext.double()[:, :h]).repeat_interleave(2, 2).repeat_interleave(2, 3)   # avgpool2_bwd
    dtt, dw = _conv_bwd(dconv, tt, w, 0)
    dz = rnd(dtt * (xd * _v(sc) + _v(sh) > 0))                                         # sZ; the epilogue sums the value as stored
    dg, db, cA, cB, cC = _bn_bwd_coef(dz, xd, mean, invstd, g)
    dx = rnd(_v(cA) * dz + _v(cB) * xd + _v(cC))
    n = c.N * c.H * c.W
    return dict(conv=conv, pooled=pooled, dz=dz, dx=dx, grads=torch.cat([dg, db, dw.reshape(-1)]),
                buffers=torch.cat([MOM * mean, (1 - MOM) + MOM * var * n / (n - 1)]))


def trans_autograd(c, x, dnext, params):
    C, h = c.C, c.C // 2
    p = params.double().clone().requires_grad_(True)
    xd = x.double().clone().requires_grad_(True)
    y = F.avg_pool2d(F.conv2d(F.relu(F.batch_norm(xd, None, None, p[:C], p[C:2 * C], True, 0.0, EPS)), p[2 * C:].reshape(h, C, 1, 1)), 2)
    y.backward(dnext.double()[:, :h])
    return dict(pooled=y.detach(), dx=xd.grad, grads=p.grad.detach())


_TRANS_CACHE = {}


def trans_reference(c):
    if c not in _TRANS_CACHE:
        x, dnext, params, table = trans_inputs(c)
        _TRANS_CACHE[c] = dict(x=x, dnext=dnext, params=params, table=table, ref=trans_chain(c, x, dnext, params, table),
                               emu=trans_chain(c, x, dnext, params, table, rb64))
    return _TRANS_CACHE[c]


# ------------------------------------------------------------------ VGG pools
TAP_PAIRS = [(a, b) for a in range(4) for b in range(a + 1, 4)]


def maxpool_input(N, C, H, W):
    """post-ReLU map: about 40 % exact zeros, bf16-representable positives, and in window (n = 0, ph = 0, pw = 0) of channel k < 6 the two
    taps TAP_PAIRS[k] hold the SAME positive value, larger than the rest of the window (the all-zero window is channel 6); with more
    than one window the same plants are repeated in the last window.  Returns (y, list of (n, c, ph, pw, first tap))"""
    g = torch.Generator().manual_seed(H * 10 + W)
    y = rb(torch.relu(torch.randn(N, C, H, W, generator=g) + 0.2))
    PH, PW = H // 2, W // 2
    plants = []
    for ph, pw in {(0, 0), (PH - 1, PW - 1)}:
        for k, (a, b) in enumerate(TAP_PAIRS):
            y[0, k, 2 * ph:2 * ph + 2, 2 * pw:2 * pw + 2] = rb(torch.tensor(0.5))
            for tap in (a, b):
                y[0, k, 2 * ph + tap // 2, 2 * pw + tap % 2] = 7.0
            plants.append((0, k, ph, pw, a))
        y[0, 6, 2 * ph:2 * ph + 2, 2 * pw:2 * pw + 2] = 0.0
        plants.append((0, 6, ph, pw, 0))
    return y, plants


def maxpool_reference(y):
    """F.max_pool2d(return_indices=True) on fp64 -> pooled and the tap 0..3 inside each window"""
    N, C, H, W = y.shape
    pooled, flat = F.max_pool2d(y.double(), 2, return_indices=True)
    hh, ww = flat // W, flat % W
    return pooled, ((hh % 2) * 2 + (ww % 2)).to(torch.uint8)


def maxpool_backward_reference(y, tap, dpool):
    """dz = dpool routed to each window's argmax where y > 0, else 0 (exact: no arithmetic)"""
    N, C, H, W = y.shape
    PH, PW = H // 2, W // 2
    dz = torch.zeros(N, C, H, W, dtype=torch.float64)
    for t in range(4):
        sel = (tap == t).double() * dpool.double()
        dz[:, :, t // 2:2 * PH:2, t % 2:2 * PW:2] = sel
    return dz * (y > 0)
