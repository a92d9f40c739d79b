"""-m gpu: mmskin.optim.Adam, bottom up.

A. `mmskin_adam_step` (adam_step_kernel, csrc/head.hip) called through the C ABI on flat tensors against torch's documented Adam update
   evaluated in fp64 from the same fp32 inputs: g' = g + wd p, m' = m + (1-b1)(g' - m), v' = b2 v + (1-b2) g'^2,
   den = sqrt(v')/sqrt(bc2) + eps, p' = p - (lr/bc1) m'/den.  The bounds are derived in `_reference`, never fitted.
B. the optimizer's host decisions (which parameters form a run, one step count per run, folding state back after a reload, GradScaler)
   against torch.optim.Adam on clones, tolerances of tests/test_optim.py::test_arena_runs_match_torch_adam."""
import io
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from gpu_util import DEV
from helpers import SMALL, arena, disable_dropout
from mmskin import _lib
from mmskin._lib import call, ptr, stream
from mmskin.optim import Adam

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
TINY = 2.0 ** -126      # smallest normal fp32: what one operation can lose when its result is subnormal and flushed to zero
SLACK = 1 + 2.0 ** -10  # the bounds below are first order in U; the dropped U^2 terms are < 2^-20 of them
BASE = dict(lr=5e-5, b1=0.9, b2=0.999, eps=1e-8, wd=1e-4, step=3)
GUARD = 64              # floats after every array that the kernel must leave alone


def _roundings(c):
    """(cast, mul): the roundings a host scalar costs -- 1 for its cast to float unless that is exact, 1 for the multiplication by it
    unless the float is 0 or a power of two (then the product is exact)."""
    cf = float(np.float32(c))
    return (0 if cf == c else 1), (0 if cf == 0.0 or math.frexp(cf)[0] == 0.5 else 1)


def _reference(p, g, m, v, lr, b1, b2, eps, wd, step):
    """fp64 update from the fp32 inputs, and the elementwise error bounds of adam_step_kernel's fp32 evaluation.

    The kernel rounds every operation once (a contracted multiply-add rounds once where two are counted, which is within the same
    bound); the host casts (float)(lr/bc1), (float)(1-b1), (float)b2, (float)(1-b2), (float)eps, (float)wd, (float)(1/sqrt(bc2)) from
    doubles.  k(c) = roundings of scalar c (see `_roundings`); sqrtf and `/` are counted at 1 ulp = 2U each, which holds for a correctly
    rounded and for a 1-ulp implementation.  Every operation may also lose TINY to a flushed subnormal.  A sum rounds to the nearest
    float, and either operand is a float, so add(a, b) = min(U |a + b|, |a|, |b|) bounds its rounding (0 when an operand is 0).
    First order in U:

      g^ = fl(g + fl(wd_f p)):            Eg  = k(wd) U |wd p| + add(g, wd p)
      d  = fl(g^ - m):                    Ed  = Eg + add(g', m)
      m^ = fl(m + fl(b1c_f d)):           Em  = b1c Ed + k(b1c) U b1c |d| + add(m, b1c d)                      [3 + k(b1c) roundings]
      v^ = fl(fl(b2_f v) + fl(fl(b2c_f g^) g^)):
                                          Ev  = b2c (2 |g'| Eg + U g'^2) + k(b2c) U b2c g'^2 + k(b2) U b2 v + U v'   [<= 6 roundings]
      s  = sqrtf(v^):                     Es  = min(Ev / (sqrt(v' - Ev) + sqrt(v')), sqrt(Ev)) + 2U sqrt(v')
      den^ = fl(fl(s inv_f) + eps_f):     Eden = inv Es + k(inv) U inv sqrt(v') + cast(eps) U eps + U den
      num^ = fl(ss_f m^):                 Enum = ss Em + k(ss) U ss |m'|
      q  = num^ / den^:                   Eq  = Enum / (den - Eden) + |num| Eden / (den (den - Eden)) + 2U |q|
      p^ = fl(p - q):                     Ep  = Eq + U |p'|

    With wd = 0 and the default betas that is |dm| <= 1.6 U max(|g'|, |m|), |dv| <= 4 U v', |dp| <= U |p'| + ~13 U (lr/bc1) max(|g'|, |m|)/den:
    inside the issue's count (4U M, 8U v', 2U |p'| + 16U (lr/bc1) M/den with M = max(|g'|, |m|)).  That count takes g' as given; where
    the decay term is not small next to g' (a zero gradient, or wd p cancelling it) the two roundings of wd p weigh k(wd) U |wd p| / |g'|,
    which no multiple of U covers, and the bound above, which carries that term, is the correct one.  `_check` asserts elementwise that
    wherever 8 |wd p| <= |g'| the derived bound is no wider than the issue's count.  The fp64 reference's own error (~1e-16 relative) is 9 orders below U and is not counted."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    ss, inv, b1c, b2c = lr / bc1, 1.0 / math.sqrt(bc2), 1.0 - b1, 1.0 - b2
    k = lambda c: sum(_roundings(c))
    wp = wd * p
    g1 = g + wp
    d = g1 - m
    m1 = m + b1c * d
    v1 = b2 * v + b2c * g1 * g1
    sq = v1.sqrt()
    den = sq * inv + eps
    num = ss * m1
    q = num / den
    p1 = p - q
    add = lambda a, b: torch.minimum(U * (a + b).abs(), torch.minimum(a.abs(), b.abs()))
    Eg = (k(wd) * U * wp.abs() + add(g, wp) + TINY) if wd != 0 else torch.zeros_like(g)
    Em = b1c * (Eg + add(g1, -m)) + k(b1c) * U * b1c * d.abs() + add(m, b1c * d) + 3 * TINY
    Ev = b2c * (2 * g1.abs() * Eg + U * g1 * g1) + k(b2c) * U * b2c * g1 * g1 + k(b2) * U * b2 * v + U * v1 + 4 * TINY
    Es = torch.minimum(Ev / ((v1 - Ev).clamp_min(0).sqrt() + sq).clamp_min(1e-300), Ev.sqrt()) + 2 * U * sq
    Eden = inv * Es + k(inv) * U * inv * sq + _roundings(eps)[0] * U * eps + U * den + TINY
    Enum = ss * Em + k(ss) * U * num.abs() + TINY
    Eq = Enum / (den - Eden) + num.abs() * Eden / (den * (den - Eden)) + 2 * U * q.abs() + TINY
    Ep = Eq + U * p1.abs()
    M = torch.maximum(g1.abs(), m.abs())
    issue = dict(p=2 * U * p1.abs() + 16 * U * ss * M / den, m=4 * U * M, v=8 * U * v1, valid=8 * wp.abs() <= g1.abs())
    return dict(p=p1, m=m1, v=v1), dict(p=SLACK * Ep, m=SLACK * Em, v=SLACK * Ev), issue


def _inputs(n, seed):
    """p ~ N(0,1); m, v of a run in progress; gradients by position: exact zeros, +-1e-20 (g*g underflows), 1e4 and N(0,1); every 16th
    position (two of the special gradients among them) has zero moments, so its denominator is eps alone."""
    gen = torch.Generator().manual_seed(seed)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    m, v = 0.1 * torch.randn(n, generator=gen), (0.1 * torch.randn(n, generator=gen)) ** 2
    i = (torch.arange(n) + n) % 16          # n = 1 -> the 1e-20 position, n = 3..5 -> N(0,1): every size has something to get wrong
    g[i % 8 == 0] = 0.0
    g[i == 1], g[i == 9] = 1e-20, -1e-20
    g[i % 8 == 2] = 1e4
    zero = (i == 0) | (i == 1) | (i == 3)
    m[zero], v[zero] = 0.0, 0.0
    return p, g, m, v


def _launch(p, g, m, v, n, lr, b1, b2, eps, wd, step):
    """the kernel on device copies with GUARD floats behind each array: (p, m, v) after the launch, on the CPU"""
    dev = [torch.cat([t, torch.full((GUARD,), 7.0)]).to(DEV) for t in (p, g, m, v)]
    call("mmskin_adam_step", ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), n, lr, b1, b2, eps, wd, step, stream())
    torch.cuda.synchronize()
    out = [t.cpu() for t in dev]
    for t, name in zip(out, "pgmv"):
        assert bool((t[n:] == 7.0).all()), f"{name}: written past n={n}"
    assert torch.equal(out[1][:n], g), "the gradient is read only"
    return dict(p=out[0][:n], m=out[2][:n], v=out[3][:n])


def _check(case, p, g, m, v, hp):
    n = p.numel()
    want, bound, issue = _reference(p, g, m, v, **hp)
    got = _launch(p, g, m, v, n, **hp)
    fig = {}
    for key in "pmv":
        err = (got[key].double() - want[key]).abs()
        fig[key] = float((err / bound[key]).max())
        # the derived bound against the issue's count where that count holds (8 TINY: the flushed-subnormal terms, which it leaves out)
        fig[key + "_vs_issue"] = float((bound[key] / (issue[key] + 8 * TINY))[issue["valid"]].max()) if bool(issue["valid"].any()) else 0.0
    print(dict(test="adam_step", case=case, err_over_bound=fig))
    for key in "pmv":
        assert bool(torch.isfinite(got[key]).all()), (case, key, "not finite")
        assert fig[key + "_vs_issue"] <= SLACK * (1 + 1e-6), (case, key, "derived bound wider than the issue's", fig)
        assert fig[key] <= 1.0, (case, key, fig)
    return got


# ------------------------------------------------------------------------------- A. the kernel
# 4 194 304 = 4096 blocks x 256 threads x 4 floats: + 4 + 3 is a second trip of the grid-stride loop, a vector remainder and the scalar tail
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1027, 65537, 4194304 + 4 + 3])
def test_kernel_sizes(n):
    p, g, m, v = _inputs(n, 10 + n % 1000)
    got = _check(["n", n], p, g, m, v, dict(BASE, wd=0.0))
    still = (g == 0) & (m == 0) & (v == 0)
    assert torch.equal(got["p"][still], p[still]) and bool((got["m"][still] == 0).all() and (got["v"][still] == 0).all())
    _check(["n", n, "wd"], p, g, m, v, BASE)


CORNERS = ([dict(step=s) for s in (1, 2, 1000, 100000)] + [dict(b1=0.0, b2=0.5), dict(eps=1e-3), dict(wd=0.0), dict(wd=0.1), dict(lr=1e-2),
           dict(b1=0.0, b2=0.5, step=1, wd=0.0), dict(lr=1e-2, eps=1e-3, wd=0.1, step=1000)])


@pytest.mark.parametrize("corner", CORNERS, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_kernel_hyperparameter_corners(corner):
    p, g, m, v = _inputs(1027, 77)
    hp = dict(BASE, **corner)
    got = _check(["corner", corner], p, g, m, v, hp)
    if hp["wd"] == 0.0:
        still = (g == 0) & (m == 0) & (v == 0)
        assert bool(still.any()) and torch.equal(got["p"][still], p[still])


@pytest.mark.parametrize("first", [True, False])
def test_kernel_gradient_cancels_moment(first):
    """g = m_old up to a few ulps: g - m is a difference of nearly equal numbers (exact in fp32; the bound on m' is then U |m'| alone).
    first: zero second moment as well, so sqrt(v') comes from this gradient only."""
    gen = torch.Generator().manual_seed(5)
    n = 1027
    p, m = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    g = m * (1 + 2.0 ** -21 * torch.randint(-4, 5, (n,), generator=gen))
    v = torch.zeros(n) if first else m * m
    _check(["g~m", first], p, g, m, v, dict(BASE, wd=0.0, step=1 if first else 50))


def test_kernel_drift_200_steps():
    """200 successive launches on n = 4099 with fresh N(0,1) gradients against an fp64 run that keeps its own fp64 state, and torch's own
    fp32 torch.optim.Adam (single tensor, not fused) on the same gradients against the same fp64 run.  Both are fp32 elementwise with a
    different association; a factor two separates a rounding difference from a wrong formula: distance(kernel) <= 2 distance(torch) for
    the parameters and both moments (distance = largest absolute difference to fp64)."""
    n, steps = 4099, 200
    hp = dict(BASE)
    gen = torch.Generator().manual_seed(9)
    p0 = torch.randn(n, generator=gen)
    Gpad = torch.randn(steps, n + 1, generator=gen)          # rows 4100 floats apart: every row starts on a 16-byte boundary
    G = Gpad[:, :n]
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, steps + 1):
        g1 = G[t - 1].double() + hp["wd"] * p64
        m64 = m64 + (1 - hp["b1"]) * (g1 - m64)
        v64 = hp["b2"] * v64 + (1 - hp["b2"]) * g1 * g1
        p64 = p64 - hp["lr"] / (1 - hp["b1"] ** t) * m64 / (v64.sqrt() / math.sqrt(1 - hp["b2"] ** t) + hp["eps"])
    Gd = Gpad.to(DEV)
    p, m, v = p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for t in range(1, steps + 1):
        call("mmskin_adam_step", ptr(p), ptr(Gd[t - 1]), ptr(m), ptr(v), n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], hp["wd"], t, stream())
    q = nn.Parameter(p0.clone().to(DEV))
    o = torch.optim.Adam([q], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"], foreach=False, fused=False)
    for t in range(steps):
        q.grad = Gd[t, :n].clone()
        o.step()
    torch.cuda.synchronize()
    dist = lambda a, b: float((a.detach().double().cpu() - b).abs().max())
    ours = dict(p=dist(p, p64), m=dist(m, m64), v=dist(v, v64))
    torchs = dict(p=dist(q, p64), m=dist(o.state[q]["exp_avg"], m64), v=dist(o.state[q]["exp_avg_sq"], v64))
    print(dict(test="adam_step", case="drift200", kernel_to_fp64=ours, torch_fp32_to_fp64=torchs))
    assert all(bool(torch.isfinite(t).all()) for t in (p, m, v))
    for key in "pmv":
        assert ours[key] <= 2 * torchs[key], (key, ours, torchs)


def test_kernel_argument_checks():
    n = 1024
    p, g, m, v = (torch.randn(n + 4, device=DEV) for _ in range(4))
    before = [t.clone() for t in (p, g, m, v)]
    args = lambda ts, n, step: [ptr(t) for t in ts] + [n, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, stream()]
    for bad in range(4):       # each pointer in turn 4 bytes off a 16-byte boundary
        ts = [t[1:] if i == bad else t for i, t in enumerate((p, g, m, v))]
        with pytest.raises(_lib.MMSkinError):
            call("mmskin_adam_step", *args(ts, n, 1))
    with pytest.raises(_lib.MMSkinError):
        call("mmskin_adam_step", *args((p, g, m, v), n, 0))
    call("mmskin_adam_step", *args((p, g, m, v), 0, 1))      # n = 0: nothing to do, nothing touched
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((p, g, m, v), before))


# ------------------------------------------------------------------------------- B. the run logic
ALIGNED = [(300, 300), (256, 300), (70000,)]      # every member clears _MIN_RUN on its own and starts on a 16-byte boundary
ODD = [(257, 257), (256, 300), (70000,)]          # 66 049 elements first: the second and third member start 4 bytes off one


def _clones(ps):
    return [nn.Parameter(p.detach().clone()) for p in ps]


def _grads(arenas, mine, ref, gen, absent=(), scale=1.0):
    """fresh gradients: every arena's as views of ONE flat tensor at the parameters' offsets (what the plan-executed backward hands out),
    None for the members in `absent`; the clones get copies"""
    gone = {id(p) for p in absent}
    for flat, ps in arenas:
        gflat = (torch.randn(flat.numel(), generator=gen) * scale).to(DEV)
        off = 0
        for p in ps:
            p.grad = None if id(p) in gone else gflat[off:off + p.numel()].view(p.shape)
            off += p.numel()
    for a, b in zip(mine, ref):
        if not any(a is p for _, ps in arenas for p in ps):
            a.grad = None if id(a) in gone else (torch.randn(a.shape, generator=gen) * scale).to(DEV)
        b.grad = None if a.grad is None else a.grad.detach().clone()


def _same(o, o_ref, mine, ref, what=""):
    """parameters, both moments and the step count of every parameter against torch's (tolerances of test_arena_runs_match_torch_adam)"""
    for i, (a, b) in enumerate(zip(mine, ref)):
        assert torch.allclose(a, b, rtol=2e-6, atol=1e-7), (what, i, float((a - b).abs().max()))
        sb = o_ref.state.get(b, {})
        sa = o.state.get(a, {})
        assert ("step" in sa) == ("step" in sb), (what, i, "state exists on one side only")
        if "step" in sb:
            for k in ("exp_avg", "exp_avg_sq"):
                assert float((sa[k] - sb[k]).abs().max()) <= 2e-6 * float(sb[k].abs().max()), (what, i, k)
            assert float(sa["step"]) == float(sb["step"]), (what, i, "step", float(sa["step"]), float(sb["step"]))


def _live(o):
    """(entries, flat moment elements) reachable from the optimizer's run table"""
    return len(o._runs), sum(st["m"].numel() + st["v"].numel() for st in o._runs.values())


def _numel(ps):
    return sum(p.numel() for p in ps)


def _setup(shapes, seed=1, free=True, **kw):
    flat, ps = arena(shapes, DEV, seed)
    mine = ps + ([nn.Parameter(torch.randn(17, 5, generator=torch.Generator().manual_seed(seed)).to(DEV))] if free else [])
    ref = _clones(mine)
    kw = dict(dict(lr=3e-3, weight_decay=1e-4), **kw)
    return (flat, ps), mine, ref, Adam(mine, **kw), torch.optim.Adam(ref, **kw), torch.Generator().manual_seed(seed + 100)


@pytest.mark.parametrize("fused", [None, True])
@pytest.mark.parametrize("shapes", [ALIGNED, ODD], ids=["aligned", "odd"])
def test_late_joiner_keeps_its_own_bias_correction(shapes, fused):
    """B has no gradient on steps 1-3 and one on steps 4-6: its first update is 1.0 lr sign(g) with step = 1 (a shared count gives
    0.58 lr and step = 4).  A | B | C never merge -- their counts stay 3 apart -- so three runs; with the odd first member B and C start
    4 bytes off a 16-byte boundary and torch steps them."""
    ar, mine, ref, o, o_ref, gen = _setup(shapes, fused=fused)
    A, B, C = ar[1]
    for it in range(1, 7):
        _grads([ar], mine, ref, gen, absent=[B] if it <= 3 else [])
        o.step(); o_ref.step()
        _same(o, o_ref, mine, ref, f"step {it}")
    assert [float(o.state[q]["step"]) for q in (A, B, C)] == [6.0, 3.0, 6.0]
    want = [A, B, C] if shapes is ALIGNED else [A]
    assert _live(o) == (len(want), 2 * _numel(want))


@pytest.mark.parametrize("fused", [None, True])
@pytest.mark.parametrize("shapes", [ALIGNED, ODD], ids=["aligned", "odd"])
def test_skipper_leaves_and_returns(shapes, fused):
    """B has a gradient on steps 1-2, none on step 3, one on steps 4-5: the run A B C of steps 1-2 ends at step 3 (A and C go on alone, B
    keeps count 2), and nothing of it stays behind in the run table."""
    ar, mine, ref, o, o_ref, gen = _setup(shapes, fused=fused)
    A, B, C = ar[1]
    for it in range(1, 6):
        _grads([ar], mine, ref, gen, absent=[B] if it == 3 else [])
        o.step(); o_ref.step()
        _same(o, o_ref, mine, ref, f"step {it}")
        if it == 2:
            assert _live(o) == (1, 2 * _numel([A, B, C]))
        if it == 3:
            want = [A, C] if shapes is ALIGNED else [A]
            assert _live(o) == (len(want), 2 * _numel(want))
    assert [float(o.state[q]["step"]) for q in (A, B, C)] == [5.0, 4.0, 5.0]
    want = [A, B, C] if shapes is ALIGNED else [A]
    assert _live(o) == (len(want), 2 * _numel(want))


def test_steady_state_is_one_launch_and_no_device_read():
    """All members present on every step: one run over the whole arena, and a steady-state step() reads nothing back from the device
    (torch's sync debug mode raises on a synchronizing call; whether the mode is effective on this build is printed)."""
    ar, mine, ref, o, o_ref, gen = _setup(ALIGNED, free=False, fused=True)
    for it in range(3):
        _grads([ar], mine, ref, gen)
        o.step(); o_ref.step()
    assert _live(o) == (1, 2 * ar[0].numel())
    (st,) = o._runs.values()
    assert st["n"] == ar[0].numel() and st["params"][0] is ar[1][0]
    _grads([ar], mine, ref, gen)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            float(ar[0][0])
            effective = False
        except RuntimeError:
            effective = True
        o.step()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    print(dict(test="adam_steady_state", sync_debug_mode_effective=effective))
    o_ref.step()
    _same(o, o_ref, mine, ref, "step 4")
    assert _live(o) == (1, 2 * ar[0].numel())


def test_grad_scaler_unscales_and_skips():
    """fused=True makes torch.amp.GradScaler.step() hand grad_scale / found_inf to step() instead of unscaling: two plain steps (the run
    forms), two scaled steps that match torch, an inf that must leave everything bit for bit as it was, then a plain step from the flat
    moments torch updated through their views."""
    ar, mine, ref, o, o_ref, gen = _setup(ALIGNED, fused=True)
    scalers = [torch.amp.GradScaler("cuda", init_scale=1024.0) for _ in range(2)]
    for it in range(2):
        _grads([ar], mine, ref, gen)
        o.step(); o_ref.step()
    assert _live(o) == (1, 2 * ar[0].numel())

    def scaled_step():
        for s, opt in zip(scalers, (o, o_ref)):
            s.scale(torch.zeros((), device=DEV))      # what scaling the loss does to the scaler: it creates its scale tensor
            s.step(opt)
            s.update()

    for it in range(2):
        _grads([ar], mine, ref, gen, scale=1024.0)
        scaled_step()
        _same(o, o_ref, mine, ref, f"scaled step {it}")
    snap = lambda opt, ps: [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), float(opt.state[p]["step"]))
                            for p in ps]
    before = snap(o, mine), snap(o_ref, ref)
    _grads([ar], mine, ref, gen, scale=1024.0)
    mine[1].grad.view(-1)[12345] = float("inf")
    ref[1].grad.view(-1)[12345] = float("inf")
    scaled_step()
    for was, now in zip(before, (snap(o, mine), snap(o_ref, ref))):
        for (p0, m0, v0, t0), (p1, m1, v1, t1) in zip(was, now):
            assert torch.equal(p0, p1) and torch.equal(m0, m1) and torch.equal(v0, v1) and t0 == t1 == 4.0
            assert bool(torch.isfinite(m1).all() and torch.isfinite(v1).all())
    assert _live(o) == (1, 2 * ar[0].numel())
    (st,) = o._runs.values()
    assert all(o.state[q]["exp_avg"].untyped_storage().data_ptr() == st["m"].untyped_storage().data_ptr() for q in ar[1])
    _grads([ar], mine, ref, gen)
    o.step(); o_ref.step()
    _same(o, o_ref, mine, ref, "plain step after the scaler")
    assert _live(o) == (1, 2 * ar[0].numel())


def _round_trip(sd):
    """through torch.save / torch.load, as a checkpoint travels (tensors that share storage still share it afterwards)"""
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    return torch.load(f, map_location=DEV)


@pytest.mark.parametrize("fused", [None, True])
@pytest.mark.parametrize("how", ["self", "torch_to_arena", "arena_to_torch"])
def test_reload_then_two_more_steps(how, fused):
    ar, mine, ref, o, o_ref, gen = _setup(ALIGNED, fused=fused)
    for it in range(3):
        _grads([ar], mine, ref, gen)
        o.step(); o_ref.step()
    _same(o, o_ref, mine, ref, "before the reload")
    if how == "self":
        o.load_state_dict(_round_trip(o.state_dict()))
    elif how == "torch_to_arena":
        o.load_state_dict(_round_trip(o_ref.state_dict()))
    else:
        sd = _round_trip(o.state_dict())
        o_ref = torch.optim.Adam(ref, lr=3e-3, weight_decay=1e-4, fused=fused)
        o_ref.load_state_dict(sd)
    for it in range(2):
        _grads([ar], mine, ref, gen)
        o.step(); o_ref.step()
        _same(o, o_ref, mine, ref, f"{how}: step {it} after the reload")
    assert float(o_ref.state[ref[0]]["step"]) == 5.0
    assert _live(o) == (1, 2 * ar[0].numel())


def test_two_param_groups_share_one_arena():
    """The halves of one arena in groups with different hyper-parameters: a run per half; a second arena in an amsgrad group takes torch's path."""
    flat, ps = arena([(300, 300), (70000,), (256, 300), (70000,)], DEV, 4)
    flat2, qs = arena([(300, 300), (4,)], DEV, 5)
    mine = ps + qs
    ref = _clones(mine)
    groups = lambda xs: [dict(params=xs[:2], lr=1e-3, weight_decay=0.0, betas=(0.8, 0.99)), dict(params=xs[2:4], lr=1e-4, weight_decay=1e-2),
                         dict(params=xs[4:], amsgrad=True)]
    o, o_ref = Adam(groups(mine)), torch.optim.Adam(groups(ref))
    gen = torch.Generator().manual_seed(6)
    for it in range(3):
        _grads([(flat, ps), (flat2, qs)], mine, ref, gen)
        o.step(); o_ref.step()
        _same(o, o_ref, mine, ref, f"step {it}")
    assert _live(o) == (2, 2 * flat.numel())
    for a, b in zip(qs, ref[4:]):
        assert torch.allclose(o.state[a]["max_exp_avg_sq"], o_ref.state[b]["max_exp_avg_sq"], rtol=2e-6, atol=0)


def test_misaligned_start_goes_to_torch():
    """A 3-element first member without a gradient: the rest would start at a 12-byte offset, which the kernel's 16-byte accesses refuse."""
    flat, ps = arena([(3,), (300, 300), (256, 300)], DEV, 7)
    ref = _clones(ps)
    o, o_ref = Adam(ps, lr=3e-3, weight_decay=1e-4), torch.optim.Adam(ref, lr=3e-3, weight_decay=1e-4)
    gen = torch.Generator().manual_seed(8)
    for it in range(3):
        _grads([(flat, ps)], ps, ref, gen, absent=[ps[0]])
        o.step(); o_ref.step()
        _same(o, o_ref, ps, ref, f"step {it}")
    assert _live(o) == (0, 0)


def test_step_with_closure():
    """step(closure) returns the closure's loss and applies the gradients the closure leaves, not the ones from before the call."""
    ar, mine, ref, o, o_ref, gen = _setup(ALIGNED)

    def closure():
        _grads([ar], mine, ref, gen)      # both sides' gradients
        return torch.tensor(1.25)

    for it in range(2):
        _grads([ar], mine, ref, torch.Generator().manual_seed(it))     # stale gradients, to be replaced
        la = o.step(closure)
        lb = o_ref.step(lambda: torch.tensor(1.25))
        assert float(la) == float(lb) == 1.25
        _same(o, o_ref, mine, ref, f"step {it}")
    assert _live(o) == (1, 2 * ar[0].numel())


def test_real_backbone_steps_through_one_run(monkeypatch):
    """ResNet-18 + concatenation, fp32 backbone.  mmskin/backbone.py keeps ALL of an encoder's parameters -- convolutions and the
    BatchNorm weights and biases alike -- in one arena (_flat_p; only the running statistics live in a second one, and they are buffers),
    and its backward hands out views of one flat gradient: exactly one run, as long as the image encoder's trainable parameters."""
    monkeypatch.setenv("MMSKIN_BACKBONE_DTYPE", "fp32")
    from models import multimodalIntraInterModal as M
    from oracle.detinit import det_init_, det_inputs
    model = det_init_(M.MultimodalModel(**dict(SMALL, cnn_model_name="resnet-18", attention_mecanism="concatenation", device=DEV))).to(DEV).train()
    disable_dropout(model)
    img, meta, lab = det_inputs(2, 64, 20, 6)
    img, meta, lab = img.to(DEV), meta.to(DEV), lab.to(DEV)
    mine = list(model.parameters())
    ref = _clones(mine)
    o = Adam(mine, lr=5e-5, weight_decay=1e-4, fused=True)
    o_ref = torch.optim.Adam(ref, lr=5e-5, weight_decay=1e-4)

    def backward():
        o.zero_grad()
        nn.functional.cross_entropy(model(img, meta), lab).backward()

    backward()
    for a, b in zip(mine, ref):
        b.grad = None if a.grad is None else a.grad.detach().clone()
    o.step(); o_ref.step()
    enc = sum(p.numel() for p in model.image_encoder.parameters() if p.requires_grad)
    assert enc > 10_000_000 and _live(o) == (1, 2 * enc)
    (st,) = o._runs.values()
    assert st["n"] == enc
    _same(o, o_ref, mine, ref, "first step")
    for it in range(2):
        backward()
        o.step()
        assert _live(o) == (1, 2 * enc)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in mine)
    assert float(st["step"]) == 3.0
