"""Probes that read the fused attention kernels (csrc/flash_attn.hip, csrc/flash_attn_bwd.hip) out element by element, the fp64 model
they are compared with, and the comparison functions -- plain torch, no GPU needed (tests/test_cpu_flash_probe.py proves the harness
on a dense fp64 attention; tests/test_gpu_flash_probe.py points it at the kernels).

The read-out.  probe_v(L, D, blk) is a V whose key D*blk + d holds the unit vector e_d and every other key is zero, so the attention
output is O[i, d] = Pd[i, D*blk + d]: the dropped, rescaled, normalised probability the kernel actually multiplied.  ceil(L / D)
launches return the whole [L, L] matrix (assemble).  probe_do is the same pattern as the output gradient: dV[j, d] = Pd[D*blk + d, j],
the probabilities as the backward recomputed them, under the dropout mask it regenerated (assemble(..., transpose=True)).  Every MFMA sum
has one non-zero term, 1.0 x p, so the read-out adds no error of its own.

The inputs are bf16-representable (`rb` of N(0,1) draws): the kernels' rounding of their operands drops out and what remains is their
own arithmetic -- fp32 scores, one bf16 rounding of a probability, fp32 row statistics."""
import math
from types import SimpleNamespace

import torch

EPS_BF16 = 2.0 ** -9          # the unit the measured ratios are printed in: half a unit in the last place of bf16 at the TOP of a binade
P_REL = 2.0 ** -8             # the per-element bound on a probability read-out.  bf16 has 8 significant bits: round-to-nearest errs by up
#                               to 2^-8 / (1 + 2^-8) just above a power of two (2^-9 just below one), truncation by up to 2^-7
P_FLOOR = 1e-30               # absolute slack: fp32 underflow of a probability next to 0
DROP_FLOOR = 1e-20            # a read-out zero counts as "dropped" only where the undropped probability is above this


def rb(t):
    """round to bf16 and back: a value every kernel operand conversion leaves alone"""
    return t.bfloat16().float()


def n_blocks(L, D):
    return (L + D - 1) // D


def probe_v(L, D, blk):
    """V [L, D]: key D*blk + d = e_d, every other key 0 (bf16-exact)"""
    v = torch.zeros(L, D)
    j = torch.arange(D * blk, min(D * blk + D, L))
    v[j, j - D * blk] = 1.0
    return v


def probe_do(L, D, blk):
    """dO [L, D]: query D*blk + d = e_d, every other query 0"""
    return probe_v(L, D, blk)


def assemble(blocks, L, transpose=False):
    """per-block read-outs [B, H, L, D] (block blk = columns D*blk .. D*blk + D - 1) -> [B, H, L, L] in fp64.  transpose: the blocks
    are dV read-outs, [key, d] = Pd[D*blk + d, key], and the result is put back as [query, key]"""
    full = torch.cat([b.detach() for b in blocks], dim=-1)[..., :L].double().cpu()
    return full.transpose(-1, -2).contiguous() if transpose else full


def forward_kernel(D, has_bias, L):
    """which forward kernel flash_launch (csrc/flash_attn.hip) selects: `Dh == 64 && !bias && L <= 1024` -> flash_fwd2_kernel"""
    return "flash_fwd2_kernel" if D == 64 and not has_bias and L <= 1024 else "flash_fwd_kernel"


# ------------------------------------------------------------------------------------------------------------------- inputs
def inputs(B, H, L, D, seed):
    """q, k, v, dO [B, H, L, D]: bf16-representable N(0,1) draws"""
    g = torch.Generator().manual_seed(seed)
    return [rb(torch.randn(B, H, L, D, generator=g)) for _ in range(4)]


def key_mask(B, L):
    """additive key mask [B, L]: BERT's finite -10000 on the second half of batch entry 0 and a -inf tail of 3 keys on the last entry
    (of min(3, L - 1) keys: a row whose keys are ALL -inf has no softmax -- at L = 1 there is no tail)"""
    m = torch.zeros(B, L)
    m[0, L // 2:] = -10000.0
    tail = min(3, L - 1)
    if tail:
        m[-1, L - tail:] = float("-inf")
    return m


def extras(kind, B, H, L, seed=1):
    """(mask_add, bias, causal) of a kind: 'plain', 'causal', 'mask', 'bias' or any '+' combination"""
    g = torch.Generator().manual_seed(seed)
    bias = torch.randn(H, L, L, generator=g) if "bias" in kind else None
    return (key_mask(B, L) if "mask" in kind else None), bias, "causal" in kind


# ------------------------------------------------------------------------------------------------------------------- fp64 model
def model_fp64(q, k, v, mask_add=None, bias=None, causal=False, dO=None, keep=None, p=0.0):
    """Attention in fp64 with the rounding model of test_gpu_flash_attention._torch_ref_bf16: operands rounded to bf16 (a no-op on
    representable inputs), the scale applied to S afterwards.  -> P, LSE, O and `masked` (the entries causal / -inf take out);
    with dO also dP = dO V^T, delta, dS = P.(dP.keep/(1-p) - delta) and dQ, dK, dV.  keep [B, H, L, L] (bool) with p: dropout on the
    probabilities, Pd = P.keep/(1-p), O = Pd V."""
    D = q.shape[-1]
    scale = 1.0 / math.sqrt(D)
    q, k, v = rb(q).double(), rb(k).double(), rb(v).double()
    L = q.shape[2]
    s = (q @ k.transpose(-1, -2)) * scale
    masked = torch.zeros(s.shape, dtype=torch.bool)
    if bias is not None:
        s = s + bias.double()[None]
    if mask_add is not None:
        s = s + mask_add.double()[:, None, None, :]
        masked = masked | torch.isneginf(mask_add)[:, None, None, :]
    if causal:
        upper = torch.triu(torch.ones(L, L, dtype=torch.bool), 1)
        s = s.masked_fill(upper, float("-inf"))
        masked = masked | upper
    lse = torch.logsumexp(s, -1)
    P = torch.softmax(s, -1)          # not exp(s - lse): next to finfo.min log L is below the rounding of lse, even in fp64
    zs = torch.ones_like(P) if keep is None else keep.double() / (1.0 - p)
    Pd = P * zs
    m = SimpleNamespace(P=P, Pd=Pd, LSE=lse, O=Pd @ v, masked=masked, scale=scale)
    if dO is not None:
        dO = rb(dO).double()
        m.dP = dO @ v.transpose(-1, -2)
        m.delta = (dO * m.O).sum(-1)
        m.dS = P * (m.dP * zs - m.delta[..., None])
        m.dQ = scale * (m.dS @ k)
        m.dK = scale * (m.dS.transpose(-1, -2) @ q)
        m.dV = Pd.transpose(-1, -2) @ dO
    return m


# ------------------------------------------------------------------------------------------------------------------- comparisons
def worst_ratio(got, want, floor=DROP_FLOOR):
    """max |got - want| / want over the entries whose reference is above `floor` (0.0 if there are none)"""
    sel = want > floor
    return float(((got - want).abs()[sel] / want[sel]).max()) if bool(sel.any()) else 0.0


def check_probs(got, want, masked=None, rel=P_REL, floor=P_FLOOR):
    """every element: |got - want| <= rel * want + floor; entries the reference masks out read back as exactly 0.0.
    -> the worst measured |got - want| / want"""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), "non-finite read-out"
    over = (got - want).abs() - (rel * want + floor)
    if bool((over > 0).any()):
        i = int(over.argmax())
        idx, g, w = [], float(got.flatten()[i]), float(want.flatten()[i])
        for n in reversed(got.shape):
            idx.insert(0, i % n)
            i //= n
        raise AssertionError(f"probability at {tuple(idx)}: got {g:.9e}, want {w:.9e}, ratio {abs(g - w) / max(w, 1e-300):.3e} > {rel:.3e}")
    if masked is not None:
        assert bool((got[masked] == 0.0).all()), f"{int((got[masked] != 0).sum())} masked entries are not exactly 0.0"
    return worst_ratio(got, want)


def check_row_sums(got, tol=P_REL):
    """each row of an (undropped) read-out sums to 1 within tol -> the worst |sum - 1|"""
    dev = float((got.double().sum(-1) - 1.0).abs().max())
    assert dev <= tol, f"row sum off by {dev:.3e} > {tol:.3e}"
    return dev


def check_mask(got, keep, undropped, floor=DROP_FLOOR):
    """the zero pattern of a dropped read-out IS the keep mask, on the entries whose undropped reference probability is above `floor`
    (below it an fp32 underflow would be mistaken for a drop) -> the number of entries compared"""
    sel = undropped > floor
    nz, keep = (got != 0)[sel], keep.bool()[sel]
    if not torch.equal(nz, keep):
        raise AssertionError(f"dropout mask differs at {int((nz != keep).sum())} of {int(sel.sum())} entries")
    return int(sel.sum())


def check_keep_share(keep, p, sel=None):
    """the kept share lies within 5 binomial standard deviations of 1 - p (a mask that agrees only because both sides are degenerate
    must not pass) -> the share"""
    kept = keep.bool() if sel is None else keep.bool()[sel]
    n = kept.numel()
    share = float(kept.double().mean())
    sd = math.sqrt(p * (1.0 - p) / n)
    assert abs(share - (1.0 - p)) <= 5.0 * sd, f"kept share {share:.5f} of {n}, expected {1 - p:.5f} +- {5 * sd:.5f}"
    return share


def check_lse(got, want, tol=1e-5):
    """|got - want| <= tol * max(1, |want|) per row -> the worst |got - want| / max(1, |want|)"""
    got, want = got.double(), want.double()
    assert bool(torch.isfinite(got).all()), "non-finite LSE"
    r = float(((got - want).abs() / want.abs().clamp_min(1.0)).max())
    assert r <= tol, f"LSE off by {r:.3e} of max(1, |lse|) > {tol:.1e}"
    return r


def ds_bound(m, p=0.0):
    """per-element bound on dS from flash_bwd_dq_kernel (derived in test_gpu_flash_probe.test_ds_per_element):
    2^-8 / (1 - p) . P_ij . max_j' |dP_ij'| + 1e-6 . max |dS|"""
    return P_REL / (1.0 - p) * m.P * m.dP.abs().amax(-1, keepdim=True) + 1e-6 * float(m.dS.abs().max())


def check_ds(got, m, p=0.0):
    """|got - dS| within ds_bound elementwise, masked entries exactly 0.0 -> the worst |got - dS| / bound"""
    got = got.double()
    assert bool(torch.isfinite(got).all()), "non-finite dS"
    ratio = (got - m.dS).abs() / ds_bound(m, p)
    r = float(ratio.max())
    assert r <= 1.0, f"dS off by {r:.3f} x its bound at element {int(ratio.argmax())}"
    assert bool((got[m.masked] == 0.0).all()), "masked dS entries are not exactly 0.0"
    return r


OPERAND_REL = 2.0 ** -16      # dS and P^T enter the backward's gradient MFMAs as bf16 hi + lo: 16 significant bits


def grad_bounds(m, q, k, dO, p=0.0):
    """per-element bounds on the fused dQ, dK, dV on representable inputs, from what (b), (d) and (e) pin:
    dQ = scale . (hi + lo)(dS) K: the operand split is within 2^-16 |dS_ij| and dS itself is within ds_bound, so
      |d dQ_id| <= scale . sum_j (2^-16 |dS_ij| + (1 + 2^-16) ds_bound_ij) |K_jd|;   dK the same through the transpose with |Q|;
    dV = (hi + lo)(Pd)^T dO: Pd = exp(x - lse) . zs, lse within 1e-5 max(1, |lse|) (|lse| < 10 here: 1e-4 covers it), so
      |d dV_jd| <= (2^-16 + 1e-4) . sum_i Pd_ij |dO_id|.
    Each plus 1e-5 of the largest element for the fp32 accumulation."""
    q, k, dO = rb(q).double(), rb(k).double(), rb(dO).double()
    ds_err = OPERAND_REL * m.dS.abs() + (1.0 + OPERAND_REL) * ds_bound(m, p)
    slop = lambda t: 1e-5 * float(t.abs().max())
    return (m.scale * (ds_err @ k.abs()) + slop(m.dQ), m.scale * (ds_err.transpose(-1, -2) @ q.abs()) + slop(m.dK),
            (OPERAND_REL + 1e-4) * (m.Pd.transpose(-1, -2) @ dO.abs()) + slop(m.dV))


def rms_err(got, want):
    """worst-element error over the rms of the reference"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max()) / (float(want.pow(2).mean().sqrt()) + 1e-30)


# ------------------------------------------------------------------------------------------------------------------- the cases
FWD_LS = (1, 31, 33, 63, 64, 65, 127, 128, 129, 193)
FWD_KINDS = ("plain", "causal", "mask", "bias", "mask+causal+bias")
# (B, H, L, D, kind): the forward probability / LSE cases, and the two that cross the flash_fwd2_kernel -> flash_fwd_kernel switch
FWD_CASES = [(2, 2, L, D, kind) for L in FWD_LS for D in (32, 64) for kind in FWD_KINDS] + \
            [(1, 1, L, 64, kind) for L in (1024, 1025) for kind in ("plain", "mask")]
PACKED_CASES = [(2, 2, L, D, kind) for L in (65, 129) for D in (32, 64) for kind in ("plain", "causal")]
# (B, H, L, D, kind, p): dropout routes -- Dh 32 (flash_fwd_kernel), Dh 64 plain (flash_fwd2_kernel), Dh 64 + bias (flash_fwd_kernel)
DROP_ROUTES = ((32, "plain"), (64, "plain"), (64, "bias"))
DROP_CASES = [(2, 2, L, D, kind, p) for L in (33, 65, 129, 193) for D, kind in DROP_ROUTES for p in (0.1, 0.5)] + \
             [(2, 2, 129, D, kind + "+causal", p) for D, kind in DROP_ROUTES for p in (0.1, 0.5)]
BWD_NODROP_CASES = [(2, 2, L, D, kind, 0.0) for L in (65, 129, 193) for D in (32, 64) for kind in ("plain", "mask+causal+bias")]
DS_CASES = [(1, 2, L, D, kind, p) for L in (33, 65, 129) for D in (32, 64) for kind in ("plain", "causal") for p in (0.0, 0.3)]
GRAD_CASES = [(1, 2, L, D, kind, p) for L in (33, 65, 129) for D in (32, 64) for kind in ("plain", "mask+causal+bias") for p in (0.0, 0.3)]
DROP_SEED, DROP_POS, DROP_POS2 = 4321, 1000, 777777      # torch.manual_seed / ops._dropout_counter[0] before every probe launch


def case_seed(B, H, L, D):
    return 1000 * L + 10 * D + B + H


def case_id(c):
    return "-".join(str(x) for x in c)
