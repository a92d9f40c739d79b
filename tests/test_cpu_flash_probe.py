"""The probe harness of tests/flash_probe.py proves itself on the CPU: run through a plain fp64 torch attention (forward and autograd
backward, with a known random keep mask and the 1/(1-p) factor) the probes must hand back exactly that mask and those probabilities;
model_fp64's dS must be autograd's gradient with respect to a zero bias; and the comparison functions the GPU tests use must REJECT a
deliberately corrupted attention (two neighbouring keys' mask bits swapped, one probability scaled by 1.01, key L-1 treated as invalid).
Also here: the dropout cases of the GPU tests keep every undropped probability above the floor under which a zero is not read as a drop."""
import math

import pytest
import torch

import flash_probe as fp

P_DROP = 0.25


def _dense(q, k, v, mask_add, bias, causal, keep=None, p=0.0, corrupt=None):
    """softmax attention in fp64, written out; corrupt: None or one of the three deliberate faults"""
    L, D = q.shape[2], q.shape[3]
    s = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(D)
    if bias is not None:
        s = s + bias.double()[None]
    if mask_add is not None:
        s = s + mask_add.double()[:, None, None, :]
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(L, L, dtype=torch.bool), 1), float("-inf"))
    if corrupt == "last_key_invalid":
        s = s.clone()
        s[..., L - 1] = float("-inf")
    pr = torch.softmax(s, -1)
    if corrupt == "scaled":
        pr = pr.clone()
        pr[-1, -1, L // 2, L // 3] *= 1.01
    if keep is not None:
        if corrupt == "swapped_bits":
            keep = keep.clone()
            row = keep[0, 0, L // 2]
            j = int((row[1:] != row[:-1]).nonzero()[0])          # a neighbouring pair whose bits differ
            row[j], row[j + 1] = row[j + 1].clone(), row[j].clone()
        pr = pr * keep.double() / (1.0 - p)
    return pr @ v.double()


def _keep(B, H, L, seed):
    return torch.rand(B, H, L, L, generator=torch.Generator().manual_seed(seed)) >= P_DROP


def _read_forward(q, k, mask_add, bias, causal, keep, p, corrupt=None):
    B, H, L, D = q.shape
    return fp.assemble([_dense(q, k, fp.probe_v(L, D, blk).expand(B, H, L, D), mask_add, bias, causal, keep, p, corrupt)
                        for blk in range(fp.n_blocks(L, D))], L)


@pytest.mark.parametrize("kind", ["causal", "mask", "bias", "mask+causal+bias"])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("L", [1, 65, 130])
def test_probes_return_the_mask_and_the_probabilities_exactly(L, D, kind):
    B, H = 2, 2
    q, k, v, dO = fp.inputs(B, H, L, D, fp.case_seed(B, H, L, D))
    mask_add, bias, causal = fp.extras(kind, B, H, L)
    keep = _keep(B, H, L, L + D)
    m = fp.model_fp64(q, k, v, mask_add, bias, causal, keep=keep, p=P_DROP)
    # the model against softmax written the torch way
    s = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(D)
    s = s + (bias.double()[None] if bias is not None else 0.0) + (mask_add.double()[:, None, None, :] if mask_add is not None else 0.0)
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(L, L, dtype=torch.bool), 1), float("-inf"))
    want = torch.softmax(s, -1)
    assert float((m.P - want).abs().max()) <= 1e-12 and float((m.LSE - torch.logsumexp(s, -1)).abs().max()) <= 1e-12
    assert torch.equal(m.masked, torch.isneginf(s))
    assert float((m.O - _dense(q, k, v, mask_add, bias, causal, keep, P_DROP)).abs().max()) <= 1e-12
    # forward probe: O = Pd
    got = _read_forward(q, k, mask_add, bias, causal, keep, P_DROP)
    assert got.shape == (B, H, L, L)
    assert float((got - want * keep / (1.0 - P_DROP)).abs().max()) <= 1e-12
    assert torch.equal(got != 0, keep & (want > 0))
    fp.check_mask(got, keep, want)
    assert fp.check_probs(got * (1.0 - P_DROP), want * keep, masked=m.masked) <= 1e-12
    assert fp.check_row_sums(_read_forward(q, k, mask_add, bias, causal, None, 0.0)) <= 1e-12
    # backward probe: dV = Pd^T through autograd
    vv = v.double().requires_grad_(True)
    out = _dense(q, k, vv, mask_add, bias, causal, keep, P_DROP)
    blocks = [torch.autograd.grad(out, vv, fp.probe_do(L, D, blk).double().expand(B, H, L, D), retain_graph=True)[0]
              for blk in range(fp.n_blocks(L, D))]
    got_b = fp.assemble(blocks, L, transpose=True)
    assert float((got_b - want * keep / (1.0 - P_DROP)).abs().max()) <= 1e-12
    fp.check_mask(got_b, keep, want)


@pytest.mark.parametrize("kind", ["plain", "causal", "mask+causal+bias"])
@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("L,D", [(1, 32), (65, 32), (65, 64), (130, 64)])
def test_model_ds_is_autograds_gradient_of_a_zero_bias(L, D, kind, p):
    B, H = 1, 2
    q, k, v, dO = fp.inputs(B, H, L, D, fp.case_seed(B, H, L, D))
    mask_add, bias, causal = fp.extras(kind, B, H, L)
    keep = _keep(B, H, L, L) if p > 0 else None
    m = fp.model_fp64(q, k, v, mask_add, bias, causal, dO=dO, keep=keep, p=p)
    zero = torch.zeros(H, L, L, dtype=torch.float64, requires_grad=True)
    leaves = [t.double().requires_grad_(True) for t in (q, k, v)]
    out = _dense(*leaves, mask_add, zero if bias is None else bias.double() + zero, causal, keep, p)
    out.backward(dO.double())
    assert float((zero.grad - m.dS[0]).abs().max()) <= 1e-12 * max(1.0, float(m.dS.abs().max()))
    for got, want in zip((t.grad for t in leaves), (m.dQ, m.dK, m.dV)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert fp.check_ds(zero.grad[None], m, p) <= 1e-6
    assert bool((m.dS[m.masked] == 0).all())


@pytest.mark.parametrize("L,D", [(65, 32), (130, 64)])
def test_comparisons_reject_a_corrupted_attention(L, D):
    """the teeth: each fault is one the norm-level bounds of test_gpu_flash_attention.py let through"""
    B, H = 2, 2
    q, k, v, _ = fp.inputs(B, H, L, D, fp.case_seed(B, H, L, D))
    keep = _keep(B, H, L, 7)
    m = fp.model_fp64(q, k, v)
    good = _read_forward(q, k, None, None, False, keep, P_DROP)
    fp.check_mask(good, keep, m.P)
    fp.check_probs(good * (1.0 - P_DROP), m.P * keep)
    # two neighbouring keys' mask bits swapped: the output moves by two probabilities of ~1/L in one row
    bad = _read_forward(q, k, None, None, False, keep, P_DROP, corrupt="swapped_bits")
    with pytest.raises(AssertionError, match="dropout mask differs at 2 of"):
        fp.check_mask(bad, keep, m.P)
    # one (query, key) probability scaled by 1.01
    plain = _read_forward(q, k, None, None, False, None, 0.0)
    assert fp.check_probs(plain, m.P) <= 1e-12
    bad = _read_forward(q, k, None, None, False, None, 0.0, corrupt="scaled")
    assert fp.rms_err(_dense(q, k, v, None, None, False, corrupt="scaled"), m.O) < 2e-2        # invisible to the output-level bound
    with pytest.raises(AssertionError, match="probability at"):
        fp.check_probs(bad, m.P)
    # key L-1 treated as invalid (a validity test off by one on the last ragged key)
    bad = _read_forward(q, k, None, None, False, None, 0.0, corrupt="last_key_invalid")
    fp.check_row_sums(bad)                                                                       # still a softmax: the row sums do not see it
    with pytest.raises(AssertionError, match="probability at"):
        fp.check_probs(bad, m.P)
    # the LSE and dS comparisons: a log2 / ln mix-up of the running maximum, and one dS entry off by 2 % of its largest neighbour
    with pytest.raises(AssertionError, match="LSE off"):
        fp.check_lse(m.LSE * (1.0 + 2e-5) + 2e-5, m.LSE)
    md = fp.model_fp64(q, k, v, dO=fp.inputs(B, H, L, D, 5)[3])
    fp.check_ds(md.dS, md)
    bad = md.dS.clone()
    i = int(md.P[0, 0, 3].argmax())
    bad[0, 0, 3, i] += 0.02 * float(md.P[0, 0, 3, i] * md.dP[0, 0, 3].abs().max())
    with pytest.raises(AssertionError, match="dS off"):
        fp.check_ds(bad, md)
    with pytest.raises(AssertionError, match="kept share"):
        fp.check_keep_share(torch.ones(B, H, L, L, dtype=torch.bool), 0.1)


@pytest.mark.parametrize("case", fp.GRAD_CASES[::3], ids=fp.case_id)
def test_derived_bounds_hold_for_the_kernels_arithmetic_emulated_in_fp64(case):
    """the stated roundings alone (P -> bf16 inside the forward's O, P and scale . dS -> bf16 hi + lo as the backward's operands) stay inside
    ds_bound and grad_bounds; a single bf16 rounding of those operands does not"""
    B, H, L, D, kind, p = case
    q, k, v, dO = fp.inputs(B, H, L, D, fp.case_seed(B, H, L, D))
    mask_add, bias, causal = fp.extras(kind, B, H, L)
    keep = _keep(B, H, L, 3) if p > 0 else None
    m = fp.model_fp64(q, k, v, mask_add, bias, causal, dO=dO, keep=keep, p=p)
    zs = 1.0 if keep is None else keep.double() / (1.0 - p)
    rb64 = lambda t: fp.rb(t.float()).double()
    delta = (dO.double() * (rb64(m.Pd) @ v.double())).sum(-1)
    ds = m.P * (m.dP * zs - delta[..., None])
    fp.check_ds(ds, m, p)
    split = lambda t: rb64(t) + rb64(t - rb64(t))          # the backward's hi + lo operands
    got = (split(ds * m.scale) @ k.double(), split(ds * m.scale).transpose(-1, -2) @ q.double(), split(m.Pd).transpose(-1, -2) @ dO.double())
    bounds = fp.grad_bounds(m, q, k, dO, p)
    for g, w, bd in zip(got, (m.dQ, m.dK, m.dV), bounds):
        assert float(((g - w).abs() / bd).max()) <= 1.0
    assert float(((rb64(m.Pd).transpose(-1, -2) @ dO.double() - m.dV).abs() / bounds[2]).max()) > 1.0


@pytest.mark.parametrize("case", fp.DROP_CASES, ids=fp.case_id)
def test_dropout_cases_stay_above_the_floor(case):
    """no undropped probability of the GPU dropout cases falls below DROP_FLOOR: a zero in their read-outs is a drop, never an underflow"""
    B, H, L, D, kind, p = case
    q, k, v, _ = fp.inputs(B, H, L, D, fp.case_seed(B, H, L, D))
    m = fp.model_fp64(q, k, v, *fp.extras(kind, B, H, L))
    assert float(m.P[~m.masked].min()) > fp.DROP_FLOOR


def test_case_tables_name_the_kernel_the_launcher_selects():
    assert fp.forward_kernel(64, False, 1024) == "flash_fwd2_kernel" and fp.forward_kernel(64, False, 1025) == "flash_fwd_kernel"
    assert fp.forward_kernel(64, True, 65) == "flash_fwd_kernel" and fp.forward_kernel(32, False, 65) == "flash_fwd_kernel"
    assert len(fp.FWD_CASES) == 104 and all(B <= 2 and H <= 2 for B, H, *_ in fp.FWD_CASES)
    assert {L for _, _, L, *_ in fp.FWD_CASES} == set(fp.FWD_LS) | {1024, 1025}
    m = fp.key_mask(2, 65)
    assert int(torch.isneginf(m[1]).sum()) == 3 and int((m[0] == -10000.0).sum()) == 33 and not bool(torch.isneginf(fp.key_mask(2, 1)).any())
    assert torch.equal(fp.probe_v(70, 32, 2)[64:70, :6], torch.eye(6)) and float(fp.probe_v(70, 32, 2).sum()) == 6.0
