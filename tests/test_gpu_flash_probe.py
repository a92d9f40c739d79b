"""-m gpu: the fused attention kernels read out element by element (tests/flash_probe.py) against an fp64 model of the same operation.

test_gpu_flash_attention.py holds these kernels to norm-level bounds on outputs and whole gradients; here every probability the
kernels multiplied, every dropout bit, every row log-sum-exp and every dS entry is compared on its own, on bf16-representable inputs,
so the only error left is the kernels' own arithmetic.  Which kernel a test pins:
  (a) probabilities, forward         flash_fwd_kernel / flash_fwd2_kernel (the launcher's choice is part of each case id)
  (b) row log-sum-exp                the same two, through attention._flash_forward with an lse buffer
  (c) dropout mask, forward          flash_fwd_kernel<.., true> (Dh 32; Dh 64 + bias) and flash_fwd2_kernel<.., true> (Dh 64 plain)
  (d) probabilities / mask, backward flash_bwd_dkv_kernel (dV under a probe dO)
  (e) dS per element                 flash_delta_kernel + flash_bwd_dq_kernel (d(bias) of a zero bias at B = 1)
  (f) dQ, dK, dV                     all three backward kernels, against fp64 and beside the unfused fp32 chain
Every test first asserts the route (attention._route in bf16-operand mode), so a fall-back to the unfused chain cannot let it pass.  The
router gives trainable attention of L <= 64 to the one-wave-per-head fp32 kernels, so the L = 33 cases of (d) - (f) call the fused
Function (attention.FlashAttnFn) directly and assert that the route is NOT FLASH_TRAIN there; the kernels have no such limit.
A -inf tail of the key mask is min(3, L - 1) keys long (flash_probe.key_mask): a row with no finite key has no softmax.
Measured on an MI355X, worst ratio against the bound: (a) 0.995 (fp32 tensors, 2^-8), 0.98 (bf16 tensors, 2^-7); (b) 2.3e-7 of 1e-5;
(c) every mask bit equal, kept entries 0.996 of 2^-8, kept shares 0.4927 - 0.9004; (d) |dP| / P 8.5e-6 against 2^-8, masks equal; (e) 0.21;
(f) unfused 6.2e-6 of 1e-4, fused per element 0.20 of the derived bound, fused over rms 1.87e-2 of the 2e-2 cap.  The whole module runs
in about 5 s."""
import functools

import pytest
import torch

import flash_probe as fp
from gpu_util import DEV, linear_mode
from mmskin import attention, ops
from mmskin._lib import call, ptr, stream

pytestmark = pytest.mark.gpu


def _dev(t):
    return None if t is None else t.to(DEV)


@functools.lru_cache(maxsize=4)
def _case(B, H, L, D, kind):
    """(q, k, v, dO, mask_add, bias, causal) of a case on the CPU -- computed once, shared, never written to"""
    return (*fp.inputs(B, H, L, D, fp.case_seed(B, H, L, D)), *fp.extras(kind, B, H, L))


@functools.lru_cache(maxsize=4)
def _model(B, H, L, D, kind):
    q, k, v, dO, mask_add, bias, causal = _case(B, H, L, D, kind)
    return fp.model_fp64(q, k, v, mask_add, bias, causal)


def _seed(pos):
    """the generator position of the next attention call (the idiom of test_gpu_flash_attention.py) -> the seed that call will use"""
    torch.manual_seed(fp.DROP_SEED)
    ops._dropout_counter[0] = pos
    return torch.initial_seed() & 0xFFFFFFFFFFFFFFFF


@functools.lru_cache(maxsize=4)
def _ref_keep(B, H, L, p, pos):
    """the mask the unfused path draws at that position: the `mask` output of mmskin_attn_dropout_forward on a [B, H, L, L] tensor of ones"""
    ones = torch.ones(B, H, L, L, device=DEV)
    y, mask = torch.empty_like(ones), torch.empty(ones.shape, device=DEV, dtype=torch.uint8)
    call("mmskin_attn_dropout_forward", ptr(ones), ptr(y), ptr(mask), ones.numel(), L, float(p), _seed(pos), int(pos), stream())
    return mask.cpu().bool()


@functools.lru_cache(maxsize=4)
def _read_forward(B, H, L, D, kind, p=0.0, pos=0, io="fp32"):
    """the [B, H, L, L] matrix the forward kernel multiplied, through ops.attention without gradients: ceil(L / D) probe launches"""
    q, k, _, _, mask_add, bias, causal = _case(B, H, L, D, kind)
    dt = torch.bfloat16 if io == "bf16" else torch.float32
    qd, kd, md, bd = _dev(q).to(dt), _dev(k).to(dt), _dev(mask_add), _dev(bias)
    blocks = []
    with linear_mode("bf16"), torch.no_grad():
        for blk in range(fp.n_blocks(L, D)):
            vd = fp.probe_v(L, D, blk).to(DEV).to(dt).expand(B, H, L, D).contiguous()
            assert attention._route("bhld", B, H, L, D, qd, kd, vd, md, bd, causal)[0] == attention.FLASH
            if p > 0:
                _seed(pos)
            out = ops.attention(qd, kd, vd, p, p > 0, mask_add=md, bias=bd, causal=causal)
            assert out.dtype == dt
            blocks.append(out)
    return fp.assemble(blocks, L)


def _fused_train(qd, kd, vd, md, bd, causal, p, pos):
    """trainable fused attention: ops.attention where the router sends it to FLASH_TRAIN (L > 64), the same Function called directly
    below that -- in bf16-operand mode, at generator position `pos`"""
    B, H, L, D = qd.shape
    family = attention._route("bhld", B, H, L, D, qd, kd, vd, md, bd, causal)[0]
    seed = _seed(pos)
    if L > 64:
        assert family == attention.FLASH_TRAIN, family
        return ops.attention(qd, kd, vd, p, p > 0, mask_add=md, bias=bd, causal=causal)
    assert family != attention.FLASH_TRAIN, family
    return attention.FlashAttnFn.apply(qd, kd, vd, md, bd, causal, p, seed if p > 0 else 0, pos if p > 0 else 0)


def _fwd_id(c):
    return fp.case_id(c) + "-" + fp.forward_kernel(c[3], "bias" in c[4], c[2])


# ---------------------------------------------------------------------------------------------- (a) probabilities, forward
@pytest.mark.parametrize("io", ["fp32", "bf16"])
@pytest.mark.parametrize("case", fp.FWD_CASES, ids=_fwd_id)
def test_forward_probabilities_per_element(case, io):
    """|got - P| <= 2^-8 P + 1e-30 per element (fp32 tensors; 2^-7 P with bf16 tensors, whose O is rounded once more on the way out):
    between the fp32 score and the read-out lies ONE bf16 rounding of the un-normalised probability; the running-maximum rescale, the
    row sum and the division are fp32 and the fp32 score accumulation moves P by ~1e-5.  Masked entries (causal, -inf) read back as
    exactly 0.0 and every row sums to 1 within 2^-8.
    Measured on an MI355X, worst |dP| / P over all 104 cases: 1.99 x 2^-9 (fp32 tensors, both kernels, the packed layout too),
    3.93 x 2^-9 (bf16 tensors); worst |row sum - 1| 3.9e-3.  That is above 1.1 x 2^-9 and NO conversion truncates: f32_to_bf16_bits is
    v_cvt_pk_bf16_f32, round to nearest even.  bf16 has 8 significant bits, so round-to-nearest errs by 2^-9 only just below a power
    of two and by 2^-8 / (1 + 2^-8) = 0.996 x 2^-8 just above one -- the measured 0.995 x 2^-8 is that worst case.  The bound 2^-8 is
    therefore the rounding's own worst case, not twice it; a truncating conversion would reach 2^-7 and fail, as does a wrong element."""
    B, H, L, D, kind = case
    kernel = fp.forward_kernel(D, "bias" in kind, L)
    assert kernel == ("flash_fwd2_kernel" if D == 64 and "bias" not in kind and L <= 1024 else "flash_fwd_kernel")
    m = _model(*case)
    got = _read_forward(*case, io=io)
    r = fp.check_probs(got, m.P, m.masked, rel=fp.P_REL if io == "fp32" else 2 * fp.P_REL)
    s = fp.check_row_sums(got)
    print(f"(a) {fp.case_id(case)} {io} {kernel}: worst |dP|/P = {r:.3e} = {r / fp.EPS_BF16:.2f} x 2^-9, worst |row sum - 1| = {s:.2e}")


@pytest.mark.parametrize("case", fp.PACKED_CASES, ids=_fwd_id)
def test_forward_probabilities_on_the_packed_layout(case):
    """the same read-out with q, k and the probe V as strided views of one [B, L, 3, H, Dh] tensor (ops.attention_packed, token-major O)"""
    B, H, L, D, kind = case
    q, k, _, _, mask_add, bias, causal = _case(*case)
    m = _model(*case)
    blocks = []
    with linear_mode("bf16"), torch.no_grad():
        qkv = torch.zeros(B, L, 3, H, D, device=DEV)
        qkv[:, :, 0], qkv[:, :, 1] = _dev(q).permute(0, 2, 1, 3), _dev(k).permute(0, 2, 1, 3)
        for blk in range(fp.n_blocks(L, D)):
            qkv[:, :, 2] = fp.probe_v(L, D, blk).to(DEV)[None, :, None, :]
            assert attention._route("packed", B, H, L, D, qkv, None, None, None, None, causal) == (attention.FLASH, True)
            out = ops.attention_packed(qkv, causal=causal)
            assert out.shape == (B, L, H, D)
            blocks.append(out.permute(0, 2, 1, 3))
    got = fp.assemble(blocks, L)
    r = fp.check_probs(got, m.P, m.masked)
    fp.check_row_sums(got)
    print(f"(a) packed {fp.case_id(case)}: worst |dP|/P = {r:.3e}")


# ---------------------------------------------------------------------------------------------- (b) row log-sum-exp
def _lse(q, k, v, mask_add, bias, causal):
    B, H, L, D = q.shape
    qd, kd, vd, md, bd = _dev(q), _dev(k), _dev(v), _dev(mask_add), _dev(bias)
    out, lse = torch.empty_like(qd), torch.empty(B, H, L, device=DEV)
    with linear_mode("bf16"), torch.no_grad():
        assert attention._route("bhld", B, H, L, D, qd, kd, vd, md, bd, causal)[0] == attention.FLASH
        attention._flash_forward(qd, kd, vd, out, lse, (B, H, L, D), (0, 1, 2), md, bd, causal, 0.0, 0, 0)      # as FlashAttnFn.forward does
    return lse.cpu(), out.cpu()


@pytest.mark.parametrize("case", fp.FWD_CASES, ids=_fwd_id)
def test_row_log_sum_exp(case):
    """the LSE the forward hands to the backward: |got - LSE| <= 1e-5 max(1, |LSE|) (fp32 accumulation of at most 1025 terms and a log);
    flash_fwd2_kernel keeps its running maximum in the log2 domain and converts at the end -- this is the check of that conversion"""
    q, k, v, _, mask_add, bias, causal = _case(*case)
    m = _model(*case)
    lse, out = _lse(q, k, v, mask_add, bias, causal)
    r = fp.check_lse(lse, m.LSE)
    assert fp.rms_err(out, m.O) < 2e-2
    print(f"(b) {_fwd_id(case)}: worst |dLSE| / max(1, |LSE|) = {r:.3e}")


@pytest.mark.parametrize("D", [32, 64])
def test_row_log_sum_exp_of_a_fully_finite_masked_entry(D):
    """finfo.min on every key of batch entry 1: its rows are uniform and their LSE is the common score + log L = finfo.min (the log is
    below its rounding), within the same bound.  flash_fwd2_kernel (Dh 64) clamps mask . log2 e at -FLT_MAX and used to convert that back
    as -FLT_MAX ln 2 = -2.36e38: measured 0.307 |LSE| off before the fix (1.2e-7 after; Dh 32: 1.4e-7), and exp(x - lse) = 0 for every
    probability the backward recomputed from it."""
    B, H, L = 2, 2, 130
    q, k, v, _ = fp.inputs(B, H, L, D, 21)
    mask = torch.zeros(B, L)
    mask[1, :] = torch.finfo(torch.float32).min
    m = fp.model_fp64(q, k, v, mask)
    uniform = float(torch.finfo(torch.float32).min) + torch.log(torch.tensor(float(L), dtype=torch.float64))
    assert float((m.LSE[1] - uniform).abs().max()) <= 1e-9 * abs(float(uniform))
    assert float((m.P[1] - 1.0 / L).abs().max()) <= 1e-12
    lse, out = _lse(q, k, v, mask, None, False)
    r = fp.check_lse(lse, m.LSE)
    assert fp.rms_err(out[1], m.O[1]) < 2e-2
    print(f"(b) fully masked, Dh {D} {fp.forward_kernel(D, False, L)}: worst |dLSE| / max(1, |LSE|) = {r:.3e}")


# ---------------------------------------------------------------------------------------------- (c) dropout mask, forward
@pytest.mark.parametrize("case", fp.DROP_CASES, ids=lambda c: _fwd_id(c[:5]) + f"-p{c[5]}")
def test_forward_dropout_mask_is_the_unfused_paths_exactly(case):
    """The zero pattern of the read-out is torch.equal to the mask the unfused path draws at the same generator position, on every
    entry whose undropped probability is above 1e-20 -- which is every unmasked entry of these cases (N(0,1) inputs, no key mask:
    test_cpu_flash_probe.test_dropout_cases_stay_above_the_floor).  Kept entries are P / (1 - p) to the bound of (a), the kept share
    lies within 5 binomial standard deviations of 1 - p, and a second position gives a different mask, again the unfused path's."""
    B, H, L, D, kind, p = case
    m = _model(B, H, L, D, kind)
    got, keep = _read_forward(B, H, L, D, kind, p, fp.DROP_POS), _ref_keep(B, H, L, p, fp.DROP_POS)
    n = fp.check_mask(got, keep, m.P)
    assert n == int((~m.masked).sum())
    share = fp.check_keep_share(got != 0, p, ~m.masked)
    r = fp.check_probs(got * (1.0 - p), m.P * keep, m.masked)
    got2, keep2 = _read_forward(B, H, L, D, kind, p, fp.DROP_POS2), _ref_keep(B, H, L, p, fp.DROP_POS2)
    fp.check_mask(got2, keep2, m.P)
    assert not torch.equal((got2 != 0)[~m.masked], (got != 0)[~m.masked])
    print(f"(c) {fp.case_id(case)} {fp.forward_kernel(D, 'bias' in kind, L)}: {n} bits equal, kept share {share:.4f}, worst |dP|/P = {r:.3e}")


# ---------------------------------------------------------------------------------------------- (d) the backward's probabilities and mask
@pytest.mark.parametrize("case", fp.DROP_CASES + fp.BWD_NODROP_CASES, ids=fp.case_id)
def test_backward_recomputes_the_probabilities_and_the_mask(case):
    """dV under a probe dO is the probability matrix as flash_bwd_dkv_kernel recomputed it (exp(x - lse), the NORMALISED probability,
    split into bf16 hi + lo as the MFMA operands) under the mask it regenerated: per element within 2^-8 P + 1e-30 of the model, masked
    entries exactly 0.0, and with dropout the zero pattern torch.equal to the unfused path's mask and to the forward's read-out of (c).
    Measured worst |dP| / P: 8.5e-6, fp32 arithmetic alone (0.995 x 2^-8 while the operand was rounded to bf16 once)."""
    B, H, L, D, kind, p = case
    q, k, v, _, mask_add, bias, causal = _case(B, H, L, D, kind)
    m = _model(B, H, L, D, kind)
    with linear_mode("bf16"):
        qd, kd, vd = (_dev(t).requires_grad_(True) for t in (q, k, v))
        out = _fused_train(qd, kd, vd, _dev(mask_add), _dev(bias), causal, p, fp.DROP_POS)
        blocks = [torch.autograd.grad(out, vd, fp.probe_do(L, D, blk).to(DEV).expand(B, H, L, D).contiguous(), retain_graph=True)[0]
                  for blk in range(fp.n_blocks(L, D))]
    got = fp.assemble(blocks, L, transpose=True)
    keep = _ref_keep(B, H, L, p, fp.DROP_POS) if p > 0 else torch.ones(B, H, L, L, dtype=torch.bool)
    r = fp.check_probs(got * (1.0 - p), m.P * keep, m.masked)
    if p > 0:
        fp.check_mask(got, keep, m.P)
        fwd = _read_forward(B, H, L, D, kind, p, fp.DROP_POS)
        assert torch.equal((got != 0)[~m.masked], (fwd != 0)[~m.masked])
    print(f"(d) {fp.case_id(case)}: worst |dP|/P = {r:.3e} = {r / fp.EPS_BF16:.2f} x 2^-9")


# ---------------------------------------------------------------------------------------------- (e) dS per element
@pytest.mark.parametrize("case", fp.DS_CASES, ids=fp.case_id)
def test_ds_per_element(case):
    """d(bias) of a zero [H, L, L] bias at B = 1 is ds_out itself (the batch sum has one term).  Bound per element:
    |got - dS_ij| <= 2^-8 / (1 - p) . P_ij . max_j' |dP_ij'| + 1e-6 max |dS|.  ds_out = pr (dp zs - delta) is stored from fp32 -- pr, dp
    (bf16-exact operands, fp32 MFMA) and zs carry fp32 errors only (the 1e-6 term); the one bf16-level error is in
    delta_i = sum_d dO_id O_id = sum_j Pd_ij dP_ij, built from an O whose probabilities the forward rounded to bf16:
    |d delta_i| <= 2^-9 sum_j Pd_ij |dP_ij| <= 2^-9 / (1 - p) max_j |dP_ij|, times P_ij, and the bound is twice that.  No further
    rounding lies on the way to ds_out (the bf16 conversion of dS feeds the dQ MFMA only).  Masked entries stay exactly 0.0: the
    launcher zero-fills and the kernel skips them."""
    B, H, L, D, kind, p = case
    q, k, v, dO, _, _, causal = _case(B, H, L, D, kind)
    with linear_mode("bf16"):
        zero = torch.zeros(H, L, L, device=DEV, requires_grad=True)
        out = _fused_train(_dev(q), _dev(k), _dev(v), None, zero, causal, p, fp.DROP_POS)
        out.backward(_dev(dO))
    keep = _ref_keep(B, H, L, p, fp.DROP_POS) if p > 0 else None
    m = fp.model_fp64(q, k, v, None, None, causal, dO=dO, keep=keep, p=p)
    r = fp.check_ds(zero.grad[None].cpu(), m, p)
    print(f"(e) {fp.case_id(case)}: worst |d dS| / bound = {r:.3f}")


# ---------------------------------------------------------------------------------------------- (f) dQ, dK, dV
GRAD_BOUND = 2e-2          # 2 x the worst measured value (1.87e-2) would be 3.7e-2: the cap of 2e-2 holds instead


@pytest.mark.parametrize("case", fp.GRAD_CASES, ids=fp.case_id)
def test_gradients_on_representable_inputs(case, monkeypatch):
    """dQ, dK, dV of the fused backward against model_fp64's on bf16-representable q, k, v, dO.  Three assertions: the unfused fp32 chain of
    this package (MMSKIN_FLASH_BWD=0) within 1e-4 of the reference (measured: 6.2e-6 at worst); every fused element within
    flash_probe.grad_bounds, derived from what (b), (d) and (e) pin (measured: 0.20 / 0.10 / 0.04 of it at worst for dq / dk / dv); and the
    fused worst-element error over the rms within GRAD_BOUND = min(2 x worst measured, 2e-2) = 2e-2, a quarter of
    test_gpu_flash_attention.py's 8e-2.
    This test found the backward wrong by that cap: with dS and P^T rounded ONCE to bf16 as MFMA operands (2^-8 of each term, on
    heavy-tailed softmax weights) 9 of the 24 cases missed it -- worst 3.25e-2 (dK), 2.56e-2 (dV), 2.37e-2 (dQ).  flash_bwd_dq_kernel and
    flash_bwd_dkv_kernel now feed both operands as bf16 hi + lo (16 significant bits, two MFMAs per fragment).  What remains in dQ / dK is
    delta, built from the forward's O whose probabilities are rounded to bf16 (the term (e) bounds); dV has no such term.
    MEASURED on an MI355X after that change, worst element over rms in units of 1e-3, dq/dk/dv per case (B-H-L-D-kind-p):
    1-2-33-32-plain-0.0 2.96/1.88/0.01;  1-2-33-32-plain-0.3 7.32/4.74/0.03;  1-2-33-32-mask+causal+bias-0.0 4.31/4.24/0.02;
    1-2-33-32-mask+causal+bias-0.3 10.70/18.70/0.03;  1-2-33-64-plain-0.0 3.00/2.47/0.02;  1-2-33-64-plain-0.3 4.39/2.24/0.03;
    1-2-33-64-mask+causal+bias-0.0 5.28/5.31/0.02;  1-2-33-64-mask+causal+bias-0.3 6.74/9.86/0.03;
    1-2-65-32-plain-0.0 2.90/2.20/0.01;  1-2-65-32-plain-0.3 3.32/2.55/0.02;  1-2-65-32-mask+causal+bias-0.0 6.16/6.19/0.04;
    1-2-65-32-mask+causal+bias-0.3 8.94/7.77/0.02;  1-2-65-64-plain-0.0 2.36/1.29/0.02;  1-2-65-64-plain-0.3 2.69/1.70/0.01;
    1-2-65-64-mask+causal+bias-0.0 8.17/6.24/0.03;  1-2-65-64-mask+causal+bias-0.3 11.80/12.10/0.03;
    1-2-129-32-plain-0.0 2.38/1.66/0.02;  1-2-129-32-plain-0.3 4.91/3.03/0.02;  1-2-129-32-mask+causal+bias-0.0 5.84/4.46/0.03;
    1-2-129-32-mask+causal+bias-0.3 12.50/17.30/0.03;  1-2-129-64-plain-0.0 1.75/1.50/0.02;  1-2-129-64-plain-0.3 2.19/2.05/0.04;
    1-2-129-64-mask+causal+bias-0.0 6.17/5.76/0.04;  1-2-129-64-mask+causal+bias-0.3 13.20/14.30/0.04"""
    B, H, L, D, kind, p = case
    q, k, v, dO, mask_add, bias, causal = _case(B, H, L, D, kind)
    keep = _ref_keep(B, H, L, p, fp.DROP_POS) if p > 0 else None
    m = fp.model_fp64(q, k, v, mask_add, bias, causal, dO=dO, keep=keep, p=p)

    def grads(fn):
        leaves = [_dev(t).requires_grad_(True) for t in (q, k, v)]
        fn(*leaves).backward(_dev(dO))
        return [t.grad.cpu() for t in leaves]

    with linear_mode("bf16"):
        fused = grads(lambda a, b, c: _fused_train(a, b, c, _dev(mask_add), _dev(bias), causal, p, fp.DROP_POS))
        monkeypatch.setenv("MMSKIN_FLASH_BWD", "0")

        def chain(a, b, c):
            assert attention._route("bhld", B, H, L, D, a, b, c, mask_add, bias, causal)[0] in (attention.LONG, attention.ROWS, attention.BLOCK)
            _seed(fp.DROP_POS)
            return ops.attention(a, b, c, p, p > 0, mask_add=_dev(mask_add), bias=_dev(bias), causal=causal)
        unfused = grads(chain)
    ef = [fp.rms_err(g, w) for g, w in zip(fused, (m.dQ, m.dK, m.dV))]
    eu = [fp.rms_err(g, w) for g, w in zip(unfused, (m.dQ, m.dK, m.dV))]
    print(f"(f) {fp.case_id(case)}: fused dq {ef[0]:.2e} dk {ef[1]:.2e} dv {ef[2]:.2e} | unfused dq {eu[0]:.2e} dk {eu[1]:.2e} dv {eu[2]:.2e}")
    assert all(torch.isfinite(g).all() for g in fused)
    rb_ = [float(((g.double() - w).abs() / bd).max()) for g, w, bd in zip(fused, (m.dQ, m.dK, m.dV), fp.grad_bounds(m, q, k, dO, p))]
    print(f"(f) {fp.case_id(case)}: worst element over its derived bound dq {rb_[0]:.3f} dk {rb_[1]:.3f} dv {rb_[2]:.3f}")
    assert max(eu) <= 1e-4, eu
    assert max(rb_) <= 1.0, rb_
    assert max(ef) <= GRAD_BOUND, ef
