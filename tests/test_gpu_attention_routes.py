"""-m gpu: every row of tests/attention_route_cases.py whose tensors are small, through the public entry points (ops.attention /
attention_blhd / attention_packed).  Per row: (a) the C entry points that ran are the ones its (family, in place) implies -- attention.call
is replaced by a recorder that forwards to the real one -- and (b) the forward, and d(q, k, v) / d(bias) where the row has gradients, agree
with fp64 torch math.  Tolerances are those the kernels' own tests apply: fp32 families 1e-4 (test_gpu_flash_attention.py forward,
test_gpu_kernels.py _chk for gradients); bf16 families 2e-2 of the bf16 emulation and 6e-2 of exact attention in the forward, 2e-2 in
relative L2 for the gradients of the fused backward (test_flash_backward_*)."""
import functools

import pytest
import torch

from attention_route_cases import (BLOCK, FLASH_TRAIN, GPU_CASES, LONG, ROWS, case_id, device_tensors, entry_points, make_inputs,
                                   reference)
from gpu_util import DEV, linear_mode, rel_err
from mmskin import attention, ops

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case_data(key):
    """inputs and both references of a row, computed once per (shape, dtype, extras) -- several rows share them"""
    case = next(c for c in GPU_CASES if _key(c) == key)
    qkv, mask, bias, causal, dO = make_inputs(case)
    return (qkv, mask, bias, causal, dO), reference(qkv, mask, bias, causal, dO), reference(qkv, mask, bias, causal, dO, rounded=True)[0]


def _key(case):
    a = case[1]
    return a["B"], a["H"], a["L"], a["Dh"], a["dtype"], case[2]


def _run(case, monkeypatch, p=0.0, training=False, backward=True):
    """one call of the row's entry point under its mode and MMSKIN_FLASH_BWD with attention.call recorded
    -> (entry-point names, first pointer of the first call, the q tensor passed, out [B, L, H, Dh], d(qkv), d(bias))"""
    cid, a, extras, _, _ = case
    (qkv, mask, bias, causal, dO), _, _ = _case_data(_key(case))
    if a["flash_bwd"] == "0":
        monkeypatch.setenv("MMSKIN_FLASH_BWD", "0")
    else:
        monkeypatch.delenv("MMSKIN_FLASH_BWD", raising=False)
    calls = []
    real = attention.call

    def recorder(name, *args):
        calls.append((name, args[0].value))
        return real(name, *args)

    with linear_mode(a["mode"]):
        entry, ts, grad_of = device_tensors(case, qkv, DEV)
        bd = bias.to(DEV).requires_grad_(a["grad"]) if bias is not None else None
        with monkeypatch.context() as m, torch.set_grad_enabled(a["grad"]):
            m.setattr(attention, "call", recorder)
            out = getattr(ops, entry)(*ts, p, training, mask_add=None if mask is None else mask.to(DEV), bias=bd, causal=causal)
            token_major = out if entry != "attention" else out.permute(0, 2, 1, 3)
            if a["grad"] and backward:
                token_major.backward(dO.to(DEV))
        torch.cuda.synchronize()
    dqkv = grad_of() if a["grad"] and backward else None
    return [n for n, _ in calls], calls[0][1], ts[0], token_major.detach(), dqkv, (bd.grad if bd is not None and a["grad"] and backward else None)


def _chk(got, want, tol):
    if float((got.detach().cpu().double() - want.detach().double()).abs().max()) < 1e-5:
        return               # mathematically-zero gradients: absolute check (as test_gpu_kernels.py)
    assert rel_err(got, want) < tol, rel_err(got, want)


@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_route_runs_its_kernels_and_matches_fp64(case, monkeypatch):
    cid, a, extras, _, (family, in_place) = case
    _, (want, want_dqkv, want_dbias), emulated = _case_data(_key(case))
    names, first_ptr, q, out, dqkv, dbias = _run(case, monkeypatch)
    # (a) the entry points of the family, forward then backward; in place = the kernel was handed the caller's own q
    assert names == entry_points(family, a["grad"], a["grad"] and extras == "bias")
    if a["layout"] != "bhld":
        assert (first_ptr == q.data_ptr()) == in_place
    # (b) numbers
    assert tuple(out.shape) == (a["B"], a["L"], a["H"], a["Dh"])
    if family in (ROWS, BLOCK, LONG):
        print(f"{cid}: forward {rel_err(out, want):.3e}")
        assert rel_err(out, want) < 1e-4
        if a["grad"]:
            _chk(dqkv, want_dqkv, 1e-4)
            if dbias is not None:
                _chk(dbias, want_dbias, 1e-4)
        return
    print(f"{cid}: forward {rel_err(out, emulated):.3e} of the bf16 emulation, {rel_err(out, want):.3e} of exact")
    assert torch.isfinite(out).all()
    assert rel_err(out, emulated) < 2e-2
    assert rel_err(out, want) < 6e-2
    if a["grad"]:
        assert family == FLASH_TRAIN
        for name, got, ref in (("dq", dqkv[:, :, 0], want_dqkv[:, :, 0]), ("dk", dqkv[:, :, 1], want_dqkv[:, :, 1]),
                               ("dv", dqkv[:, :, 2], want_dqkv[:, :, 2]), ("dbias", dbias, want_dbias)):
            if got is None:
                continue
            l2 = float((got.double().cpu() - ref).norm() / ref.norm())
            print(f"{cid}: {name} relative L2 {l2:.3e}")
            assert torch.isfinite(got).all(), name
            assert l2 < 2e-2, (name, l2)


@pytest.mark.parametrize("case", GPU_CASES, ids=case_id)
def test_dropout_counter_advances_once_per_call(case, monkeypatch):
    """B * H * L * L counters per call when p > 0 and training, whatever the route (and however many routers it used to pass); none
    otherwise."""
    a = case[1]
    span = a["B"] * a["H"] * a["L"] * a["L"]
    ops._dropout_counter[0] = 12345
    _run(case, monkeypatch, 0.1, True, backward=False)
    assert ops._dropout_counter[0] == 12345 + span
    _run(case, monkeypatch, 0.1, False, backward=False)
    _run(case, monkeypatch, 0.0, True, backward=False)
    assert ops._dropout_counter[0] == 12345 + span
