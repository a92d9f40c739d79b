"""The Linear route table of csrc/linear.hip (linear_path) as data, and the fp64 reference the route tests share.  No GPU needed to import:
tests/test_cpu_linear_routes.py asks the library for the route of every row, tests/test_gpu_linear_routes.py runs them.

Each row is (mode, M, K, N, route).  The comment behind a row names the branch of linear.hip the shape stands on."""
import math

import torch

from mmskin import _lib

SMALL, BIG_F32, BIG_BF16, PADDED = _lib.LINEAR_SMALL, _lib.LINEAR_BIG_F32, _lib.LINEAR_BIG_BF16, _lib.LINEAR_PADDED_BF16

ROUTE_CASES = [
    # ---- LIN_SMALL, fp32 mode: gemm_f32 forward, linear_bwd_small_kernel (M < 4096) or separate gemm_f32 launches + colsum backward
    ("fp32", 1, 1, 1, SMALL),          # gemm_f32_tile: one element, every tile guard (m < M, n < N, k < K) at its edge
    ("fp32", 1, 129, 1, SMALL),        # gemm_f32_tile: K = LG_BK + 1, a second K step of one element
    ("fp32", 31, 127, 33, SMALL),      # gemm_f32: one tile short of LG_T rows / two tiles of columns, K one short of LG_BK
    ("fp32", 33, 130, 31, SMALL),      # gemm_f32: the mirror image (ragged second row tile, K = LG_BK + 2)
    ("fp32", 2047, 64, 64, SMALL),     # linear_big: M >= 2048 fails by one row
    ("fp32", 2048, 64, 96, SMALL),     # linear_big: N % 64 fails at M = 2048; colsum: M >= 2048 && N % 4 == 0 -> colsum4, CW = 24 (256 % CW != 0)
    ("fp32", 4095, 36, 20, SMALL),     # linear_backward_impl: M < 4096 -> linear_bwd_small_kernel, last row below the threshold
    ("fp32", 4096, 36, 20, SMALL),     # linear_backward_impl: M >= 4096 -> separate GEMMs; gemm_f32: dW contraction K = 4096 takes split-K
    ("fp32", 4100, 36, 30, SMALL),     # colsum: M >= 2048 && N % 4 != 0 -> colsum_kernel row groups (G = 16) + split_reduce_kernel
    ("fp32", 40000, 8, 6, SMALL),      # colsum: G = min(M / 256, 128) capped at 128; gemm_f32: split-K dW with S = ceil_div(K, 512) slices
    ("fp32", 8, 5000, 40, SMALL),      # gemm_f32: K >= 4096 && tiles < 256 in the FORWARD; bias / ReLU turn split-K off
    ("fp32", 4096, 32, 4100, SMALL),   # gemm_f32: split-K in dx (contraction over N = 4100) and in dW (over M = 4096)
    # ---- LIN_SMALL, bf16 mode: shapes linear_big_padded turns away
    ("bf16", 2048, 24, 64, SMALL),     # linear_big_padded: K >= 32 fails
    ("bf16", 2048, 36, 64, SMALL),     # linear_big_padded: K % 8 == 0 fails
    ("bf16", 2047, 64, 64, SMALL),     # linear_big / linear_big_padded: M >= 2048 fails by one row
    ("bf16", 2048, 64, 28, SMALL),     # linear_big_padded: N >= 32 fails (added: the N side of the minimum)
    # ---- LIN_BIG_F32 / LIN_BIG_BF16: the same shapes in both modes
    ("fp32", 2048, 64, 64, BIG_F32),   # linear_big: the smallest shape it takes
    ("fp32", 2049, 64, 128, BIG_F32),  # linear_big: one row into a ragged last row block
    ("fp32", 2500, 192, 64, BIG_F32),  # linear_big: K of three 64-blocks, ragged rows
    ("fp32", 4120, 128, 320, BIG_F32),   # linear_big: N = 2.5 x 128-column tiles, M >= 4096
    ("bf16", 2048, 64, 64, BIG_BF16),    # linear_path: bf16 && linear_big, the smallest shape
    ("bf16", 2049, 64, 128, BIG_BF16),   # linear_forward_impl: N % 128 == 0 (the residual-epilogue width), ragged rows
    ("bf16", 2500, 192, 64, BIG_BF16),   # linear_path: bf16 && linear_big, N % 128 != 0
    ("bf16", 4120, 128, 320, BIG_BF16),  # linear_path: bf16 && linear_big; colsum4 with cols_pad / 4 = 80 > 32 chunk columns (gy = 3)
    # ---- LIN_PADDED_BF16
    ("bf16", 2048, 32, 32, PADDED),    # linear_big_padded: K >= 32 && N >= 32 at their minimum
    ("bf16", 2048, 64, 72, PADDED),    # linear_big_padded: only N off the 64-multiples
    ("bf16", 2048, 72, 64, PADDED),    # linear_big_padded: only K off the 64-multiples
    ("bf16", 2055, 96, 200, PADDED),   # linear_big_padded: both widths padded (96 -> 128, 200 -> 256), ragged rows
]


def case_id(case):
    mode, M, K, N, route = case
    return f"{mode}-{M}x{K}x{N}-{('small', 'big_f32', 'big_bf16', 'padded')[route]}"


def rb(t):
    """round to bf16-representable fp32"""
    return t.bfloat16().float()


def make_inputs(mode, M, K, N, seed=None):
    """x, w, b, dy on the CPU in fp32; bf16-representable x, w, dy in bf16 mode so that operand rounding is not part of the error"""
    g = torch.Generator().manual_seed(M * 7 + K * 3 + N if seed is None else seed)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    dy = torch.randn(M, N, generator=g)
    if mode == "bf16":
        x, w, dy = rb(x), rb(w), rb(dy)
    return x, w, b, dy


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_grad64(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def reference(x, w, b, dy, act, relu_mask=None):
    """fp64 Linear (+ activation) and its gradients on the CPU.  act: 'none' / 'relu' / 'gelu'.  relu_mask: the mask y > 0 the backward
    under test really used (a sign that differs next to z = 0 is rounding, checked separately by the caller); None: z > 0.
    Returns z (pre-activation), y, dx, dw, db -- dy None: z and y only."""
    x, w = x.double(), w.double()
    z = x @ w.T
    if b is not None:
        z = z + b.double()
    y = z.clamp_min(0) if act == "relu" else gelu64(z) if act == "gelu" else z
    if dy is None:
        return z, y
    g = dy.double()
    if act == "relu":
        g = g * ((z > 0) if relu_mask is None else relu_mask)
    elif act == "gelu":
        g = g * gelu_grad64(z)
    return z, y, g @ w, g.T @ x, g.sum(0)
