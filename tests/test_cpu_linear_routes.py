"""The route table of tests/linear_route_cases.py against the library's own answer (mmskin_linear_route reads linear_path, the one
route decision of csrc/linear.hip) -- no GPU needed: the query launches nothing."""
import pytest

from linear_route_cases import BIG_BF16, BIG_F32, PADDED, ROUTE_CASES, SMALL, case_id
from mmskin import _lib


@pytest.fixture
def lib():
    lib = _lib.load()
    prev = lib.mmskin_get_linear_dtype()
    yield lib
    assert lib.mmskin_set_linear_dtype(prev) == 0


@pytest.mark.parametrize("case", ROUTE_CASES, ids=case_id)
def test_route_table(lib, case):
    mode, M, K, N, route = case
    assert lib.mmskin_set_linear_dtype(_lib.BF16 if mode == "bf16" else _lib.F32) == 0
    assert lib.mmskin_linear_route(M, K, N) == route


def test_route_follows_the_mode_and_agrees_with_x16_pitch(lib):
    """the same shape moves between routes with the operand mode only; a kept bf16 operand exists exactly on the two bf16 GEMM routes"""
    for M, K, N, in_f32, in_bf16 in ((2048, 64, 64, BIG_F32, BIG_BF16), (2048, 64, 72, SMALL, PADDED), (2047, 64, 64, SMALL, SMALL)):
        for dtype, want in ((_lib.F32, in_f32), (_lib.BF16, in_bf16)):
            assert lib.mmskin_set_linear_dtype(dtype) == 0
            assert lib.mmskin_linear_route(M, K, N) == want
            pitch = lib.mmskin_linear_x16_pitch(M, K, N)
            assert pitch == {BIG_BF16: K, PADDED: (K + 63) // 64 * 64}.get(want, 0)
    assert lib.mmskin_linear_route(0, 64, 64) == -1 and lib.mmskin_linear_route(64, -1, 64) == -1
