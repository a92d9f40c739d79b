"""The route table of tests/attention_route_cases.py against mmskin.attention.attention_route, the one attention route decision -- no GPU
and no library needed: the function takes plain values and launches nothing."""
import pytest

from attention_route_cases import BLOCK, FLASH, FLASH_TRAIN, LONG, ROUTE_CASES, ROWS, case_id
from mmskin.attention import attention_route


@pytest.mark.parametrize("case", ROUTE_CASES, ids=case_id)
def test_route_table(case):
    cid, args, extras, gpu, expect = case
    assert attention_route(**args) == expect


def test_every_family_and_both_ways_of_reading_are_in_the_table():
    seen = {c[4] for c in ROUTE_CASES}
    assert {f for f, _ in seen} == {FLASH, FLASH_TRAIN, ROWS, BLOCK, LONG}
    for family in (FLASH, FLASH_TRAIN, ROWS, BLOCK, LONG):
        assert (family, False) in seen, family                     # each family is reachable through the permuted copies
    assert {(FLASH, True), (ROWS, True)} <= {e for c in ROUTE_CASES if c[1]["layout"] != "bhld" for e in [c[4]]}


def test_the_names_ops_keeps():
    """ops.py re-exports the attention entry points, and the dropout counter stays the one list object (tests rewind ops._dropout_counter[0])"""
    from mmskin import _autograd, attention, ops
    for name in ("attention", "attention_blhd", "attention_packed", "attention_route", "window_attention", "window_attention_ok",
                 "channel_attention", "channel_attention_ok", "LongAttentionFn", "_bmm"):
        assert getattr(ops, name) is getattr(attention, name), name
    assert ops._dropout_counter is _autograd._dropout_counter and ops._dropout_state is _autograd._dropout_state
    assert attention._dropout_state is _autograd._dropout_state
