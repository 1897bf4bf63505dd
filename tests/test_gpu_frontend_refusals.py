"""The front ends' refusals with a context: code and cvo_last_error text of every case of refusal_cases.py, exactly as
tests/golden/frontend_refusals.json records them (scripts/make_refusal_golden.py, run before the entry points were given one
body per pair and the stereo pair one locked chain), the two-fault cases that pin which refusal wins among them.  Nothing is
launched: every case is refused before device work.  Then the one call that succeeds: a refused call leaves the matcher's, the
filter's and the stereo front end's stats as that call left them."""
import ctypes as C
import json
import os

import pytest

import refusal_cases as rc
from unified_cvo_amd import _capi

pytestmark = pytest.mark.gpu

RECORD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_refusals.json")))
CASES = [c for c in rc.cases() if c.ctx]


@pytest.fixture(scope="module")
def ctx():
    L = _capi.lib()
    h = C.c_void_p()
    assert L.cvo_ctx_create(0, C.byref(h)) == 0
    yield h
    L.cvo_ctx_destroy(h)


@pytest.mark.parametrize("fn", sorted({c.fn for c in CASES}))
def test_refusals_equal_the_record(ctx, fn):
    L = _capi.lib()
    mine = [c for c in CASES if c.fn == fn]
    assert mine
    for case in mine:
        assert rc.run(L, ctx, case) == RECORD["cases"][case.name], case.name


def test_a_refused_call_leaves_the_stats_of_the_last_success(ctx):
    got = rc.survival(_capi.lib(), ctx)
    assert got["after_success"] == RECORD["stats"]["after_success"]
    assert got["after_refusals"] == RECORD["stats"]["after_refusals"] == got["after_success"]
