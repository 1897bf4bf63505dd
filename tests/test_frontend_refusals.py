"""The front ends' refusals without a GPU: every case of refusal_cases.py that needs no context - the _host twins, and every
context entry point called without a context - answers with the code tests/golden/frontend_refusals.json records
(scripts/make_refusal_golden.py, run before the entry points were given one body per pair)."""
import json
import os

import pytest

import refusal_cases as rc
from unified_cvo_amd import _capi

RECORD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_refusals.json")))
CASES = [c for c in rc.cases() if not c.ctx]


def test_the_record_holds_every_case_and_no_other():
    assert sorted(RECORD["cases"]) == sorted(c.name for c in rc.cases())


@pytest.mark.parametrize("fn", sorted({c.fn for c in CASES}))
def test_refusals_equal_the_record(fn):
    L = _capi.lib()
    mine = [c for c in CASES if c.fn == fn]
    assert mine
    for case in mine:
        assert rc.run(L, None, case) == RECORD["cases"][case.name], case.name
