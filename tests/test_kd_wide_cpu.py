"""The host side of the multi-block ordering (ORDER=wide), without a GPU: the route rule every upload path calls
(cvo_debug_order_route_rule) over its whole table, and the plan the host uploads with a wide job (cvo_debug_wide_plan)
against the statement np_kd.order's own record of its splits and, at sizes up to the cap of 2^24 points, against a
recursion over np_kd.kd_left alone (np_kd.wide_plan); the same plan at other leaf capacities (cvo_debug_wide_plan_at).  Every
comparison is exact."""
import os
import re

import numpy as np
import pytest

import cases
import kd_wide_cases
import np_kd
from unified_cvo_amd import _capi, debug_order_route_rule, debug_wide_plan, debug_wide_plan_at, synth

KD_MAX = 16384
WIDE_MAX = 1 << 24
HOOKS = ("cvo_debug_cloud_order_route", "cvo_debug_order_route_rule", "cvo_debug_wide_plan", "cvo_debug_wide_plan_at",
         "cvo_debug_cloud_wide_pivots")


def _today(n, finite, order, no_sort):
    """The rule before ORDER=wide existed: k_kd_order (1) for 8 .. 16384 finite points of a context whose ORDER is unset or
    reads as `device`, without NO_SORT; the host (0) otherwise."""
    return int(8 <= n <= KD_MAX and finite and not no_sort and order in (None, "device"))


@pytest.mark.parametrize("order", [None, "device", "host", "virtual", "wide"])
def test_route_rule_table(order):
    for n in (0, 7, 8, KD_MAX, KD_MAX + 1, WIDE_MAX, WIDE_MAX + 1):
        for finite in (True, False):
            for no_sort in (False, True):
                got = debug_order_route_rule(n, finite, order, no_sort)
                if order == "wide":
                    ok = finite and not no_sort
                    want = 2 if ok and KD_MAX < n <= WIDE_MAX else (1 if ok and 8 <= n <= KD_MAX else 0)
                else:
                    want = _today(n, finite, order, no_sort)
                assert got == want, (n, finite, order, no_sort, got, want)


def test_unknown_order_text_is_the_device():
    for text in ("", "WIDE", "wide ", "1", "gpu"):
        for n in (8, KD_MAX, KD_MAX + 1):
            assert debug_order_route_rule(n, True, text, False) == _today(n, True, None, False), (text, n)


def _rows_set(rows):
    return sorted(map(tuple, np.asarray(rows).tolist()))


@pytest.mark.parametrize("n", [16385, 16896, 20000, 32768, 32769, 33281, 65536, 65537, 70001, 262145])
def test_plan_equals_the_statements_splits(n):
    W, rows = debug_wide_plan(n)
    assert 1024 <= W <= KD_MAX
    record = []
    np_kd.order(synth.geometric_pair(n, 7)[0], record=record)
    want = [(level, lo, hi, left) for level, axis, lo, hi, left, _ in record if axis is not None and hi - lo > W]
    assert len(rows) == len(want) > 0
    assert _rows_set(rows) == sorted(want)
    # level by level, by position inside a level: the order the kernels' tile tables are built in
    assert rows.tolist() == sorted(rows.tolist(), key=lambda r: (r[0], r[1]))


@pytest.mark.parametrize("n", [1 << 22, WIDE_MAX - 1, WIDE_MAX])
def test_plan_up_to_the_cap(n):
    W, rows = debug_wide_plan(n)
    want = np_kd.wide_plan(n, W)
    assert rows.tolist() == [list(r) for r in want]
    assert all(lo % 512 == 0 and (hi % 512 == 0 or hi == n) and 0 < left < hi - lo for _, lo, hi, left in want)


def test_plan_edges():
    W, rows = debug_wide_plan(KD_MAX + 1)
    assert rows[0].tolist() == [0, 0, KD_MAX + 1, np_kd.kd_left(KD_MAX + 1)]
    for n in (0, 7, W):
        assert len(debug_wide_plan(n)[1]) == 0                      # nothing above a leaf: no cut
    with pytest.raises(Exception):
        debug_wide_plan(WIDE_MAX + 1)
    # two global levels first at the size whose halves no longer both fit a leaf
    levels = lambda n: 1 + int(debug_wide_plan(n)[1][:, 0].max())
    assert levels(2 * W) == 1 and levels(2 * W + 1) == 2


@pytest.mark.parametrize("leaf", [1024, 2048, 16384])
def test_plan_at_a_given_leaf(leaf):
    """The sizes test_gpu_kd_wide_edges.py runs: the crafted clouds', the scatter's, the WIDE_LEAF cases'."""
    for n in (kd_wide_cases.N, kd_wide_cases.SCATTER_N) + kd_wide_cases.LEAF_SIZES:
        rows = debug_wide_plan_at(n, leaf)
        assert rows.tolist() == [list(r) for r in np_kd.wide_plan(n, leaf)], (n, leaf)
        assert len(rows) > 0 and all(hi - lo > leaf for _, lo, hi, _ in rows.tolist())
    assert len(debug_wide_plan_at(leaf, leaf)) == 0 and len(debug_wide_plan_at(leaf + 1, leaf)) == 1


def test_plan_at_the_default_leaf_is_the_default_plan():
    W, rows = debug_wide_plan(70001)
    assert np.array_equal(debug_wide_plan_at(70001, W), rows)
    for leaf in (0, 1023, KD_MAX + 1, -1):
        with pytest.raises(Exception):
            debug_wide_plan_at(70001, leaf)
    with pytest.raises(Exception):
        debug_wide_plan_at(WIDE_MAX + 1, 2048)


def test_header_and_binding_list_hold_the_hooks():
    text = open(os.path.join(cases.ROOT, "include", "cvo_hip_debug.h")).read()
    declared = set(re.findall(r"\b(cvo_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    for sym in HOOKS:
        assert sym in declared and sym in _capi.EXPORTED, sym
        assert hasattr(_capi.lib(), sym), sym
