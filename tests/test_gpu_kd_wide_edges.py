"""The multi-block ordering (ORDER=wide, cvo_k_kd_wide.h) at the edges of its select, its scatter and its leaves, on the MI355X.

test_gpu_kd_wide.py's three opinions (the route is the device's, a permutation, the leaf sets of np_kd.order, the same on a
second call) on clouds that put each mechanism where it can go wrong - kd_wide_cases.py, held to their claims without a GPU
by test_kd_wide_cases_cpu.py:
  - the select: a pivot whose digits are 00 / FF in every pass (threads 0 and 255 of the block scan), keys that differ in
    their low byte only, a pivot among negative keys, the first / all of 4000 equal keys;
  - the scatter: a root segment of 293 tiles, whose tiles 257 .. 292 add up their predecessors' counts in two trips;
  - the leaves: WIDE_LEAF = 2048 and 16384 - a leaf exactly at the capacity of a block of 16384, leaves in either buffer.
And a second look that says WHERE an ordering went wrong: a context with WIDE_RECORD=1 keeps the select's (pivot, rem) of
every planned cut (cvo_debug_cloud_wide_pivots), which _locate holds against the statement's own segments - the first
(level, segment) whose pivot or rem differs, else the first cut whose left SET differs, else the first leaf.  Every
comparison is exact: integers, leaf sets, key bit patterns.

Can these tests fail?  Each of three one-line changes of the kernels was built and run once on the MI355X against the 70
tests of this module and of test_gpu_kd_wide.py that only upload and read back (left out: its three tests that score or
solve on wide-ordered clouds - test_attribute_gathers, test_from_the_device, test_one_solve - which would read attributes
through an inverse permutation with holes).  Every change leaves the stores behind `at < len` and the ids behind their
clamps - k_kd_wide_leaves clamps what it writes to `order` for this reason - and no loop depends on data.
  1. kd_wide_select: `rem <= incl` -> `rem < incl` (a rank that is the last of its digit is found by nobody).
     58 of 70 fail.  Here: all 8 test_crafted_cases, test_the_device_selects_the_crafted_pivot[digits-ff, all-of-equals,
     top-byte-00] (the root's select itself: pivot 0 rem 0 for 0xc0ffffff rem 5), test_the_scatters_second_trip, all 16
     test_other_leaf_capacities, the upload_many test, test_pivots_are_kept_only_where_asked_for.  test_gpu_kd_wide.py alone
     notices too: every size class and most degenerate clouds fail (some pass of some level has its rank on a digit's end).
     _locate names it, e.g. "the select of level 1, segment [0, 10240) cut at 5120 (number 1 of the plan), axis 0: pivot
     0xc0efefef rem 317, the statement has 0xc0effd60 rem 1".
  2. k_kd_wide_scatter: the prefix loop reads its first trip only (`q += KD_WIDE_THREADS` -> `break`).
     1 of 70 fails: test_the_scatters_second_trip.  test_gpu_kd_wide.py alone does NOT notice (no segment above 256 tiles).
  3. k_kd_wide_scatter: `eq < rem` -> `eq <= rem` in goes_left (one equal key too many goes left).
     18 of 70 fail.  Here: test_crafted_cases[low-byte-only, negative-side, first-of-equals, all-of-equals] (the cases with
     more equals than go left, or with equals on a later cut), test_the_scatters_second_trip ("every pivot agrees; the scatter
     of level 1, segment [300032, 600001) cut at 150016 (number 2 of the plan)": equal float32 keys among 300 000 points), the
     signed-zeros test_other_leaf_capacities at both leaves.  test_gpu_kd_wide.py alone notices through lattice, the signed
     zeros and the duplicate rows; its generic clouds pass."""
import numpy as np
import pytest

import kd_wide_cases as kc
import np_kd
from test_gpu_kd_wide import BLOCK, HOST, WIDE, _context, _order_and_route, _three_opinions
from unified_cvo_amd import CvoError, CvoPointCloud, debug_wide_plan_at, synth

pytestmark = pytest.mark.gpu

DEFAULT_LEAF = 1024


@pytest.fixture(scope="module")
def contexts():
    """(ORDER=wide, its host twin ORDER=virtual, ORDER=wide with WIDE_RECORD=1)"""
    gs = _context("wide"), _context("virtual"), _context("wide", WIDE_RECORD=1)
    yield gs
    for g in gs:
        g.close()


@pytest.fixture(scope="module", params=kc.LEAVES)
def leaf_context(request):
    g = _context("wide", WIDE_LEAF=request.param, WIDE_RECORD=1)
    yield request.param, g
    g.close()


def _locate(g, x, leaf):
    """None, or where the ordering of x by the recording context g (leaves of `leaf`) first leaves the statement."""
    n = x.shape[0]
    c = g.upload(CvoPointCloud.from_xyz(x))
    try:
        assert c.debug_order_route() == WIDE
        order, (pivot, rem) = c.debug_order(), c.debug_wide_pivots()
    finally:
        c.free()
    record = []
    want = np_kd.order(x, record=record)
    cuts = [r for r in record if r[1] is not None and r[3] - r[2] > leaf]
    plan = np_kd.wide_plan(n, leaf)
    assert [(level, lo, hi, left) for level, _, lo, hi, left, _ in cuts] == plan == [tuple(r) for r in debug_wide_plan_at(n, leaf).tolist()]
    assert len(pivot) == len(rem) == len(plan)
    for k, (level, axis, lo, hi, left, members) in enumerate(cuts):
        keys = np.sort(np_kd.ordered_key(x[members, axis]))
        p = int(keys[left - 1])
        r = left - int((keys < p).sum())
        if (int(pivot[k]), int(rem[k])) != (p, r):
            return (f"the select of level {level}, segment [{lo}, {hi}) cut at {left} (number {k} of the plan), axis {axis}: pivot "
                    f"{int(pivot[k]):#010x} rem {int(rem[k])}, the statement has {p:#010x} rem {r}")
    for k, (level, axis, lo, hi, left, _) in enumerate(cuts):
        if not np.array_equal(np.sort(order[lo:lo + left]), np.sort(want[lo:lo + left])):
            missing = left - len(np.intersect1d(order[lo:lo + left], want[lo:lo + left]))
            return (f"every pivot agrees; the scatter of level {level}, segment [{lo}, {hi}) cut at {left} (number {k} of the plan): "
                    f"{missing} of the statement's left points are not on its left")
    differ = np.flatnonzero((np_kd.leaf_sets(order) != np_kd.leaf_sets(want)).any(axis=1))
    if len(differ):
        at = 4 * int(differ[0])
        level, lo, m, NP = next(l for l in np_kd.wide_plan_leaves(n, leaf) if l[1] <= at < l[1] + l[2])
        return (f"every pivot and every cut agrees; the leaf block [{lo}, {lo + m}) of level {level} (NP {NP}): position {at} "
                f"is the first of {len(differ)} runs of four that differ")
    return None


def _hold(g, x, leaf, name):
    where = _locate(g, x, leaf)
    assert where is None, f"{name}: {where}"


@pytest.mark.parametrize("name", list(kc.CRAFTED))
def test_crafted_cases(contexts, name):
    x = kc.crafted(name)
    _hold(contexts[2], x, DEFAULT_LEAF, name)  # (first: a failure then says where)
    _three_opinions(contexts, x, name)


@pytest.mark.parametrize("name", list(kc.CRAFTED))
def test_the_device_selects_the_crafted_pivot(contexts, name):
    """The case reaches the device as crafted: the root segment's select IS (P, rem)."""
    P, _, _, rem, _ = kc.CRAFTED[name]
    c = contexts[2].upload(CvoPointCloud.from_xyz(kc.crafted(name)))
    try:
        pivot, rems = c.debug_wide_pivots()
    finally:
        c.free()
    assert (int(pivot[0]), int(rems[0])) == (P, rem), (name, hex(int(pivot[0])), int(rems[0]))


def test_the_scatters_second_trip(contexts):
    """600001 points: the root segment has 293 tiles, so tiles 257 .. 292 read the counts of more than 256 earlier tiles."""
    n = kc.SCATTER_N
    level, lo, hi, _ = np_kd.wide_plan(n, DEFAULT_LEAF)[0]
    assert (level, lo, hi) == (0, 0, n) and -(-(hi - lo) // kc.TILE) > 257
    x = kc.slab(n)
    _hold(contexts[2], x, DEFAULT_LEAF, n)
    _three_opinions(contexts, x, n)


@pytest.mark.parametrize("n", kc.LEAF_SIZES)
@pytest.mark.parametrize("kind", list(kc.LEAF_KINDS))
def test_other_leaf_capacities(contexts, leaf_context, kind, n):
    leaf, g = leaf_context
    assert (leaf, n) in kc.leaf_plan_properties()
    x = kc.LEAF_KINDS[kind](n)
    _hold(g, x, leaf, (leaf, kind, n))
    _three_opinions((g, contexts[1]), x, (leaf, kind, n))


def test_two_wide_clouds_in_one_call_at_the_largest_leaf():
    """upload_many under WIDE_LEAF=16384: two plans, tables and leaf scratch (seg_stride 8194) in one region, the per-point
    buffers shared; each cloud is what its single upload is, and keeps its own pivots."""
    g = _context("wide", WIDE_LEAF=16384, WIDE_RECORD=1)
    try:
        xs = [kc.slab(32769, 21), kc.slab(20000, 22)]
        pcs = [CvoPointCloud.from_xyz(x) for x in xs]
        single = []
        for pc in pcs:
            c = g.upload(pc)
            try:
                single.append((c.debug_order(), c.debug_order_route(), c.debug_wide_pivots()))
            finally:
                c.free()
        many = g.upload_many(pcs, threads=2)
        try:
            for x, m, (order, route, (pivot, rem)) in zip(xs, many, single):
                assert m.debug_order_route() == route == WIDE
                assert np.array_equal(m.debug_order(), order), len(x)
                p, r = m.debug_wide_pivots()
                assert np.array_equal(p, pivot) and np.array_equal(r, rem) and len(p) == len(np_kd.wide_plan(len(x), 16384))
                assert np.array_equal(np_kd.leaf_sets(order), np_kd.leaf_sets(np_kd.order(x))), len(x)
        finally:
            for m in many:
                m.free()
    finally:
        g.close()


def test_pivots_are_kept_only_where_asked_for(contexts):
    """WIDE_RECORD unset: no record; set: only for clouds the multi-block ordering itself ordered."""
    w, _, rec = contexts
    x = synth.geometric_pair(20000, 7)[0]
    for g, xx, route in ((w, x, WIDE), (rec, x[:16384], BLOCK), (rec, x[:7], HOST)):
        c = g.upload(CvoPointCloud.from_xyz(xx))
        try:
            assert c.debug_order_route() == route
            with pytest.raises(CvoError):
                c.debug_wide_pivots()
        finally:
            c.free()
    # ... and the record changes nothing: the same order with and without it
    pc = CvoPointCloud.from_xyz(x)
    assert np.array_equal(_order_and_route(w, pc)[0], _order_and_route(rec, pc)[0])


@pytest.mark.parametrize("value", [np.inf, -np.inf])
def test_an_infinity_goes_to_the_host(contexts, value):
    w = contexts[0]
    for column in range(3):
        bad = synth.geometric_pair(20000, 7)[0].copy()
        bad[11717, column] = value
        order, route = _order_and_route(w, CvoPointCloud.from_xyz(bad))
        assert route == HOST and np.array_equal(order, np.arange(20000)), (value, column)
