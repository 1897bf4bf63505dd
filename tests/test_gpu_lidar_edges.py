"""The LiDAR kernels on the MI355X at the places where their own structure changes (lidar_cases.EDGE_CASES; DESIGN.md section 3,
"structural classes"): every sort size of k_lidar_pick, the four words of a component's row mask, ring starts on block, wave
and lane boundaries of k_lidar_project, shapes that make k_lidar_union merge many trees late, empty and tiny results of the
device route, the validator's limits, and one context's scratch across calls of very different sizes.  LIDAR_HOST=0 unless a
test says otherwise; every comparison is exact, against the numpy statement (np_lidar.py).
tests/test_lidar_cpu.py::test_the_edge_cases_reach_their_edges holds, on the CPU, that each case reaches its edge."""
import numpy as np
import pytest

import cases
import lidar_cases as lc
import np_lidar
from unified_cvo_amd import CvoGPU, CvoPointCloud, LidarRand

pytestmark = pytest.mark.gpu

HOST_BELOW = 12000  # scans with fewer points take the CPU twin unless LIDAR_HOST says otherwise
EMPTY = ("n1", "n3")  # the cases that select nothing


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    g.set_option("LIDAR_HOST", 0)
    yield g
    g.close()


def _select_equals_the_statement(gpu, name, on_device=True):
    """lidar_select of a case: indices, is_edge, the nine counts and the generator are the statement's -> (index, is_edge)."""
    scan, cfg = lc.case(name)
    want = lc.statement(name)
    rand, after = LidarRand(1), LidarRand(1)
    index, is_edge = gpu.lidar_select(scan, cfg, rand)
    st = gpu.debug_lidar_stats()
    assert st["on_device"] == on_device, (name, st)
    assert index.dtype == want["index"].dtype and np.array_equal(index, want["index"]) and np.array_equal(is_edge, want["is_edge"]), name
    assert {k: st[k] for k in lc.COUNTS} == {k: want[k] for k in lc.COUNTS}, (name, st)
    for _ in range(want["draws"]):
        after.next()
    assert rand.state() == after.state(), name
    return index, is_edge


def _cloud_of(scan, index):
    r = np_lidar.rows(scan.xyzi, index, scan.semantic, scan.num_classes)
    return CvoPointCloud.from_arrays(r["xyz"], r["feat"], r.get("label"), r["geotype"])


@pytest.mark.parametrize("name", lc.EDGE_CASES)
def test_kernels_equal_the_statement_at_the_edges(gpu, name):
    """Select: indices, is_edge, all nine counts (valid / invalid pin the union-find's components, draws / thinned the two
    thinning compactions) and the generator.  Upload, where something is selected: `.pixel` is the statement's index and the
    resident cloud orders as an ordinary upload of the statement's rows does."""
    scan, cfg = lc.case(name)
    want = lc.statement(name)
    _select_equals_the_statement(gpu, name)
    if name in EMPTY:
        return  # (test_an_empty_selection_is_an_empty_cloud_on_both_routes)
    assert len(want["index"]) > 0
    rand, after = LidarRand(1), LidarRand(1)
    d = gpu.upload_lidar(scan, cfg, rand)
    try:
        assert gpu.debug_lidar_stats()["on_device"] and np.array_equal(d.pixel, want["index"]), name
        for _ in range(want["draws"]):
            after.next()
        assert rand.state() == after.state(), name
        lc.same_resident(gpu, d, _cloud_of(scan, want["index"]))
    finally:
        d.free()


def test_an_empty_selection_is_an_empty_cloud_on_both_routes(gpu):
    """A scan of which nothing is selected (one point, three points): upload_lidar returns what an ordinary upload of an empty
    cloud returns, a resident cloud of no points - no refusal - with an empty `.pixel`, on the kernels and on the twin alike;
    no draw is made, the counts are the statement's, and the context goes on giving right answers."""
    empty = CvoPointCloud.from_arrays(np.zeros((0, 3), np.float32), np.zeros((0, 1), np.float32), None, np.zeros((0, 2), np.float32))
    try:
        for name in EMPTY:
            scan, cfg = lc.case(name)
            want = lc.statement(name)
            assert len(want["index"]) == 0 and want["draws"] == 0
            seen = {}
            for route in (0, 1):
                gpu.set_option("LIDAR_HOST", route)
                rand = LidarRand(7)
                d = gpu.upload_lidar(scan, cfg, rand)
                try:
                    st = gpu.debug_lidar_stats()
                    assert st["on_device"] == (route == 0) and {k: st[k] for k in lc.COUNTS} == {k: want[k] for k in lc.COUNTS}, (name, route, st)
                    assert d.handle and d.n == 0 and d.pixel.shape == (0,) and d.debug_order().shape == (0,), (name, route)
                    assert rand.state() == LidarRand(7).state(), (name, route)
                    lc.same_resident(gpu, d, empty)
                    seen[route] = (d.n, d.pixel.tobytes(), d.debug_order().tobytes(), tuple(st[k] for k in lc.COUNTS))
                finally:
                    d.free()
                index, is_edge = gpu.lidar_select(scan, cfg, rand)
                assert len(index) == 0 and len(is_edge) == 0 and rand.state() == LidarRand(7).state(), (name, route)
            assert seen[0] == seen[1], name
            gpu.set_option("LIDAR_HOST", 0)
            _select_equals_the_statement(gpu, "room16")  # a good call afterwards
    finally:
        gpu.set_option("LIDAR_HOST", 0)


def test_one_context_many_sizes(gpu):
    """The scratch of one context, laid out per call from the image's cells and the scan's points, across calls of very
    different sizes: each equals its statement, and the second run of the first case equals the first bit for bit."""
    g = CvoGPU(params=cases.load_params("geometric_gpu"))  # a context of its own: what came before is part of the test
    try:
        g.set_option("LIDAR_HOST", 0)
        got = [(name, _select_equals_the_statement(g, name)) for name in ("wide4096", "n1", "tall128", "room16", "max", "blob30_alone", "wide4096")]
        (_, first), (_, last) = got[0], got[-1]
        assert first[0].tobytes() == last[0].tobytes() and first[1].tobytes() == last[1].tobytes()
    finally:
        g.close()


def test_routes_agree_at_the_edges(gpu):
    """LIDAR_HOST = 0, 1 and unset: the same indices, is_edge, `.pixel`, resident order and generator state."""
    try:
        for name in ("wide4096", "tall128", "serpent", "all_near"):
            scan, cfg = lc.case(name)
            res = {}
            for route in (0, 1, None):
                gpu.set_option("LIDAR_HOST", route)
                rand = LidarRand(7)
                index, is_edge = gpu.lidar_select(scan, cfg, rand)
                assert gpu.debug_lidar_stats()["on_device"] == (route == 0 or (route is None and scan.n >= HOST_BELOW)), (name, route)
                d = gpu.upload_lidar(scan, cfg, rand)  # the second frame of a chain
                res[route] = [index, is_edge, d.pixel, d.debug_order(), np.array(rand.state()[0])]
                d.free()
            for route in (1, None):
                for a, b in zip(res[0], res[route]):
                    assert a.dtype == b.dtype and np.array_equal(a, b), (name, route)
    finally:
        gpu.set_option("LIDAR_HOST", 0)


def test_repeats_are_identical_where_arrival_order_could_leak(gpu):
    """Ten repeats of the union's late merges (comb, loop) and of the two-trip sort (wide4096): indices, is_edge and counts."""
    for name in ("comb", "loop", "wide4096"):
        scan, cfg = lc.case(name)
        first = _select_equals_the_statement(gpu, name)
        stats = gpu.debug_lidar_stats()
        for _ in range(10):
            again = gpu.lidar_select(scan, cfg, LidarRand(1))
            assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes() and gpu.debug_lidar_stats() == stats, name
