"""The RGB-D selector's kernels (k_rgbd_gray_grad, k_rgbd_hist, k_rgbd_smooth, k_rgbd_select of cvo_k_rgbd.h) on the MI355X at
their block, cell and threshold edges: every case of rgbd_cases.EDGE_CASES with RGBD_HOST=0 against the numpy statement
(np_rgbd.py), stage by stage through debug_rgbd_readback - g2, the block thresholds, the smoothed thresholds with their zero
slack, and the selections of ALL six potentials, those the schedule never tries included.  Every comparison is exact; a
failure names the first differing stage and its first differing index.  test_rgbd_cpu.py asserts that each case reaches the
edge it is named after."""
import numpy as np
import pytest

import cases
import np_rgbd
import rgbd_cases as rc
from unified_cvo_amd import CvoGPU, CvoError, StereoFrame
from unified_cvo_amd.api import DSO_EDGES, FULL

pytestmark = pytest.mark.gpu

ORDER = rc.edge_order()


def _context():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    g.set_option("RGBD_HOST", 0)
    return g


@pytest.fixture(scope="module")
def gpu():
    g = _context()
    yield g
    g.close()


def _compare(gpu, name, what):
    """One read-back of the context's last selection against the statement's stages of case `name`."""
    back = gpu.debug_rgbd_readback()
    f = rc.edge_frame(name)
    assert back["g2"].shape == (f.rows, f.cols) and len(back["ths"]) == len(back["sm"]) == (f.cols // 32) * (f.rows // 32) + 100, what
    diff = rc.first_difference(back, rc.edge_statement(name))
    if diff:
        pytest.fail(f"{what}: {diff}")
    nb = (f.cols // 32) * (f.rows // 32)
    assert not back["ths"][nb:].any() and not back["sm"][nb:].any(), what  # the slack
    return back


def _check_selection(gpu, name):
    """DSO_EDGES of a case: the points, the route and the schedule, then every stage."""
    f, want = rc.edge_frame(name), rc.edge_statement(name)["points"][DSO_EDGES]
    pc = gpu.rgbd_points(f, DSO_EDGES)
    st = gpu.debug_rgbd_stats()
    tried, counts = want["schedule"]
    assert st["on_device"] and st["potentials"] == tried and st["counts"] == counts, (name, st, tried, counts)
    back = _compare(gpu, name, name)
    assert [len(back["selected"][p]) for p in tried] == counts
    rc.assert_points_equal(pc, want, (name, DSO_EDGES), name in rc.NAN_COORDINATES)
    assert st["edge_selected"] == counts[-1] and st["edge_points"] == len(want["pixel"]), (name, st)


def test_the_order_alternates_large_and_small_frames():
    assert sorted(ORDER) == sorted(rc.EDGE_CASES)
    assert ORDER[ORDER.index("shape_36x3205") + 1] == "shape_33x33"
    size = [rc.edge_frame(n).rows * rc.edge_frame(n).cols for n in ORDER]
    assert all(size[i] > size[i + 1] for i in range(0, len(size) - 1, 2))


@pytest.mark.parametrize("name", ORDER)
def test_kernels_equal_the_statement_stage_by_stage(gpu, name):
    _check_selection(gpu, name)
    f, want = rc.edge_frame(name), rc.edge_statement(name)["points"][FULL]
    rc.assert_points_equal(gpu.rgbd_points(f, FULL), want, (name, FULL), name in rc.NAN_COORDINATES)
    st = gpu.debug_rgbd_stats()
    assert st["on_device"] and st["surface_points"] == len(want["pixel"]) and st["with_depth"] == want["with_depth"], (name, st)


def test_one_context_across_the_cases_leaks_no_state():
    """A fresh context runs every case once, large and small frames in turn (36 x 3205 immediately before 33 x 33): the
    scratch region is reused and the thresholds are zeroed again, so every stage equals the statement whatever ran before."""
    g = _context()
    try:
        for name in ORDER:
            _check_selection(g, name)
        for name in reversed(ORDER[:6]):
            _check_selection(g, name)
    finally:
        g.close()


def test_the_widest_accepted_image_and_the_first_refused_one(gpu):
    _check_selection(gpu, "shape_36x3205")
    f = rc.refused_frame()
    with pytest.raises(CvoError, match="error -5.*threshold index.*200 of 200"):
        gpu.rgbd_points(f, DSO_EDGES)
    _compare(gpu, "shape_36x3205", "after a refused call the last selection still stands")
    rc.assert_points_equal(gpu.rgbd_points(f, FULL), rc.statement_points(f, FULL), "refused shape, FULL")
    assert gpu.debug_rgbd_stats()["on_device"]


def test_the_read_back_is_refused_without_a_selection_on_the_device():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    try:
        def refused():
            with pytest.raises(CvoError, match="error -2: cvo_debug_rgbd_readback"):  # CVO_E_INVALID
                g.debug_rgbd_readback()

        refused()  # no call yet
        name = "shape_64x95"
        f = rc.edge_frame(name)
        for route, method in ((1, DSO_EDGES), (0, FULL), (1, FULL)):
            g.set_option("RGBD_HOST", 0)
            g.rgbd_points(f, DSO_EDGES)
            _compare(g, name, "a good call")
            g.set_option("RGBD_HOST", route)
            g.rgbd_points(f, method)
            assert g.debug_rgbd_stats()["on_device"] == (route == 0)
            refused()  # the host route; a FULL-only call on either route
        g.set_option("RGBD_HOST", 0)
        g.upload_rgbd(f, 0.1).free()  # the recipe selects on the device, then back-projects both sets
        _compare(g, name, "the recipe")
    finally:
        g.close()


def test_the_stereo_route_shares_the_selector(gpu):
    """stereo_points(DSO_EDGES) runs rgbd_device_select on the frame's gray plane: the same six selections."""
    name = "shape_65x64"
    f = rc.edge_frame(name)
    gpu.rgbd_points(f, DSO_EDGES)
    first = _compare(gpu, name, "the RGB-D call")
    disparity = np.full((f.rows, f.cols), 20.0, np.float32)
    s = StereoFrame(f.image, disparity, 700.0, 700.0, f.cols / 2.0, f.rows / 2.0, 0.54)
    gpu.set_option("STEREO_HOST", 0)
    try:
        gpu.stereo_points(s, DSO_EDGES)
        st = gpu.debug_stereo_stats()
        tried, counts = rc.edge_statement(name)["points"][DSO_EDGES]["schedule"]
        assert st["on_device"] and st["tried"] == tried and st["counts"] == counts, st
        second = _compare(gpu, name, "the stereo call")
        for p in rc.POTS:
            assert np.array_equal(first["selected"][p], second["selected"][p]), p
        gpu.stereo_points(s, FULL)  # lays the region out again without a selection
        with pytest.raises(CvoError, match="cvo_debug_rgbd_readback"):
            gpu.debug_rgbd_readback()
    finally:
        gpu.set_option("STEREO_HOST", None)
