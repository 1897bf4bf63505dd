"""The five twin pairs that share one body per pair (voxel, RGB-D points, FAST, stereo points, LiDAR): at the smallest shapes
the context entry point with X_HOST=1 returns exactly what the _host twin returns and reports on_device == 0, with X_HOST=0
it reports on_device == 1 and the same output.  A 16 x 24 frame, 64 points, the smallest scan of lidar_cases.py."""
import ctypes as C

import numpy as np
import pytest

import cases
import lidar_cases
from unified_cvo_amd import CvoGPU, LidarRand, RGBDFrame, StereoFrame, _capi
from unified_cvo_amd import fast_select_host, lidar_select_host, rgbd_points_host, stereo_points_host
from unified_cvo_amd.api import CV_FAST, DSO_EDGES, FULL

pytestmark = pytest.mark.gpu

ROWS, COLS = 16, 24
_rng = np.random.default_rng(21)
IMAGE = _rng.integers(0, 256, (ROWS, COLS, 3), dtype=np.uint8)
GRAY = _rng.integers(0, 256, (ROWS, COLS), dtype=np.uint8)
DEPTH = _rng.uniform(0.5, 4.0, (ROWS, COLS)).astype(np.float32)
DEPTH[::5, ::3] = 0.0  # (no depth)
DISPARITY = _rng.uniform(1.0, 20.0, (ROWS, COLS)).astype(np.float32)
DISPARITY[::4, ::7] = -10.0  # (invalid)
XYZ = _rng.uniform(-1.0, 1.0, (64, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    yield g
    g.close()


def _cloud(pc):
    return [pc.pixel, pc.positions(), pc.features(), pc.geometric_types()]


def _voxel_host(xyz, size):
    kept, n = np.zeros(len(xyz), np.int32), C.c_int()
    assert _capi.lib().cvo_voxel_select_host(len(xyz), xyz.ctypes.data_as(C.POINTER(C.c_float)), size, kept.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n)) == 0
    return [kept[:n.value]]


def _voxel(g):
    return [g.voxel_select(XYZ, 0.25)], g.debug_voxel_stats()["capacity"] != 0


def _rgbd(method):
    frame = RGBDFrame(IMAGE, DEPTH, 20.0, 20.0, 12.0, 8.0, 1.0)
    return (lambda: _cloud(rgbd_points_host(frame, method))), (lambda g: (_cloud(g.rgbd_points(frame, method)), g.debug_rgbd_stats()["on_device"]))


def _stereo(method):
    frame = StereoFrame(IMAGE, DISPARITY, 20.0, 20.0, 12.0, 8.0, 0.5)
    return (lambda: _cloud(stereo_points_host(frame, method))), (lambda g: (_cloud(g.stereo_points(frame, method)), g.debug_stereo_stats()["on_device"]))


def _lidar_host():
    scan, cfg = lidar_cases.case("n1")
    rand = LidarRand(1)
    index, is_edge = lidar_select_host(scan, cfg, rand)
    return [index, is_edge, np.array(rand.state()[0])]


def _lidar(g):
    scan, cfg = lidar_cases.case("n1")
    rand = LidarRand(1)
    index, is_edge = g.lidar_select(scan, cfg, rand)
    return [index, is_edge, np.array(rand.state()[0])], g.debug_lidar_stats()["on_device"]


PAIRS = {
    "voxel": ("VOXEL_HOST", lambda: _voxel_host(XYZ, 0.25), _voxel),
    "rgbd full": ("RGBD_HOST",) + _rgbd(FULL),
    "rgbd dso": ("RGBD_HOST",) + _rgbd(DSO_EDGES),
    "fast": ("STEREO_HOST", lambda: list(fast_select_host(GRAY)), lambda g: (list(g.fast_select(GRAY)), g.debug_stereo_stats()["on_device"])),
    "stereo fast": ("STEREO_HOST",) + _stereo(CV_FAST),
    "stereo full": ("STEREO_HOST",) + _stereo(FULL),
    "lidar": ("LIDAR_HOST", _lidar_host, _lidar),
}


@pytest.mark.parametrize("name", list(PAIRS))
def test_context_entry_equals_its_twin_on_either_route(gpu, name):
    switch, twin, entry = PAIRS[name]
    want = twin()
    try:
        for host in (1, 0):
            gpu.set_option(switch, host)
            got, on_device = entry(gpu)
            assert bool(on_device) == (host == 0), (name, host)
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), (name, host)
    finally:
        gpu.set_option(switch, None)
