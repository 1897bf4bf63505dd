"""The five twin pairs that share one body per pair (voxel, RGB-D points, FAST, stereo points, LiDAR): at the smallest shapes
the context entry point with X_HOST=1 returns exactly what the _host twin returns and reports on_device == 0, with X_HOST=0
it reports on_device == 1 and the same output.  A 16 x 24 frame, 64 points, the smallest scan of lidar_cases.py.

Every front end lays its device buffers out anew, per call, in a region that grows: in one fresh context on the device route,
small -> at least four times larger -> small again equals the twin each time (the region is reallocated by the second call,
and the third binds its buffers into the larger region)."""
import ctypes as C

import numpy as np
import pytest

import bki_cases
import cases
import dfilter_cases
import lidar_cases
from unified_cvo_amd import CvoGPU, DFilterConfig, LidarRand, MapConfig, RGBDFrame, StereoFrame, _capi
from unified_cvo_amd import disparity_filter_host, fast_select_host, lidar_select_host, map_open_host, nlm_denoise_host, rgbd_points_host
from unified_cvo_amd import stereo_disparity_host, stereo_points_host
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


# ---- the growable regions: small, at least four times larger, small again ----
HOST_SWITCHES = ("VOXEL_HOST", "RGBD_HOST", "STEREO_HOST", "LIDAR_HOST", "NLM_HOST", "SGM_HOST", "DFILTER_HOST", "BKI_HOST")
_big = np.random.default_rng(22)
BIG = dict(image=_big.integers(0, 256, (2 * ROWS, 2 * COLS, 3), dtype=np.uint8), gray=_big.integers(0, 256, (2 * ROWS, 2 * COLS), dtype=np.uint8),
           right=_big.integers(0, 256, (2 * ROWS, 2 * COLS), dtype=np.uint8), depth=_big.uniform(0.5, 4.0, (2 * ROWS, 2 * COLS)).astype(np.float32),
           xyz=_big.uniform(-1.0, 1.0, (256, 3)).astype(np.float32),
           map=dfilter_cases.blobs(2 * ROWS, 2 * COLS, 2), scan="room16", hits="hits255")
BIG["depth"][::5, ::3] = 0.0
# (the stereo constructor keeps rows 100 .. h - 30 alone: the larger stereo frame is tall enough to keep some points)
BIG.update(stereo_image=_big.integers(0, 256, (136, COLS, 3), dtype=np.uint8), disparity=_big.uniform(1.0, 20.0, (136, COLS)).astype(np.float32))
BIG["disparity"][::4, ::7] = -10.0
SMALL = dict(image=IMAGE, stereo_image=IMAGE, gray=GRAY, right=_rng.integers(0, 256, (ROWS, COLS), dtype=np.uint8), depth=DEPTH, disparity=DISPARITY, xyz=XYZ,
             map=dfilter_cases.blobs(ROWS, COLS, 1), scan="n1", hits="hits1")
DFILTER = (1.0, 20, 3, 1)  # (dfilter_cases' "blobs": every pass acts)


def _lidar_of(select, name):
    scan, cfg = lidar_cases.case(name)
    rand = LidarRand(1)
    index, is_edge = select(scan, cfg, rand)
    return [index, is_edge, np.array(rand.state()[0])]


def _voxel_size(g, s):
    return [g.voxel_select(s["xyz"], 0.25)], g.debug_voxel_stats()["capacity"] != 0


def _points(kind, method):
    def frame(s):
        return RGBDFrame(s["image"], s["depth"], 20.0, 20.0, 12.0, 8.0, 1.0) if kind == "rgbd" else StereoFrame(s["stereo_image"], s["disparity"], 20.0, 20.0, 12.0, 8.0, 0.5)
    twin = rgbd_points_host if kind == "rgbd" else stereo_points_host
    def entry(g, s):
        if kind == "rgbd":
            return _cloud(g.rgbd_points(frame(s), method)), g.debug_rgbd_stats()["on_device"]
        return _cloud(g.stereo_points(frame(s), method)), g.debug_stereo_stats()["on_device"]
    return (lambda s: _cloud(twin(frame(s), method))), entry


def _map_rows(m, s):
    """a map after one more frame: the table read back, the cloud, the sizes"""
    cfg, frames = bki_cases.all_cases()[s["hits"]]
    assert cfg.kwargs() == bki_cases.all_cases()["hits1"][0].kwargs()  # (one map takes all three frames)
    xyz, feat, label, origin = frames[0]
    m.insert((xyz, feat, label), origin=origin)
    stats = m.debug_stats(readback=True)
    return [stats["keys"]] + [bki_cases.bits(a) for a in (stats["ms"], stats["fs"]) + tuple(m.cloud())] + [np.array(m.size())], stats["on_device"]


# name -> (twin(shapes), entry(context, shapes) -> (result, on_device)); the maps take (map, shapes)
GROWN = {
    "voxel": (lambda s: _voxel_host(s["xyz"], 0.25), _voxel_size),
    "rgbd full": _points("rgbd", FULL),
    "rgbd dso": _points("rgbd", DSO_EDGES),
    "fast": (lambda s: list(fast_select_host(s["gray"])), lambda g, s: (list(g.fast_select(s["gray"])), g.debug_stereo_stats()["on_device"])),
    "stereo fast": _points("stereo", CV_FAST),
    "stereo full": _points("stereo", FULL),
    "lidar": (lambda s: _lidar_of(lidar_select_host, s["scan"]), lambda g, s: (_lidar_of(g.lidar_select, s["scan"]), g.debug_lidar_stats()["on_device"])),
    "nlm": (lambda s: [nlm_denoise_host(s["gray"])], lambda g, s: ([g.nlm_denoise(s["gray"])], g.debug_nlm_stats()["on_device"])),
    "sgm": (lambda s: [stereo_disparity_host(s["gray"], s["right"])], lambda g, s: ([g.stereo_disparity(s["gray"], s["right"])], g.debug_sgm_stats()["on_device"])),
    "dfilter": (lambda s: [disparity_filter_host(s["map"], DFilterConfig(*DFILTER))],
                lambda g, s: ([g.disparity_filter(s["map"], DFilterConfig(*DFILTER))], g.debug_dfilter_stats()["on_device"])),
    "map": None,
}


@pytest.fixture(scope="module")
def device_gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))  # one fresh context, every front end on the device
    for switch in HOST_SWITCHES:
        g.set_option(switch, 0)
    yield g
    g.close()


@pytest.mark.parametrize("name", list(GROWN))
def test_regions_regrown_and_reused_still_equal_the_twin(device_gpu, name):
    if name == "map":
        config = MapConfig(**bki_cases.all_cases()["hits1"][0].kwargs())
        host, dev = map_open_host(config), device_gpu.map_open(config)
        twin, entry = (lambda s: _map_rows(host, s)[0]), (lambda g, s: _map_rows(dev, s))
    else:
        twin, entry = GROWN[name]
    try:
        for step, shapes in enumerate((SMALL, BIG, SMALL)):
            want = twin(shapes)
            got, on_device = entry(device_gpu, shapes)
            assert on_device, (name, step)
            assert len(got) == len(want)
            for a, b in zip(got, want):
                if name == "dfilter":  # (bit patterns, as test_gpu_dfilter.py compares; the map's rows are bits already)
                    assert not dfilter_cases.first_difference(a, b), (name, step)
                assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), (name, step)
    finally:
        if name == "map":
            host.close()
            dev.close()
