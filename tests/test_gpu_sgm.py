"""The stereo matcher on the MI355X: cvo_stereo_disparity with SGM_HOST=0 - the kernels of cvo_k_sgm.h on every size - against
the numpy statement (np_sgm.py).  Every comparison is exact, and every call is checked through debug_sgm_stats to have run on
the device.  On a mismatch the census planes and S of that call are read back once and the first differing stage is named.
The census kernel's tile and the lanes over d (d = lane + 64 j) set the shapes: the smallest at which each mechanism can go
wrong."""
import numpy as np
import pytest

import cases
import np_sgm
import sgm_cases as sc
from unified_cvo_amd import CvoGPU, CvoError, SGMConfig, StereoFrame, _capi, stereo_disparity_host
from unified_cvo_amd.api import CV_FAST, FULL

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 8


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    g.set_option("SGM_HOST", 0)
    yield g
    g.close()


def _lines(rows, cols, paths):
    return ([rows, rows, cols, cols] + [rows + cols - 1] * 4)[:paths] + [0] * (8 - paths)


def _on_device(gpu, rows, cols, config):
    st = gpu.debug_sgm_stats()
    cfg = {**np_sgm.DEFAULTS, **config}
    assert st["on_device"] and (st["tile_w"], st["tile_h"]) == (TILE_W, TILE_H), st
    assert (st["rows"], st["cols"], st["max_disparity"], st["paths"]) == (rows, cols, cfg["max_disparity"], cfg["paths"]), st
    assert st["lines"] == _lines(rows, cols, cfg["paths"]), st


def _compare(gpu, got, want, what):
    """want: the statement's stages.  On a mismatch: one read-back, the first stage that differs.  got None: the map itself was
    not returned (upload_stereo_pair) and what followed from it differed."""
    if got is not None and np.array_equal(got, want["disparity"]):
        return
    back = gpu.debug_sgm_readback()
    for stage in ("census_left", "census_right", "S"):
        bad = np.argwhere(back[stage] != want[stage])
        if len(bad):
            i = tuple(bad[0])
            pytest.fail(f"{what}: first differing stage {stage}: {len(bad)} entries, first at {i}: {back[stage][i]} for {want[stage][i]}")
    if got is None:
        pytest.fail(f"{what}: census and S equal the statement; the selection or what follows it differs")
    bad = np.argwhere(got != want["disparity"])
    i = tuple(bad[0])
    pytest.fail(f"{what}: census and S equal the statement, the selection differs at {len(bad)} pixels, first at {i}: {got[i]} for {want['disparity'][i]}")


def _check(gpu, kind, rows, cols, seed=0, d0=0, **config):
    left, right = sc.planes(kind, rows, cols, seed, d0)
    got = gpu.stereo_disparity(left, right, SGMConfig(**config))
    _on_device(gpu, rows, cols, config)
    _compare(gpu, got, sc.statement(kind, rows, cols, seed, d0, **config), (kind, rows, cols, d0, config))
    return got


@pytest.mark.parametrize("rows,cols,D,d0,seed", sc.SHIFT_CASES)
def test_the_lane_seams_of_d(gpu, rows, cols, D, d0, seed):
    """The shift cases of test_sgm_cpu.py: d0 = 63 and 64 at D = 128 and 129 at D = 256 put the winner and its neighbours on
    either side of a lane seam (d = 63 | 64: lane 63 of j = 0 | lane 0 of j = 1)."""
    for paths in (4, 8):
        got = _check(gpu, "shift", rows, cols, seed, d0, max_disparity=D, paths=paths)
        assert np.all(np.floor(got[:, d0 + 4:cols - 4][got[:, d0 + 4:cols - 4] >= 0] + 0.5) == d0)


@pytest.mark.parametrize("rows,cols", ((1, 1), (1, 70), (70, 1), (7, 63), (70, 9), (9, 70), (3, 5)))
def test_the_path_lines(gpu, rows, cols):
    """rows = 1 and cols = 1: every diagonal has length 1; (7, 63) at D = 128: cols < D; tall and wide: rows + cols - 1
    diagonals either way.  (_on_device checks the lines launched per direction.)"""
    for paths in (4, 8):
        for kind, d0 in (("noise", 0), ("shift", 3)):
            _check(gpu, kind, rows, cols, 0, d0, max_disparity=128, paths=paths)
    _check(gpu, "noise", rows, cols, 1, max_disparity=64)
    _check(gpu, "noise", rows, cols, 1, max_disparity=256)


@pytest.mark.parametrize("rows", (TILE_H - 1, TILE_H, TILE_H + 1, 2 * TILE_H + 1))
@pytest.mark.parametrize("cols", (TILE_W - 1, TILE_W, TILE_W + 1, 2 * TILE_W + 1))
def test_on_and_around_the_census_tile(gpu, rows, cols):
    _check(gpu, "noise", rows, cols, max_disparity=64)


def test_the_byte_bound(gpu):
    """p2 = 193 on noise: L up to 255, S up to 2040."""
    for paths in (4, 8):
        for p1 in (10, 193):
            _check(gpu, "noise", 24, 100, max_disparity=64, p1=p1, p2=193, paths=paths)
    _check(gpu, "noise", 9, 130, max_disparity=128, p1=0, p2=193)


@pytest.mark.parametrize("uniqueness", (0, 99))
@pytest.mark.parametrize("lr_max_diff", (-1, 0, 1))
def test_the_selection_switches(gpu, uniqueness, lr_max_diff):
    for kind, rows, cols, d0 in (("noise", 9, 130, 0), ("shift", 24, 100, 17), ("constant_right", 7, 63, 0)):
        _check(gpu, kind, rows, cols, 0, d0, max_disparity=64, uniqueness=uniqueness, lr_max_diff=lr_max_diff)


def test_ties_take_the_first_disparity(gpu):
    """A constant right plane: all costs of a pixel tie over u - d >= 0; the first argmin is 0 on every lane layout."""
    for D in (64, 128, 256):
        got = _check(gpu, "constant_right", 7, 63, max_disparity=D, uniqueness=0, lr_max_diff=-1)
        assert np.all(got == 0)


def test_twin_equals_device_on_two_planes(gpu):
    """96 x 320, default configuration (the statement takes about a second at this size; nothing larger goes through numpy)."""
    left, right, truth = sc.two_planes(96, 320)
    got = _check(gpu, "two_planes", 96, 320)
    assert np.array_equal(got, stereo_disparity_host(left, right))
    region = np.s_[52:, 34:-4]
    assert (np.floor(got[region] + 0.5) == truth[region]).mean() > 0.98
    for _ in range(3):
        assert np.array_equal(gpu.stereo_disparity(left, right), got)  # (the region is reused: no state leaks between calls)


def test_upload_stereo_pair_equals_upload_stereo_with_the_statements_map(gpu):
    rows, cols, d0 = 160, 200, 20
    left, right = sc.shift(rows, cols, d0, 7)
    want_map = sc.statement("shift", rows, cols, 7, d0)["disparity"]
    calib = dict(fx=707.09, fy=707.09, cx=100.0, cy=80.0, baseline=0.54)
    third = gpu.upload_stereo(StereoFrame(left, np.full((rows, cols), 20.25, np.float32), **calib), FULL)  # a fixed cloud near both
    eye = np.eye(4, dtype=np.float32)
    try:
        for method in (CV_FAST, FULL):
            a = gpu.upload_stereo_pair(StereoFrame(left, None, **calib), right, method=method)
            _on_device(gpu, rows, cols, {})
            b = gpu.upload_stereo(StereoFrame(left, want_map, **calib), method)
            if a.n != b.n or not np.array_equal(a.pixel, b.pixel):
                _compare(gpu, None, sc.statement("shift", rows, cols, 7, d0), ("upload_stereo_pair", method))
            assert a.n > 100, method
            ip_a, ip_b = gpu.inner_product_gpu(a, third, eye, 0.5), gpu.inner_product_gpu(b, third, eye, 0.5)
            assert np.float32(ip_a).tobytes() == np.float32(ip_b).tobytes() and ip_a > 0, (ip_a, ip_b)
            a.free()
            b.free()
        # a BGR frame: the left plane is the front end's own gray of the image; a gray plane given with the frame wins
        bgr = np.repeat(left[..., None], 3, 2)
        a = gpu.upload_stereo_pair(StereoFrame(bgr, None, **calib), right, method=FULL)
        b = gpu.upload_stereo(StereoFrame(bgr, want_map, **calib), FULL)
        assert a.n == b.n and np.array_equal(a.pixel, b.pixel)  # (gray of (x, x, x) is x: the same map)
        a.free()
        b.free()
        other = sc.noise(rows, cols, 3)[0]
        a = gpu.upload_stereo_pair(StereoFrame(other, None, gray=left, **calib), right, method=FULL)
        assert np.array_equal(a.pixel, gpu.upload_stereo(StereoFrame(other, want_map, gray=left, **calib), FULL).pixel)
        a.free()
    finally:
        third.free()


def test_routes_and_the_default(gpu):
    left, right = sc.noise(9, 70)
    want = sc.statement("noise", 9, 70)["disparity"]
    try:
        gpu.set_option("SGM_HOST", 1)
        assert np.array_equal(gpu.stereo_disparity(left, right), want) and not gpu.debug_sgm_stats()["on_device"]
        with pytest.raises(CvoError, match="cvo_debug_sgm_readback"):
            gpu.debug_sgm_readback()
        gpu.set_option("SGM_HOST", None)
        gpu.stereo_disparity(*sc.noise(3, 5))
        assert not gpu.debug_sgm_stats()["on_device"]  # small frames take the twin by default
        gpu.stereo_disparity(*sc.noise(96, 320))
        assert gpu.debug_sgm_stats()["on_device"]
    finally:
        gpu.set_option("SGM_HOST", 0)


def test_refusals_then_a_good_call(gpu):
    """Each refusal names its call and code and leaves the context usable."""
    left, right = sc.noise(5, 5)
    for what, rows, cols, over, code in sc.refusals():
        if what in ("rows", "cols"):
            continue  # (shapes an array cannot take: by return code in test_sgm_cpu.py)
        with pytest.raises(CvoError, match=f"error {getattr(_capi, 'CVO_E_' + code)}: cvo_stereo_disparity"):
            if rows * cols > 1 << 20:
                _refuse_large(gpu, rows, cols, over)
            else:
                gpu.stereo_disparity(np.zeros((rows, cols), np.uint8), np.zeros((rows, cols), np.uint8), SGMConfig(**over))
    with pytest.raises(CvoError, match=f"error {_capi.CVO_E_INVALID}: cvo_cloud_upload_stereo_pair"):
        gpu.upload_stereo_pair(StereoFrame(left, None, 700.0, 700.0, 2.0, 2.0, 0.5), right, SGMConfig(paths=5))
    with pytest.raises(CvoError, match=f"error {_capi.CVO_E_INVALID}: cvo_cloud_upload_stereo_pair"):
        gpu.upload_stereo_pair(StereoFrame(left, None, 0.0, 700.0, 2.0, 2.0, 0.5), right)  # the front end's refusal: fx = 0
    _check(gpu, "noise", 9, 70)


def _refuse_large(gpu, rows, cols, over):
    """A frame too large to allocate for a refusal: the call through ctypes with a small buffer, which a refusal never reads."""
    import ctypes as C
    buf, out = np.zeros(16, np.uint8), np.zeros(16, np.float32)
    cfg = SGMConfig(**over).c_struct()
    bp = C.POINTER(C.c_ubyte)
    gpu._check(gpu.L.cvo_stereo_disparity(gpu.ctx, rows, cols, buf.ctypes.data_as(bp), buf.ctypes.data_as(bp), C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float))))
