"""The disparity post-filter on the MI355X: cvo_disparity_filter with DFILTER_HOST=0 - the kernels of cvo_k_dfilter.h on every
size - against the numpy statement (np_dfilter.py).  Every comparison is exact (bit patterns), and every call is checked
through debug_dfilter_stats to have run on the device.  On a mismatch the maps the device kept after each stage are read back
once and the first differing stage is named.  The cases (dfilter_cases.py) are the smallest at which each mechanism can go
wrong: the kernels' 64 x 4 tile, a wave's 64 pixels of one row, the 64-pixel steps of the gap scan, the mean's 4 + 3 halo."""
import ctypes as C

import numpy as np
import pytest

import cases
import dfilter_cases as dc
import np_dfilter
import sgm_cases as sc
from unified_cvo_amd import CvoGPU, CvoError, DFilterConfig, SGMConfig, StereoFrame, _capi, disparity_filter_host
from unified_cvo_amd.api import CV_FAST, FULL

pytestmark = pytest.mark.gpu

CASES = dc.cases()


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))  # one context across sizes and routes
    g.set_option("DFILTER_HOST", 0)
    g.set_option("SGM_HOST", 0)
    yield g
    g.close()


def _config(cfg):
    return DFilterConfig(cfg.speckle_sim_threshold, cfg.speckle_size, cfg.ipol_gap_width, cfg.adaptive_mean)


def _on_device(gpu, shape, want=None):
    st = gpu.debug_dfilter_stats()
    assert st["on_device"] and (st["tile_w"], st["tile_h"]) == (dc.TILE_W, dc.TILE_H), st
    assert (st["rows"], st["cols"]) == tuple(shape), st
    if want is not None:
        assert (st["segments"], st["removed"], st["filled"]) == want["counts"], (st, want["counts"])


def _compare(gpu, got, want, cfg, what):
    """want: the statement's stages.  On a mismatch: one read-back, the first stage that differs."""
    if not dc.first_difference(got, want["out"]):
        return
    back = gpu.debug_dfilter_stats(readback=True)
    stages = (("after_speckle", "speckle", cfg.speckle_size > 1), ("after_gap", "gap", cfg.ipol_gap_width >= 1), ("mean_tmp", "mean_tmp", cfg.adaptive_mean))
    for mine, theirs, ran in stages:
        if ran and back[mine] is not None:
            bad = dc.first_difference(back[mine], want[theirs])
            if bad:
                pytest.fail(f"{what}: first differing stage {theirs}: {bad}")
    pytest.fail(f"{what}: every stage read back equals the statement; the last pass differs: {dc.first_difference(got, want['out'])}")


def _check(gpu, name):
    d, cfg = CASES[name]
    want = dc.statement(name)
    got = gpu.disparity_filter(d, _config(cfg))
    _on_device(gpu, d.shape, want)
    _compare(gpu, got, want, cfg, name)
    return got


@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("mean ")])
def test_kernels_equal_the_statement(gpu, name):
    _check(gpu, name)


def test_the_tile_the_cases_were_made_for(gpu):
    _check(gpu, "1x1")  # (_on_device compares the stats' tile with dfilter_cases.TILE_W x TILE_H)
    d, cfg = dc.speckle_straddle()
    xs = np.argwhere(d >= 0)[:, 1]
    assert xs.min() < dc.TILE_W <= xs.max() and (np.argwhere(d >= 0)[:, 0].max() > 2 * dc.TILE_H)


def test_the_means_window_on_small_and_tile_sized_maps(gpu):
    """7 .. 16 wide and high: the first sizes at which the horizontal (H >= 7, W >= 8) and the vertical pass (W >= 7, H >= 8)
    write anything, and all coordinates mod 8; one and two tiles plus 1."""
    touched = 0
    for name in CASES:
        if name.startswith("mean "):
            got = _check(gpu, name)
            touched += int((got != CASES[name][0]).sum())
    assert touched > 500


def test_speckle_size_on_either_side_of_a_segment(gpu):
    d, cfg = CASES["speckle straddle"]
    got = _check(gpu, "speckle straddle")
    sizes = sorted(int((d == v).sum()) for v in (5.0, 6.0, 7.0))
    assert sizes == [cfg.speckle_size - 1, cfg.speckle_size, cfg.speckle_size + 1]
    assert (got == 5.0).sum() == 0 and (got == 6.0).sum() == cfg.speckle_size and (got == 7.0).sum() == cfg.speckle_size + 1


def test_repeats_and_out_is_in(gpu):
    """The region is reused and its counters cleared: no state leaks between calls of different sizes; out may be the input."""
    first = {n: _check(gpu, n) for n in ("blobs", "golden", "serpentine removed", "blobs")}
    for name in ("golden", "blobs"):
        d = CASES[name][0].copy()
        assert gpu.disparity_filter(d, _config(CASES[name][1]), out=d) is d
        _on_device(gpu, d.shape, dc.statement(name))
        assert not dc.first_difference(d, first[name])


def test_twin_equals_device(gpu):
    for name in ("golden", "blobs", "blobs sim 0"):
        d, cfg = CASES[name]
        assert not dc.first_difference(gpu.disparity_filter(d, _config(cfg)), disparity_filter_host(d, _config(cfg)))


SGM = dict(max_disparity=64)


def _pair():
    left, right, _ = sc.two_planes(64, 200, 3)
    return left, right


@pytest.mark.parametrize("dcfg", (np_dfilter.Config(), np_dfilter.Config(1.0, 30, 2, 0), np_dfilter.Config(1.0, 0, 0, 0)))
def test_filtered_matcher_equals_the_statement_of_the_statement(gpu, dcfg):
    left, right = _pair()
    raw = sc.statement("two_planes", 64, 200, 3, **SGM)["disparity"]
    want = np_dfilter.stages(raw, dcfg)
    got = gpu.stereo_disparity(left, right, SGMConfig(**SGM), dfilter=_config(dcfg))
    assert gpu.debug_sgm_stats()["on_device"]
    _on_device(gpu, raw.shape, want)
    _compare(gpu, got, want, dcfg, ("stereo_disparity filtered", vars(dcfg)))
    # ... and the unfiltered call followed by the filter
    assert not dc.first_difference(gpu.disparity_filter(gpu.stereo_disparity(left, right, SGMConfig(**SGM)), _config(dcfg)), got)


def test_filtered_matcher_on_mixed_routes(gpu):
    """matcher on the host and filter on the device, and the reverse: the same map"""
    left, right = _pair()
    dcfg = DFilterConfig(1.0, 30, 3, 1)
    want = gpu.stereo_disparity(left, right, SGMConfig(**SGM), dfilter=dcfg)
    try:
        gpu.set_option("SGM_HOST", 1)
        assert not dc.first_difference(gpu.stereo_disparity(left, right, SGMConfig(**SGM), dfilter=dcfg), want)
        assert not gpu.debug_sgm_stats()["on_device"] and gpu.debug_dfilter_stats()["on_device"]
        gpu.set_option("SGM_HOST", 0)
        gpu.set_option("DFILTER_HOST", 1)
        assert not dc.first_difference(gpu.stereo_disparity(left, right, SGMConfig(**SGM), dfilter=dcfg), want)
        assert gpu.debug_sgm_stats()["on_device"] and not gpu.debug_dfilter_stats()["on_device"]
    finally:
        gpu.set_option("SGM_HOST", 0)
        gpu.set_option("DFILTER_HOST", 0)


def test_upload_stereo_pair_filtered_equals_upload_stereo_of_the_filtered_map(gpu):
    left, right, _ = sc.two_planes(160, 200, 3)  # (the size test_gpu_sgm.py uploads: FAST finds corners on it)
    rows, cols = left.shape
    dcfg = DFilterConfig(1.0, 30, 3, 1)
    filtered = gpu.disparity_filter(gpu.stereo_disparity(left, right, SGMConfig(**SGM)), dcfg)
    calib = dict(fx=707.09, fy=707.09, cx=100.0, cy=80.0, baseline=0.54)
    for method in (CV_FAST, FULL):
        a = gpu.upload_stereo_pair(StereoFrame(left, None, **calib), right, SGMConfig(**SGM), method=method, dfilter=dcfg)
        _on_device(gpu, (rows, cols))
        b = gpu.upload_stereo(StereoFrame(left, filtered, **calib), method)
        plain = gpu.upload_stereo_pair(StereoFrame(left, None, **calib), right, SGMConfig(**SGM), method=method)
        assert a.n == b.n and np.array_equal(a.pixel, b.pixel) and a.n > 100, method
        if method == FULL:
            assert plain.n != a.n  # (the filter removed and filled pixels)
        for c in (a, b, plain):
            c.free()


def test_routes_and_the_default(gpu):
    d, cfg = CASES["blobs"]
    want = dc.statement("blobs")
    try:
        gpu.set_option("DFILTER_HOST", 1)
        assert not dc.first_difference(gpu.disparity_filter(d, _config(cfg)), want["out"])
        st = gpu.debug_dfilter_stats()
        assert not st["on_device"] and (st["tile_w"], st["tile_h"]) == (0, 0) and (st["segments"], st["removed"], st["filled"]) == want["counts"]
        with pytest.raises(CvoError, match="cvo_debug_dfilter_stats"):
            buf = np.zeros(d.shape, np.float32)
            gpu._check(gpu.L.cvo_debug_dfilter_stats(gpu.ctx, None, None, None, None, None, None, buf.ctypes.data_as(C.POINTER(C.c_float)), None, None))
        gpu.set_option("DFILTER_HOST", None)
        gpu.disparity_filter(CASES["mean 9x9"][0])
        assert not gpu.debug_dfilter_stats()["on_device"]  # small maps take the twin by default
        gpu.disparity_filter(CASES["constant 256"][0])
        assert gpu.debug_dfilter_stats()["on_device"]
    finally:
        gpu.set_option("DFILTER_HOST", 0)


def test_refusals_then_a_good_call(gpu):
    """Each refusal names its call and code, writes nothing and leaves the context usable."""
    for what, d, cfg, code in dc.refusals():
        out = np.full(d.shape, 77, np.float32)
        with pytest.raises(CvoError, match=f"error {getattr(_capi, 'CVO_E_' + code)}: cvo_disparity_filter"):
            gpu.disparity_filter(d, _config(cfg), out=out)
        assert np.all(out == 77), what
    left, right = sc.noise(5, 5)
    with pytest.raises(CvoError, match=f"error {_capi.CVO_E_INVALID}: cvo_stereo_disparity_filtered"):
        gpu.stereo_disparity(left, right, dfilter=DFilterConfig(10.0))  # the matcher's -10 is not below -sim
    with pytest.raises(CvoError, match=f"error {_capi.CVO_E_INVALID}: cvo_stereo_disparity_filtered"):
        gpu.stereo_disparity(left, right, SGMConfig(paths=5), dfilter=DFilterConfig())
    with pytest.raises(CvoError, match=f"error {_capi.CVO_E_INVALID}: cvo_cloud_upload_stereo_pair_filtered"):
        gpu.upload_stereo_pair(StereoFrame(left, None, 700.0, 700.0, 2.0, 2.0, 0.5), right, dfilter=DFilterConfig(1.0, -1))
    _check(gpu, "blobs")
