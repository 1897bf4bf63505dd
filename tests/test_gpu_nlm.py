"""Non-local-means denoising on the MI355X: cvo_nlm_denoise / cvo_nlm_denoise_lab with NLM_HOST=0 - the kernel of cvo_k_nlm.h on
every size - against the numpy statement (np_nlm.py).  Every comparison is exact, and every call is checked to have run on the
device.  The kernel's tile is 64 - 2 th columns by 16 rows; the shapes sit on and around its edges."""
import numpy as np
import pytest

import cases
import nlm_cases as nc
import np_nlm
from unified_cvo_amd import CvoGPU, CvoError, _capi, nlm_denoise_host

pytestmark = pytest.mark.gpu

TILE_H = 16


def tile_w(template_window):
    return 64 - 2 * (template_window // 2)


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    g.set_option("NLM_HOST", 0)
    yield g
    g.close()


def _denoise(gpu, img, h=10, windows=(7, 21), in_lds=True):
    out = gpu.nlm_denoise(img, h, *windows)
    st = gpu.debug_nlm_stats()
    k = np_nlm.weights(h, 1 if img.ndim == 2 else img.shape[2], *windows)
    assert st["on_device"] and (st["tile_w"], st["tile_h"]) == (tile_w(windows[0]), TILE_H), st
    assert (st["mult"], st["shift"], st["n_nonzero"]) == (k["mult"], k["shift"], k["n_nonzero"]) and st["table_in_lds"] == in_lds, st
    return out


def _edges(W, H):
    return [(r, c) for r in (1, H - 1, H, H + 1, 2 * H + 1) for c in (1, W - 1, W, W + 1, 2 * W + 1)]


REFLECT = [(r, c) for r in (13, 14, 27) for c in (13, 14, 27)]  # b = 13: the border reflects once up to 14 pixels, twice below


@pytest.mark.parametrize("rows,cols", _edges(tile_w(7), TILE_H) + REFLECT)
def test_one_channel_on_and_around_the_tile(gpu, rows, cols):
    img = nc.image("steps", rows, cols)
    assert np.array_equal(_denoise(gpu, img), nc.statement("steps", rows, cols))


@pytest.mark.parametrize("channels", (2, 3))
def test_more_channels(gpu, channels):
    W = tile_w(7)
    for rows, cols in ((1, 1), (TILE_H - 1, W + 1), (TILE_H + 1, W - 1), (TILE_H, W), (2 * TILE_H + 1, 2 * W + 1), (13, 14), (14, 13), (27, 27)):
        for kind in ("steps", "random"):
            img = nc.image(kind, rows, cols, channels)
            assert np.array_equal(_denoise(gpu, img), nc.statement(kind, rows, cols, channels)), (kind, rows, cols)


def test_lab(gpu):
    W = tile_w(7)
    for rows, cols, h, hc in ((1, 1, 10, 10), (TILE_H + 1, W + 1, 10, 10), (2 * TILE_H + 1, W - 1, 10, 7), (13, 14, 3, 20), (27, 2 * W + 1, 10, 10)):
        lab = nc.image("steps", rows, cols, 3)
        got = gpu.nlm_denoise_lab(lab, h, hc)
        st = gpu.debug_nlm_stats()
        assert st["on_device"] and st["table_in_lds"] and st["n_nonzero"] == np_nlm.weights(hc, 2)["n_nonzero"], st
        assert np.array_equal(got, nc.statement_lab("steps", rows, cols, h, hc)), (rows, cols)
    work = lab.copy()
    assert gpu.nlm_denoise_lab(work, out=work) is work and np.array_equal(work, got)  # in place


@pytest.mark.parametrize("windows", ((3, 5), (1, 1), (5, 11), (6, 20)))
def test_other_windows(gpu, windows):
    """(6, 20): even sizes grow by one, to (7, 21).  (8, 20) grows to a 9 x 9 template, th = 4: test_refusals."""
    W = tile_w(windows[0])
    for rows, cols in ((1, W), (TILE_H + 1, W + 1), (13, 14), (2 * TILE_H + 1, W - 1)):
        for channels in (1, 3):
            img = nc.image("steps", rows, cols, channels)
            assert np.array_equal(_denoise(gpu, img, 10, windows), nc.statement("steps", rows, cols, channels, 10, windows)), (rows, cols, channels)
    if windows == (6, 20):
        assert np.array_equal(nc.statement("steps", 13, 14, 1, 10, windows), nc.statement("steps", 13, 14))


@pytest.mark.parametrize("channels,h,in_lds", ((1, 3, True), (1, 20, True), (3, 3, True), (3, 20, True), (1, 39, True), (1, 40, False), (3, 25, False),
                                               (2, 10.5, True)))
def test_h_and_the_table_bound(gpu, channels, h, in_lds):
    """The table's nonzero run is held in LDS up to 8192 entries (one channel: h = 39 has 8020, h = 40 has 8437); beyond, the
    kernel reads the rest from global memory."""
    assert (np_nlm.weights(h, channels)["n_nonzero"] <= 8192) == in_lds
    for rows, cols in ((TILE_H + 1, tile_w(7) + 1), (14, 27)):
        for kind in ("steps", "random"):
            img = nc.image(kind, rows, cols, channels)
            assert np.array_equal(_denoise(gpu, img, h, in_lds=in_lds), nc.statement(kind, rows, cols, channels, h)), (kind, rows, cols)


def test_the_special_planes(gpu):
    for kind in ("white", "checker", "constant"):
        for channels in (1, 3):
            img = nc.image(kind, TILE_H + 7, tile_w(7) + 9, channels)
            got = _denoise(gpu, img)
            assert np.array_equal(got, nc.statement(kind, TILE_H + 7, tile_w(7) + 9, channels)) and np.array_equal(got, img), (kind, channels)


def test_a_strip_at_kitti_width(gpu):
    """120 x 1241, one channel (the statement takes under a second at this size)."""
    img = nc.image("steps", 120, 1241)
    want = nc.statement("steps", 120, 1241)
    assert (want != img).mean() > 0.5
    assert np.array_equal(_denoise(gpu, img), want)


def test_a_tall_image(gpu):
    """16 x 65536 + 1 rows of one pixel: more rows of tiles than a grid's second axis holds.  Windows (3, 3): nine offsets."""
    rows = 16 * 65536 + 1
    img = nc.image("steps", rows, 1)
    want = nc.statement("steps", rows, 1, 1, 10, (3, 3))
    assert (want != img).mean() > 0.5
    assert np.array_equal(_denoise(gpu, img, 10, (3, 3)), want)


def test_repeats_routes_and_in_place(gpu):
    img = nc.image("steps", 40, 70, 3)
    first = _denoise(gpu, img)
    assert np.array_equal(first, nc.statement("steps", 40, 70, 3)) and np.array_equal(first, nlm_denoise_host(img))
    for _ in range(9):
        assert np.array_equal(gpu.nlm_denoise(img), first)
    work = img.copy()
    assert gpu.nlm_denoise(work, out=work) is work and np.array_equal(work, first)
    try:
        gpu.set_option("NLM_HOST", 1)
        assert np.array_equal(gpu.nlm_denoise(img), first) and not gpu.debug_nlm_stats()["on_device"]
        gpu.set_option("NLM_HOST", None)
        gpu.nlm_denoise(nc.image("steps", 3, 5))
        assert not gpu.debug_nlm_stats()["on_device"]  # under 256 pixels the default route is the twin
        gpu.nlm_denoise(img)
        assert gpu.debug_nlm_stats()["on_device"]
    finally:
        gpu.set_option("NLM_HOST", 0)


def test_refusals_then_a_good_call(gpu):
    """Each refusal names its call and code, writes nothing and leaves the context usable."""
    img = nc.image("steps", 20, 33)
    want = nc.statement("steps", 20, 33)
    for what, rows, cols, ch, h, tw, sw, hc, code in nc.refusals():
        if what == "pixels" or what.startswith(("rows", "cols", "channels")):
            continue  # (shapes an array cannot take: by return code in test_nlm_cpu.py)
        out = np.full((5, 5, 3), 77, np.uint8)
        with pytest.raises(CvoError, match=f"error {getattr(_capi, 'CVO_E_' + code)}: cvo_nlm_denoise"):
            if what.startswith("h_color"):
                gpu.nlm_denoise_lab(np.zeros((5, 5, 3), np.uint8), h, hc, tw, sw, out=out)
            else:
                gpu.nlm_denoise(np.zeros((5, 5, 3), np.uint8), h, tw, sw, out=out)
        assert np.all(out == 77), what
        assert np.array_equal(gpu.nlm_denoise(img), want), what
    with pytest.raises(CvoError, match=f"error {_capi.CVO_E_UNSUPPORTED}: cvo_nlm_denoise_lab"):
        gpu.nlm_denoise_lab(np.zeros((5, 5, 3), np.uint8), 10, 10, 8, 20)
    assert np.array_equal(gpu.nlm_denoise(img), want) and gpu.debug_nlm_stats()["on_device"]
