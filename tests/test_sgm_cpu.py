"""The stereo matcher without a GPU: the CPU twin (cvo_stereo_disparity_host) equal to the statement (np_sgm.py) over shapes,
disparity ranges, path counts and every switch of the configuration; every refusal by its return code, nothing written; and
the statement's own properties on frames with a known disparity, asserted on the statement so that they hold before any GPU
run."""
import ctypes as C

import numpy as np
import pytest

import np_sgm
import sgm_cases as sc
from unified_cvo_amd import CvoError, SGMConfig, _capi, stereo_disparity_host

SHAPES = ((1, 1), (1, 70), (3, 5), (7, 63), (9, 130), (24, 100))


def _twin(kind, rows, cols, seed=0, d0=0, **config):
    return stereo_disparity_host(*sc.planes(kind, rows, cols, seed, d0), SGMConfig(**config))


def test_the_census_of_a_small_plane_by_hand():
    """3 x 3, centre pixel: the 62 neighbours clamp onto the nine pixels; bit = neighbour < centre, first neighbour first."""
    img = np.array([[5, 1, 9], [7, 4, 2], [0, 8, 3]], np.uint8)
    word = 0
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if (dy, dx) != (0, 0):
                word = (word << 1) | int(img[min(max(1 + dy, 0), 2), min(max(1 + dx, 0), 2)] < img[1, 1])
    assert int(np_sgm.census(img)[1, 1]) == word and word < 1 << 62
    assert np.all(np_sgm.census(np.full((4, 6), 7, np.uint8)) == 0)


@pytest.mark.parametrize("rows,cols", SHAPES)
@pytest.mark.parametrize("D", (64, 128, 256))
def test_twin_equals_the_statement(rows, cols, D):
    for paths in (4, 8):
        for kind, d0 in (("noise", 0), ("shift", 3)):
            want = sc.statement(kind, rows, cols, 0, d0, max_disparity=D, paths=paths)["disparity"]
            got = _twin(kind, rows, cols, 0, d0, max_disparity=D, paths=paths)
            assert got.dtype == np.float32 and np.array_equal(got, want), (kind, paths)


def test_twin_where_the_bytes_reach_their_bound():
    """p2 = 193 on noise: L may reach 62 + 193 = 255 and S 2040 (the statement asserts both bounds); with p1 = p2 = 193 the
    statement's L does come within 55 of the byte's end."""
    left, right = sc.noise(24, 100)
    cost = np_sgm.cost_volume(np_sgm.census(left), np_sgm.census(right), 64)
    assert max(np_sgm.path(cost, dv, du, 193, 193).max() for dv, du in np_sgm.DIRECTIONS) > 200
    for paths in (4, 8):
        for p1 in (10, 193):
            cfg = dict(max_disparity=64, p1=p1, p2=193, paths=paths)
            assert np.array_equal(_twin("noise", 24, 100, **cfg), sc.statement("noise", 24, 100, **cfg)["disparity"]), cfg
    cfg = dict(max_disparity=128, p1=0, p2=193)
    assert np.array_equal(_twin("noise", 9, 130, **cfg), sc.statement("noise", 9, 130, **cfg)["disparity"])


@pytest.mark.parametrize("uniqueness", (0, 99))
@pytest.mark.parametrize("lr_max_diff", (-1, 0, 1))
def test_twin_on_the_selection_switches(uniqueness, lr_max_diff):
    for kind, rows, cols, d0 in (("noise", 9, 130, 0), ("shift", 24, 100, 17), ("constant_right", 7, 63, 0)):
        cfg = dict(max_disparity=64, uniqueness=uniqueness, lr_max_diff=lr_max_diff)
        want = sc.statement(kind, rows, cols, 0, d0, **cfg)
        assert np.array_equal(_twin(kind, rows, cols, 0, d0, **cfg), want["disparity"]), kind
    # the switches decide something: noise is all invalid at 99 %, and without either test every pixel is valid
    if uniqueness == 99:
        assert not sc.statement("noise", 9, 130, max_disparity=64, uniqueness=99, lr_max_diff=lr_max_diff)["valid"].any()
    if uniqueness == 0 and lr_max_diff < 0:
        assert sc.statement("noise", 9, 130, max_disparity=64, uniqueness=0, lr_max_diff=-1)["valid"].all()


def test_ties_take_the_first_disparity():
    """A constant right plane: every cost of a pixel ties over u - d >= 0, and the first argmin is d = 0."""
    st = sc.statement("constant_right", 7, 63, max_disparity=64, uniqueness=0, lr_max_diff=-1)
    assert np.all(st["d"] == 0) and np.all(st["disparity"] == 0)


@pytest.mark.parametrize("paths", (4, 8))
def test_the_statement_finds_a_known_shift(paths):
    """left[:, d0:] = right[:, :cols - d0]: over d0 + 4 <= u < cols - 4 every valid pixel has d* = d0 and |disp - d0| < 0.5,
    and at most 1 % of the region is invalid (a cap, not a measurement: the statement leaves 0 - 2 pixels of 1800 - 4480)."""
    for rows, cols, D, d0, seed in sc.SHIFT_CASES:
        st = sc.statement("shift", rows, cols, seed, d0, max_disparity=D, paths=paths)
        region = np.s_[:, d0 + 4:cols - 4]
        valid, d, disp = st["valid"][region], st["d"][region], st["disparity"][region]
        assert np.all(d[valid] == d0) and np.all(np.abs(disp[valid] - d0) < 0.5), (rows, cols, D, d0)
        assert (~valid).sum() <= 0.01 * valid.size, ((~valid).sum(), valid.size)
        assert np.all(st["disparity"][~st["valid"]] == np_sgm.INVALID)


def test_the_statement_finds_two_planes():
    """32 x 200, D = 64: rows above the middle shifted by 10, below by 30; u >= 34, rows within 3 of the boundary excluded."""
    rows, cols = 32, 200
    truth = sc.two_planes(rows, cols)[2]
    st = sc.statement("two_planes", rows, cols, max_disparity=64)
    keep = np.abs(np.arange(rows) - rows // 2 + 0.5) > 3
    valid, d, disp, want = (a[keep][:, 34:] for a in (st["valid"], st["d"], st["disparity"], truth))
    assert np.all(d[valid] == want[valid]) and np.all(np.abs(disp[valid] - want[valid]) < 0.5)
    assert (~valid).sum() <= 0.01 * valid.size, ((~valid).sum(), valid.size)


def test_refusals_write_nothing():
    L = _capi.lib()
    bp, fp = C.POINTER(C.c_ubyte), C.POINTER(C.c_float)
    img = np.full(25, 9, np.uint8)
    call = L.cvo_stereo_disparity_host
    for what, rows, cols, over, code in sc.refusals():
        cfg = SGMConfig(**over).c_struct()
        out = np.full(25, 77, np.float32)
        assert call(rows, cols, img.ctypes.data_as(bp), img.ctypes.data_as(bp), C.byref(cfg), out.ctypes.data_as(fp)) == getattr(_capi, "CVO_E_" + code), what
        assert np.all(out == 77), what
    cfg = SGMConfig().c_struct()
    out = np.full(25, 77, np.float32)
    i, o = img.ctypes.data_as(bp), out.ctypes.data_as(fp)
    for args in ((None, i, C.byref(cfg), o), (i, None, C.byref(cfg), o), (i, i, None, o), (i, i, C.byref(cfg), None)):
        assert call(5, 5, *args) == _capi.CVO_E_INVALID
    assert np.all(out == 77)
    # an invalid configuration outranks an unsupported size
    bad = SGMConfig(paths=3).c_struct()
    assert call(4097, 4096, i, i, C.byref(bad), o) == _capi.CVO_E_INVALID
    with pytest.raises(CvoError):
        stereo_disparity_host(np.zeros((5, 5), np.uint8), np.zeros((5, 5), np.uint8), SGMConfig(max_disparity=100))
    with pytest.raises(ValueError):
        stereo_disparity_host(np.zeros((5, 5), np.uint8), np.zeros((5, 6), np.uint8))
    d = _capi.cvo_sgm_config_t()
    L.cvo_sgm_config_default(C.byref(d))
    assert (d.max_disparity, d.p1, d.p2, d.uniqueness, d.lr_max_diff, d.paths) == (128, 10, 120, 5, 1, 8)
    assert tuple(vars(SGMConfig()).values()) == (128, 10, 120, 5, 1, 8) == tuple(np_sgm.DEFAULTS.values())


def test_the_edges_of_the_configuration_are_accepted():
    left, right = sc.noise(3, 5)
    for over in (dict(p1=0, p2=0), dict(p1=193, p2=193), dict(uniqueness=0), dict(uniqueness=99), dict(lr_max_diff=-7), dict(lr_max_diff=1000)):
        assert np.array_equal(stereo_disparity_host(left, right, SGMConfig(**over)), np_sgm.disparity(left, right, **over)), over
