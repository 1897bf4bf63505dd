"""RGB-D front end, CPU twin (cvo_rgbd_points_host) against the numpy statement np_rgbd.py.  Every comparison is exact:
indices equal, float rows bit-equal.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import np_rgbd
import rgbd_cases as rc
from unified_cvo_amd import CvoError, RGBDFrame, _capi, rgbd_points_host, synth
from unified_cvo_amd.api import DSO_EDGES, FULL


def test_schedule_branches_of_the_statement():
    """The frames make every branch of dso_select_pixels' schedule run (the statement returns the potentials tried)."""
    seen = set()
    for name, (_, tried) in rc.FRAMES.items():
        if tried is None:
            continue
        f = rc.frame(name)
        uv, got, counts = np_rgbd.dso_select(np_rgbd.gray_plane(f.image))
        assert got == tried, (name, got, counts)
        seen.add(tuple(got))
        if name == "edge":
            assert counts[0] > 10000 and counts[1] < 6666 and len(uv) == counts[2] == counts[0]
        if name == "noisy720":
            assert min(counts) > 10000  # left the loop through `times == 5`, not through the count
    assert {(3, 4, 5), (3, 4), (3, 2), (3, 4, 3), (3, 4, 5, 6, 7)} <= seen


def test_gradient_is_exact_in_float32_and_has_perfect_squares():
    """dx, dy are multiples of 0.5, g2 a multiple of 0.25 below 2^16: float32 holds them exactly (no contraction can
    change them); int(sqrtf(g2)) must come out right at dx = 3, dy = 4."""
    for name in ("textured", "small", "mono"):
        f = rc.frame(name)
        I = np_rgbd.gray_plane(f.image, f.gray)
        grad, g2 = np_rgbd.gradient(I)
        I64 = I.astype(np.float64)
        dx = np.zeros_like(I64)
        dy = np.zeros_like(I64)
        dx[1:-1, 1:-1] = 0.5 * (I64[1:-1, 2:] - I64[1:-1, :-2])
        dy[1:-1, 1:-1] = 0.5 * (I64[2:, 1:-1] - I64[:-2, 1:-1])
        assert np.array_equal(grad.reshape(-1, 2)[:, 0].astype(np.float64), dx.reshape(-1))
        assert np.array_equal(g2.astype(np.float64), (dx * dx + dy * dy).reshape(-1))
        assert np.all(np.mod(g2.astype(np.float64) * 4, 1) == 0) and g2.max() < 2 ** 16
        assert np.count_nonzero(g2 == 25.0) > 0 and np.count_nonzero(g2 == 169.0) > 0, name
        assert np.all(np.sqrt(g2[g2 == 25.0]).astype(np.int64) == 5)


def test_threshold_index_aliases_on_odd_shapes():
    """200 x 150 reads block column 6 of 6 (the next block row's first entry); 1241 x 376 reads into the zero slack."""
    idx = np_rgbd.threshold_index(150, 200)[np_rgbd.considered(150, 200)]
    assert 200 // 32 == 6 and np.any(idx % 6 == 0) and idx.max() >= 24
    idx = np_rgbd.threshold_index(376, 1241)[np_rgbd.considered(376, 1241)]
    assert idx.max() >= (1241 // 32) * (376 // 32)


@pytest.mark.parametrize("depth", rc.DEPTHS)
@pytest.mark.parametrize("name", list(rc.FRAMES))
def test_points_equal_the_statement(name, depth):
    f = rc.frame(name, depth)
    for method in (DSO_EDGES, FULL):
        rc.assert_points_equal(rgbd_points_host(f, method), rc.statement_points(f, method), (name, depth, method))


def test_caller_gray_plane_overrides_the_formula():
    f = rc.own_gray(rc.frame("small"))
    got = rgbd_points_host(f, DSO_EDGES)
    rc.assert_points_equal(got, rc.statement_points(f, DSO_EDGES), "own-gray")
    assert not np.array_equal(got.pixel, rgbd_points_host(rc.frame("small"), DSO_EDGES).pixel)


def test_semantic_frame_drops_class_10_and_copies_rows():
    f = rc.frame("semantic")
    cls = np.argmax(f.semantic.reshape(-1, 19), axis=1)
    assert np.count_nonzero(cls == 10) > 1000
    for method in (DSO_EDGES, FULL):
        pc = rgbd_points_host(f, method)
        assert pc.num_classes() == 19 and not np.any(cls[pc.pixel] == 10)
        assert np.array_equal(pc.labels(), f.semantic.reshape(-1, 19)[pc.pixel])
    plain = RGBDFrame(f.image, f.depth, f.fx, f.fy, f.cx, f.cy, f.scaling_factor)
    assert rgbd_points_host(plain, FULL).num_points() > rgbd_points_host(f, FULL).num_points()


def test_all_zero_depth_is_an_empty_cloud():
    for depth in rc.DEPTHS:
        f = rc.zero_depth(rc.frame("small", depth))
        for method in (DSO_EDGES, FULL):
            pc = rgbd_points_host(f, method)
            assert pc.num_points() == 0 and len(pc.pixel) == 0


def test_full_is_column_major_with_type_half_half():
    f = rc.frame("small")
    pc = rgbd_points_host(f, FULL)
    u, v = pc.pixel % f.cols, pc.pixel // f.cols
    assert np.all(np.diff(u * f.rows + v) > 0) and np.any(np.diff(pc.pixel) < 0)
    assert np.all(pc.geometric_types_ == 0.5)
    e = rgbd_points_host(f, DSO_EDGES)
    assert np.all(e.geometric_types_ == np.array([0.9, 0.1], np.float32))


def test_gradient_index_quirk_matters():
    """Features 3 and 4 read gradient_[v w + u] and gradient_[v w + u + 1] of the interleaved array - the statement's
    values - and differ from the `intended` gradient_[2 (v w + u)], gradient_[2 (v w + u) + 1] on this frame."""
    f = rc.frame("small")
    pc = rgbd_points_host(f, DSO_EDGES)
    grad, _ = np_rgbd.gradient(np_rgbd.gray_plane(f.image))
    quirk = (grad[pc.pixel].astype(np.float64) / 500.0 + 0.5).astype(np.float32)
    intended = (grad[2 * pc.pixel].astype(np.float64) / 500.0 + 0.5).astype(np.float32)
    assert np.array_equal(pc.features()[:, 3], quirk)
    assert np.count_nonzero(pc.features()[:, 3] != intended) > len(quirk) // 4


def test_byte_round_trip_is_the_identity():
    c = np.arange(256)
    f = (c.astype(np.float32).astype(np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(np_rgbd.byte_round_trip(f), c.astype(np.uint8))


def test_recipe_of_the_statement_is_edges_then_surfaces():
    f = rc.frame("small")
    r = rc.statement_recipe(f, 0.1)
    ne = int(r["is_edge"].sum())
    assert 0 < ne < len(r["pixel"]) and np.all(r["is_edge"][:ne] == 1) and np.all(r["is_edge"][ne:] == 0)
    assert np.all(r["geotype"][:ne] == np.array([1, 0], np.float32)) and np.all(r["geotype"][ne:] == np.array([0, 1], np.float32))
    assert np.all(r["feat"][:, 3:] == 0)
    want = (f.image.reshape(-1, 3)[r["pixel"]].astype(np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(r["feat"][:, :3], want)  # the pixel's channels over 255: the gradient features are dropped


def _raw_call(fs, method=FULL, pixel=True):
    L = _capi.lib()
    px = np.full(16, -7, np.int32)
    n = C.c_int(-7)
    rcode = L.cvo_rgbd_points_host(C.byref(fs), method, px.ctypes.data_as(C.POINTER(C.c_int)) if pixel else None, C.byref(n), None, None, None, None)
    assert n.value == -7 and np.all(px == -7)  # nothing written on a refusal
    return rcode


def test_refusals():
    f = rc.frame("tiny")
    for field, value in (("rows", 0), ("cols", -1), ("channels", 2), ("channels", 4), ("image", None), ("depth", None), ("depth_type", 5),
                         ("fx", 0.0), ("fx", float("nan")), ("fy", -1.0), ("fy", float("inf")), ("scaling_factor", 0.0),
                         ("scaling_factor", float("nan")), ("num_classes", 3)):
        fs = f.c_struct()
        setattr(fs, field, value)
        assert _raw_call(fs) == _capi.CVO_E_INVALID, (field, value)
    assert _raw_call(f.c_struct(), pixel=False) == _capi.CVO_E_INVALID
    for method in (0, 1, 3, 4, 5, 6, 7):  # CV_FAST, RANDOM ... LOAM: OpenCV detectors, rand(), LiDAR
        assert _raw_call(f.c_struct(), method) == _capi.CVO_E_UNSUPPORTED
    assert _raw_call(f.c_struct(), 9) == _capi.CVO_E_INVALID and _raw_call(f.c_struct(), -1) == _capi.CVO_E_INVALID
    with pytest.raises(CvoError):
        bad = rc.frame("tiny")
        bad.fx = 0.0
        rgbd_points_host(bad, FULL)
    # images under 32 pixels on a side are valid: zero whole blocks, zero thresholds
    assert rgbd_points_host(f, DSO_EDGES).num_points() > 0


def test_threshold_index_beyond_the_allocation_is_unsupported():
    """A 3210 x 36 image: (x >> 5) + (y >> 5) * (cols / 32) reaches 100 + 1 * 100 of 100 * 1 + 100 entries (it takes more
    than 100 block columns and a ragged last block row)."""
    rows, cols = 36, 3210
    img = np.zeros((rows, cols), np.uint8)
    f = RGBDFrame(img, np.ones((rows, cols), np.uint16), 500, 500, 1600, 18, 5000)
    assert ((rows - 4) >> 5) * (cols // 32) + ((cols - 6) >> 5) >= (cols // 32) * (rows // 32) + 100
    with pytest.raises(np_rgbd.Unsupported):
        np_rgbd.dso_select(np_rgbd.gray_plane(f.image))
    assert _raw_call(f.c_struct(), DSO_EDGES) == _capi.CVO_E_UNSUPPORTED
    assert rgbd_points_host(f, FULL).num_points() == rows * cols
