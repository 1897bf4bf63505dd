"""Stereo front end, CPU twin (cvo_stereo_points_host) against the numpy statement np_stereo.py.  Every comparison is exact:
indices equal, float rows bit-equal.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import np_rgbd
import np_stereo
import rgbd_cases as rc
import stereo_cases as sc
from unified_cvo_amd import CvoError, StereoFrame, _capi, stereo_points_host
from unified_cvo_amd.api import CV_FAST, DSO_EDGES, FULL

F32 = np.float32


@pytest.mark.parametrize("name", list(sc.FRAMES))
def test_points_equal_the_statement(name):
    f = sc.frame(name)
    for method in sc.METHODS:
        want = sc.statement_points(name, method)
        sc.assert_points_equal(stereo_points_host(f, method), want, (name, method))
    v = sc.statement_points(name, FULL)["pixel"] // f.cols
    if name == "narrow":
        assert set(v) == set(range(100, 111))  # 100 <= v <= 140 - 30
    if name == "row130":
        assert set(v) == {100}
    if name == "short":
        assert all(len(sc.statement_points(name, m)["pixel"]) == 0 for m in sc.METHODS)  # fewer than 130 rows: no points
    if name == "mono":
        assert stereo_points_host(f, CV_FAST).features().shape[1] == 3
    if name == "semantic":
        cls = np.argmax(f.semantic.reshape(-1, 19), axis=1)
        assert np.count_nonzero(cls == 10) > 1000
        for method in sc.METHODS:
            pc = stereo_points_host(f, method)
            assert pc.num_classes() == 19 and not np.any(cls[pc.pixel] == 10)
            assert np.array_equal(pc.labels(), f.semantic.reshape(-1, 19)[pc.pixel])
        tried, counts, used = sc.statement_points(name, CV_FAST)["schedule"]
        plain = sc.statement_points("kitti", CV_FAST)["schedule"]
        assert used == 10 and plain[2] == 11 and 24000 < counts[-1] <= 28000  # num_want 28000 with classes: one threshold earlier


def test_types_orders_and_nan_rows():
    f = sc.frame("kitti")
    fast, edge, full = (stereo_points_host(f, m) for m in sc.METHODS)
    assert np.all(fast.geometric_types_ == np.array([1, 0], F32)) and np.all(edge.geometric_types_ == np.array([0.9, 0.1], F32))
    assert np.all(full.geometric_types_ == 0.5)
    assert np.all(np.diff(fast.pixel) > 0)                                             # row-major
    u, v = full.pixel % f.cols, full.pixel // f.cols
    assert np.all(np.diff(u * f.rows + v) > 0) and np.any(np.diff(full.pixel) < 0)     # column-major
    nan_rows = np.isnan(full.positions()).any(axis=1)
    assert nan_rows.sum() == 6 and np.all(np.isnan(f.disparity.reshape(-1)[full.pixel[nan_rows]]))  # a NaN disparity fails no test
    assert not np.any(f.disparity.reshape(-1)[full.pixel[~nan_rows]] < F32(0.05))


def _edge_frame(fx, baseline, background, rows=140, cols=16):
    rs = np.random.default_rng(5)
    img = rs.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    disp = np.full((rows, cols), background, F32)
    return img, disp, dict(fx=fx, fy=fx, cx=8.0, cy=105.0, baseline=baseline)


def _kept(img, disp, cal):
    f = StereoFrame(img, disp, **cal)
    pc = stereo_points_host(f, FULL)
    sc.assert_points_equal(pc, sc.points_of(f, FULL), "edges")
    return set(pc.pixel.tolist()), pc


def test_keep_predicate_on_the_image_edges():
    img, disp, cal = _edge_frame(100.0, 0.02, 10.0)
    h, w = disp.shape
    kept, _ = _kept(img, disp, cal)
    at = lambda u, v: v * w + u
    assert at(1, 105) not in kept and at(2, 105) in kept and at(w - 2, 105) in kept and at(w - 1, 105) not in kept
    assert at(5, 99) not in kept and at(5, 100) in kept and at(5, h - 30) in kept and at(5, h - 29) not in kept
    assert len(kept) == (w - 3) * (h - 30 - 100 + 1)


def test_keep_predicate_on_the_disparity_edges():
    img, disp, cal = _edge_frame(100.0, 0.02, 10.0)  # |baseline| fx = 2: a disparity of 0.05 is 40 m away, inside the 55 m cut
    w = disp.shape[1]
    below = np.nextafter(F32(0.05), F32(0))
    values = [F32(0.05), below, F32(-10), F32(0), F32(np.inf), F32(np.nan)]
    for k, val in enumerate(values):
        disp[102, 3 + k] = val
    kept, pc = _kept(img, disp, cal)
    got = [102 * w + 3 + k in kept for k in range(len(values))]
    assert got == [True, False, False, False, True, True]  # 0.05f is kept (0.05f > 0.05 in double), NaN passes, inf is depth 0
    assert float(F32(0.05)) > 0.05 >= float(below)
    row = {int(p): x for p, x in zip(pc.pixel, pc.positions())}
    assert np.all(row[102 * w + 3 + 4] == 0) and np.all(np.isnan(row[102 * w + 3 + 5])) and row[102 * w + 3][2] == F32(2.0) / F32(0.05)
    neg = dict(cal, baseline=-0.02)  # the absolute value of the baseline is used
    assert _kept(img, disp, neg)[0] == kept


def test_keep_predicate_at_55_metres():
    """fx = fy = 1 makes Kinv exact (x = (u - cx) depth) and a disparity of 1 makes depth = |baseline|, so the pixel at the
    principal point has norm = sqrt(b b) = b: at b = 55 it is rejected (norm >= 55), at the float just below 55 it is kept."""
    prev55 = np.nextafter(F32(55), F32(0))
    for baseline, inside in ((55.0, False), (float(prev55), True)):
        img, disp, cal = _edge_frame(1.0, baseline, 10.0)
        w = disp.shape[1]
        u, v = int(cal["cx"]), int(cal["cy"])
        disp[v, u] = disp[v, u + 1] = F32(1)  # (u + 1: x = z = depth, norm = sqrt(2) depth, beyond 55 either way)
        _, norm = np_stereo.back_project(np.array([u]), np.array([v]), np.array([1], F32), sc.calib(StereoFrame(img, disp, **cal)))
        assert norm[0] == F32(baseline)
        kept, pc = _kept(img, disp, cal)
        assert (v * w + u in kept) == inside and v * w + u + 1 not in kept and v * w + u + 2 in kept
        if inside:
            p = pc.positions()[list(pc.pixel).index(v * w + u)]
            assert p[0] == 0 and p[1] == 0 and p[2] == prev55


def test_recipe_of_twin_pieces_equals_the_statement():
    """The multi-frame KITTI driver's block from the twin's pieces - the DSO_EDGES and FULL points through the voxel
    contract's CPU twin - against the statement's recipe, at the driver's divisor 5 and at 10."""
    L = _capi.lib()

    def voxel(xyz, s):
        kept = np.zeros(max(len(xyz), 1), np.int32)
        n = C.c_int()
        assert L.cvo_voxel_select_host(len(xyz), np.ascontiguousarray(xyz, F32).ctypes.data_as(C.POINTER(C.c_float)), s,
                                       kept.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n)) == 0
        return kept[:n.value]

    f = sc.frame("kitti", 0.0, False)
    for div in (5, 10):
        r = sc.statement_recipe("kitti", 0.5, div)
        pix, xyz = [], []
        for method, s in ((DSO_EDGES, F32(0.5) / F32(div)), (FULL, F32(0.5))):
            pc = stereo_points_host(f, method)
            k = voxel(pc.positions(), float(s))
            pix.append(pc.pixel[k])
            xyz.append(pc.positions()[k])
        ne = int(r["is_edge"].sum())
        assert 0 < ne == len(pix[0]) < len(r["pixel"])
        assert np.array_equal(np.concatenate(pix), r["pixel"]) and np.array_equal(sc.bits(np.concatenate(xyz)), sc.bits(r["xyz"]))
        assert np.all(r["geotype"][:ne] == np.array([1, 0], F32)) and np.all(r["geotype"][ne:] == np.array([0, 1], F32))
        want = (f.image.reshape(-1, 3)[r["pixel"]].astype(np.float64) / 255.0).astype(F32)
        assert np.array_equal(r["feat"][:, :3], want) and np.all(r["feat"][:, 3:] == 0)
    assert len(sc.statement_recipe("kitti", 0.5, 10)["pixel"]) > len(sc.statement_recipe("kitti", 0.5, 5)["pixel"])


def _raw_call(fs, method=FULL, pixel=True):
    L = _capi.lib()
    px = np.full(16, -7, np.int32)
    n = C.c_int(-7)
    rcode = L.cvo_stereo_points_host(C.byref(fs), method, px.ctypes.data_as(C.POINTER(C.c_int)) if pixel else None, C.byref(n), None, None, None, None)
    assert n.value == -7 and np.all(px == -7)  # nothing written on a refusal
    return rcode


def test_refusals():
    f = sc.frame("narrow")
    for field, value in (("rows", 0), ("cols", -1), ("channels", 2), ("channels", 4), ("image", None), ("disparity", None),
                         ("fx", 0.0), ("fx", float("nan")), ("fy", 0.0), ("fy", float("inf")), ("baseline", 0.0),
                         ("baseline", float("nan")), ("baseline", float("-inf")), ("num_classes", 3)):
        fs = f.c_struct()
        setattr(fs, field, value)
        assert _raw_call(fs) == _capi.CVO_E_INVALID, (field, value)
    assert _raw_call(f.c_struct(), pixel=False) == _capi.CVO_E_INVALID
    for method in (1, 3, 4, 5, 6, 7):  # RANDOM ... LOAM
        assert _raw_call(f.c_struct(), method) == _capi.CVO_E_UNSUPPORTED
    assert _raw_call(f.c_struct(), 9) == _capi.CVO_E_INVALID and _raw_call(f.c_struct(), -1) == _capi.CVO_E_INVALID
    big = f.c_struct()
    big.rows, big.cols = 4097, 4096
    assert _raw_call(big) == _capi.CVO_E_UNSUPPORTED  # more than 2^24 pixels
    wide = StereoFrame(np.zeros((36, 3210), np.uint8), np.ones((36, 3210), F32), 500, 500, 1600, 18, 0.5)
    assert _raw_call(wide.c_struct(), DSO_EDGES) == _capi.CVO_E_UNSUPPORTED  # the DSO threshold index leaves its allocation
    assert stereo_points_host(wide, CV_FAST).num_points() == 0 and stereo_points_host(wide, FULL).num_points() == 0
    with pytest.raises(CvoError):
        bad = StereoFrame(f.image, f.disparity, 0.0, f.fy, f.cx, f.cy, f.baseline)
        stereo_points_host(bad, FULL)
    tiny = StereoFrame(np.zeros((5, 6), np.uint8), np.ones((5, 6), F32), 1, 1, 3, 2, 0.5)  # under 7 on a side: valid, no corners
    assert stereo_points_host(tiny, CV_FAST).num_points() == 0


def test_rgbd_constructor_still_refuses_cv_fast():
    """cvo_rgbd_points_host keeps refusing method 0: RGB-D users get CV_FAST pixels from cvo_fast_select with CVO_FAST_RGBD."""
    f = rc.frame("tiny")
    fs = f.c_struct()
    px = np.full(16, -7, np.int32)
    n = C.c_int(-7)
    r = _capi.lib().cvo_rgbd_points_host(C.byref(fs), CV_FAST, px.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n), None, None, None, None)
    assert r == _capi.CVO_E_UNSUPPORTED and n.value == -7 and np.all(px == -7)
    assert np_rgbd.DSO_EDGES == DSO_EDGES and np_rgbd.FULL == FULL and CV_FAST == 0
