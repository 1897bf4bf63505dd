"""Stereo front end on the MI355X: cvo_stereo_points / cvo_cloud_upload_stereo / _recipe against the numpy statement
(np_stereo.py), the CPU twin and an ordinary upload of the statement's rows.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import cases
import stereo_cases as sc
from unified_cvo_amd import CvoGPU, CvoPointCloud, CvoError, StereoFrame, _capi, synth
from unified_cvo_amd.api import CV_FAST, DSO_EDGES, FULL

pytestmark = pytest.mark.gpu

LEAF = 0.5
HOST_BELOW, RECIPE_HOST_BELOW = 10000, 24000  # frames with fewer pixels take the CPU twin unless STEREO_HOST says otherwise
RECIPE_FRAMES = ("kitti", "mono", "narrow", "short")


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    yield g
    g.close()


def _cloud(want):
    return CvoPointCloud.from_arrays(want["xyz"], want["feat"], want.get("label"), want["geotype"])


def _same_resident(gpu, d, want_cloud):
    if want_cloud.num_points() == 0:
        assert d.n == 0
        return
    u = gpu.upload(want_cloud)
    try:
        assert d.n == u.n and np.array_equal(d.debug_order(), u.debug_order())
    finally:
        u.free()


@pytest.mark.parametrize("name", list(sc.FRAMES))
def test_kernels_equal_the_statement(gpu, name):
    """STEREO_HOST=0: the kernels on every frame, the small ones included; the NaN-disparity rows are the statement's."""
    f = sc.frame(name)
    gpu.set_option("STEREO_HOST", 0)
    try:
        for method in sc.METHODS:
            want = sc.statement_points(name, method)
            sc.assert_points_equal(gpu.stereo_points(f, method), want, (name, method))
            st = gpu.debug_stereo_stats()
            assert st["on_device"] and st["candidates"] == want["candidates"] and st["kept"] == len(want["pixel"]), (name, method, st)
            if method == CV_FAST:
                tried, counts, used = want["schedule"]
                assert st["tried"] == tried and st["counts"] == counts and st["threshold_used"] == used, (name, st)
            elif method == DSO_EDGES:
                assert st["tried"] == want["schedule"][0] and st["counts"] == want["schedule"][1] and st["threshold_used"] == -1
            if method != FULL or f.rows * f.cols < 100000:  # (an ordinary upload of FULL's 280 000 rows is not what this test is about)
                d = gpu.upload_stereo(f, method)
                assert np.array_equal(d.pixel, want["pixel"])
                _same_resident(gpu, d, _cloud(want))
                d.free()
        if name in ("kitti", "mono"):
            full = sc.statement_points(name, FULL)
            assert np.isnan(full["xyz"]).any(axis=1).sum() == 6
    finally:
        gpu.set_option("STEREO_HOST", None)


@pytest.mark.parametrize("name", RECIPE_FRAMES)
def test_recipe_equals_the_statement(gpu, name):
    f = sc.frame(name, 0.0, False)
    gpu.set_option("STEREO_HOST", 0)
    try:
        for div in (5, 10):
            r = sc.statement_recipe(name, LEAF, div)
            d = gpu.upload_stereo_recipe(f, LEAF, div)
            assert d.n == len(r["pixel"]) and np.array_equal(d.pixel, r["pixel"]) and np.array_equal(d.is_edge, r["is_edge"].astype(bool)), (name, div)
            st = gpu.debug_stereo_stats()
            assert st["on_device"] and st["candidates"] == r["stats"]["candidates"] and st["kept"] == r["stats"]["kept"], (name, st)
            assert st["tried"] == r["stats"]["schedule"][0] and st["counts"] == r["stats"]["schedule"][1]
            _same_resident(gpu, d, CvoPointCloud.from_arrays(r["xyz"], r["feat"], None, r["geotype"]))
            d.free()
        if name == "kitti":
            assert 1000 < len(sc.statement_recipe(name, LEAF, 5)["pixel"]) < len(sc.statement_recipe(name, LEAF, 10)["pixel"])
    finally:
        gpu.set_option("STEREO_HOST", None)


def test_recipe_refuses_a_nan_disparity_in_the_kept_region(gpu):
    """The voxel contract refuses non-finite coordinates, on both routes; cvo_cloud_upload_stereo takes such rows as
    cvo_cloud_upload does (test_kernels_equal_the_statement compares the two)."""
    f = sc.frame("mono")
    for route in (0, 1):
        gpu.set_option("STEREO_HOST", route)
        try:
            with pytest.raises(CvoError, match="non-finite"):
                gpu.upload_stereo_recipe(f, LEAF)
        finally:
            gpu.set_option("STEREO_HOST", None)


def test_routes_agree_and_repeats_are_identical(gpu):
    for name in ("kitti", "mono", "semantic", "narrow", "small"):  # 466 616, 64 000, 466 616, 10 080 and 8 400 pixels
        f = StereoFrame(**synth.stereo_frame(rows=140, cols=60)) if name == "small" else sc.frame(name, 0.0, False)
        res = {}
        for route in (0, 1, None):
            gpu.set_option("STEREO_HOST", route)
            try:
                out = []
                for method in sc.METHODS:
                    p = gpu.stereo_points(f, method)
                    assert gpu.debug_stereo_stats()["on_device"] == (route == 0 or (route is None and f.rows * f.cols >= HOST_BELOW)), (name, route)
                    out += [p.pixel, p.positions(), p.features()]
                d = gpu.upload_stereo_recipe(f, LEAF)
                assert gpu.debug_stereo_stats()["on_device"] == (route == 0 or (route is None and f.rows * f.cols >= RECIPE_HOST_BELOW)), (name, route)
                e = gpu.upload_stereo(f, CV_FAST)
                assert gpu.debug_stereo_stats()["on_device"] == (route == 0 or (route is None and f.rows * f.cols >= HOST_BELOW)), (name, route)
                res[route] = out + [d.pixel, d.is_edge, d.debug_order(), e.pixel, e.debug_order()]
                d.free()
                e.free()
            finally:
                gpu.set_option("STEREO_HOST", None)
        for route in (1, None):
            for a, b in zip(res[0], res[route]):
                assert np.array_equal(sc.bits(a) if a.dtype == np.float32 else a, sc.bits(b) if b.dtype == np.float32 else b), (name, route)
    f = sc.frame("kitti", 0.0, False)
    gpu.set_option("STEREO_HOST", 0)
    try:
        first, first_recipe = gpu.upload_stereo(f, CV_FAST), gpu.upload_stereo_recipe(f, LEAF)
        for _ in range(10):
            d, r = gpu.upload_stereo(f, CV_FAST), gpu.upload_stereo_recipe(f, LEAF)
            assert np.array_equal(d.pixel, first.pixel) and np.array_equal(d.debug_order(), first.debug_order())
            assert np.array_equal(r.pixel, first_recipe.pixel) and np.array_equal(r.is_edge, first_recipe.is_edge)
            assert np.array_equal(r.debug_order(), first_recipe.debug_order())
            d.free()
            r.free()
        first.free()
        first_recipe.free()
    finally:
        gpu.set_option("STEREO_HOST", None)


def test_own_gray_plane_and_mono_padding(gpu):
    gpu.set_option("STEREO_HOST", 0)
    try:
        f = sc.frame("kitti")
        g = np.ascontiguousarray(f.image[..., 1])
        own = StereoFrame(f.image, f.disparity, f.fx, f.fy, f.cx, f.cy, f.baseline, gray=g)
        got = gpu.stereo_points(own, CV_FAST)
        sc.assert_points_equal(got, sc.points_of(own, CV_FAST), "own-gray")
        assert not np.array_equal(got.pixel, sc.statement_points("kitti", CV_FAST)["pixel"])
        m = sc.frame("mono")
        want = sc.statement_points("mono", CV_FAST)
        assert want["feat"].shape[1] == 3
        padded = np.zeros((len(want["pixel"]), 5), np.float32)
        padded[:, :3] = want["feat"]
        d = gpu.upload_stereo(m, CV_FAST)
        _same_resident(gpu, d, CvoPointCloud.from_arrays(want["xyz"], padded, None, want["geotype"]))
        d.free()
    finally:
        gpu.set_option("STEREO_HOST", None)


def _trace_equal(r1, r2):
    assert r1.iterations == r2.iterations and np.array_equal(r1.transform, r2.transform)
    assert len(r1.trace) == len(r2.trace) > 0
    for t1, t2 in zip(r1.trace, r2.trace):
        for name, _ in _capi.cvo_trace_t._fields_:
            x, y = getattr(t1, name), getattr(t2, name)
            assert (x == y) if isinstance(x, (int, float)) else (list(x) == list(y)), (t1.k, name)


def test_resident_cloud_is_an_upload_of_the_statement_rows():
    """Two views of the scene, the camera moved sideways by 3 pixels, uploaded with CV_FAST: align and inner product on the
    clouds of upload_stereo equal, bit for bit, those on upload(statement rows).  The plumbing, not accuracy."""
    p = cases.load_params("geometric_gpu")
    p.MAX_ITER = 40
    g = CvoGPU(params=p)
    try:
        g.set_option("STEREO_HOST", 0)
        fa, fb = sc.frame("kitti", 0.0, False), sc.frame("kitti", 3.0, False)
        wa, wb = sc.points_of(fa, CV_FAST), sc.points_of(fb, CV_FAST)
        da, db = g.upload_stereo(fa, CV_FAST), g.upload_stereo(fb, CV_FAST)
        assert np.array_equal(da.pixel, wa["pixel"]) and np.array_equal(db.pixel, wb["pixel"])
        assert da.n > 5000 and not np.array_equal(da.pixel, db.pixel)
        ua, ub = g.upload(_cloud(wa)), g.upload(_cloud(wb))
        assert np.array_equal(da.debug_order(), ua.debug_order()) and np.array_equal(db.debug_order(), ub.debug_order())
        init = np.eye(4, dtype=np.float32)
        it = 40
        _trace_equal(g.align(da, db, init, max_iterations=it, trace_capacity=it, trace_dense=it),
                     g.align(ua, ub, init, max_iterations=it, trace_capacity=it, trace_dense=it))
        ip1, ip2 = g.inner_product_gpu(da, db, init, 0.3), g.inner_product_gpu(ua, ub, init, 0.3)
        assert ip1 == ip2 and ip1 > 0
    finally:
        g.close()


def test_refusals_and_their_messages_leave_the_context_usable(gpu):
    f = sc.frame("narrow")
    before = gpu.upload_stereo_recipe(f, LEAF).pixel
    ipp = C.POINTER(C.c_int)
    for field, value, text in (("rows", 0, "rows and cols"), ("cols", -1, "rows and cols"), ("channels", 2, "channels must be 1 or 3"),
                               ("image", None, "image is NULL"), ("disparity", None, "disparity is NULL"), ("fx", 0.0, "fx and fy"),
                               ("fy", float("nan"), "fx and fy"), ("fx", float("inf"), "fx and fy"), ("baseline", 0.0, "baseline"),
                               ("baseline", float("nan"), "baseline"), ("num_classes", 3, "semantic")):
        fs = f.c_struct()
        setattr(fs, field, value)
        px = np.full(2 * f.rows * f.cols, -7, np.int32)
        n = C.c_int(-7)
        calls = (lambda h: gpu.L.cvo_stereo_points(gpu.ctx, C.byref(fs), FULL, px.ctypes.data_as(ipp), C.byref(n), None, None, None, None),
                 lambda h: gpu.L.cvo_cloud_upload_stereo(gpu.ctx, C.byref(fs), CV_FAST, C.byref(h), px.ctypes.data_as(ipp), C.byref(n)),
                 lambda h: gpu.L.cvo_cloud_upload_stereo_recipe(gpu.ctx, C.byref(fs), 0.5, 5.0, C.byref(h), px.ctypes.data_as(ipp), None, C.byref(n)))
        for call in calls:
            h = C.c_void_p(0)
            assert call(h) == _capi.CVO_E_INVALID and text in gpu.L.cvo_last_error(gpu.ctx).decode(), (field, gpu.L.cvo_last_error(gpu.ctx))
            assert n.value == -7 and np.all(px == -7) and not h.value  # nothing written
    for leaf in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(CvoError, match="leaf"):
            gpu.upload_stereo_recipe(f, leaf)
    for div in (0.0, -4.0, float("nan"), float("inf")):
        with pytest.raises(CvoError, match="edge_divisor"):
            gpu.upload_stereo_recipe(f, 0.5, div)
    for method in (1, 5, 6):  # RANDOM, CANNY_EDGES, EDGES_ONLY
        with pytest.raises(CvoError, match="error -5.*not supported"):
            gpu.stereo_points(f, method)
        with pytest.raises(CvoError, match="error -5.*not supported"):
            gpu.upload_stereo(f, method)
    wide = StereoFrame(np.zeros((36, 3210), np.uint8), np.ones((36, 3210), np.float32), 500, 500, 1600, 18, 0.5)
    with pytest.raises(CvoError, match="error -5.*threshold index"):
        gpu.upload_stereo_recipe(wide, 0.5)
    with pytest.raises(CvoError, match="error -5.*threshold index"):
        gpu.stereo_points(wide, DSO_EDGES)
    assert gpu.stereo_points(wide, CV_FAST).num_points() == 0
    assert np.array_equal(gpu.upload_stereo_recipe(f, LEAF).pixel, before)
