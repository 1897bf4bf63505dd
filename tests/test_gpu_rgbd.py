"""RGB-D front end on the MI355X: cvo_rgbd_points / cvo_cloud_upload_rgbd against the numpy statement (np_rgbd.py), the
CPU twin and an ordinary upload of the statement's rows.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import cases
import np_rgbd
import rgbd_cases as rc
from unified_cvo_amd import CvoGPU, CvoPointCloud, CvoError, RGBDFrame, _capi
from unified_cvo_amd.api import DSO_EDGES, FULL

pytestmark = pytest.mark.gpu

LEAF = 0.1


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    yield g
    g.close()


def _recipe_cloud(r):
    return CvoPointCloud.from_arrays(r["xyz"], r["feat"], None, r["geotype"])


def _assert_recipe_equal(d, r, name):
    assert d.n == len(r["pixel"]) and np.array_equal(d.pixel, r["pixel"]), name
    assert np.array_equal(d.is_edge, r["is_edge"].astype(bool)), name


@pytest.mark.parametrize("depth", rc.DEPTHS)
@pytest.mark.parametrize("name", list(rc.FRAMES))
def test_kernels_equal_the_statement(gpu, name, depth):
    """RGBD_HOST=0: the kernels on every frame, the small ones included."""
    f = rc.frame(name, depth)
    gpu.set_option("RGBD_HOST", 0)
    try:
        for method in (DSO_EDGES, FULL):
            want = rc.statement_points(f, method)
            rc.assert_points_equal(gpu.rgbd_points(f, method), want, (name, depth, method))
            st = gpu.debug_rgbd_stats()
            assert st["on_device"]
            if method == DSO_EDGES:
                tried, counts = want["schedule"]
                assert st["potentials"] == tried and st["counts"] == counts, (name, st)
                if rc.FRAMES[name][1] is not None:
                    assert tried == rc.FRAMES[name][1]
                assert st["edge_selected"] == counts[-1] and st["edge_points"] == len(want["pixel"])
            else:
                assert st["surface_points"] == len(want["pixel"]) and st["with_depth"] == want["with_depth"], (name, st)
        r = rc.statement_recipe(f, LEAF)
        d = gpu.upload_rgbd(f, LEAF)
        _assert_recipe_equal(d, r, (name, depth))
        st = gpu.debug_rgbd_stats()
        assert st["on_device"] and st["with_depth"] == r["stats"]["with_depth"]
        assert st["edge_points"] == r["stats"]["edge"]["candidates"] and st["surface_points"] == r["stats"]["surface"]["candidates"]
        assert st["potentials"] == r["stats"]["edge"]["schedule"][0] and st["counts"] == r["stats"]["edge"]["schedule"][1]
        u = gpu.upload(_recipe_cloud(r))
        assert np.array_equal(d.debug_order(), u.debug_order())
        d.free()
        u.free()
    finally:
        gpu.set_option("RGBD_HOST", None)


def test_routes_agree_and_repeats_are_identical(gpu):
    for name in ("textured", "small", "semantic", "mono"):
        f = rc.frame(name)
        res = {}
        for route in (0, 1, None):
            gpu.set_option("RGBD_HOST", route)
            try:
                e, s = gpu.rgbd_points(f, DSO_EDGES), gpu.rgbd_points(f, FULL)
                d = gpu.upload_rgbd(f, LEAF)
                on_device = gpu.debug_rgbd_stats()["on_device"]
                assert on_device == (route == 0 or (route is None and f.rows * f.cols >= 32768)), (name, route)
                res[route] = (e.pixel, e.positions(), e.features(), s.pixel, s.positions(), s.features(), d.pixel, d.is_edge, d.debug_order())
                d.free()
            finally:
                gpu.set_option("RGBD_HOST", None)
        for route in (1, None):
            for a, b in zip(res[0], res[route]):
                assert np.array_equal(rc.bits(a) if a.dtype == np.float32 else a, rc.bits(b) if b.dtype == np.float32 else b), (name, route)
    f = rc.frame("textured", "f32")
    gpu.set_option("RGBD_HOST", 0)
    try:
        first = gpu.upload_rgbd(f, LEAF)
        e0 = gpu.rgbd_points(f, DSO_EDGES)
        for _ in range(10):
            d = gpu.upload_rgbd(f, LEAF)
            assert np.array_equal(d.pixel, first.pixel) and np.array_equal(d.is_edge, first.is_edge)
            assert np.array_equal(d.debug_order(), first.debug_order())
            d.free()
            assert np.array_equal(gpu.rgbd_points(f, DSO_EDGES).pixel, e0.pixel)
        first.free()
    finally:
        gpu.set_option("RGBD_HOST", None)


def test_own_gray_and_zero_depth(gpu):
    gpu.set_option("RGBD_HOST", 0)
    try:
        f = rc.own_gray(rc.frame("textured"))
        rc.assert_points_equal(gpu.rgbd_points(f, DSO_EDGES), rc.statement_points(f, DSO_EDGES), "own-gray")
        _assert_recipe_equal(gpu.upload_rgbd(f, LEAF), rc.statement_recipe(f, LEAF), "own-gray")
        for depth in rc.DEPTHS:
            z = rc.zero_depth(rc.frame("small", depth))
            for method in (DSO_EDGES, FULL):
                assert gpu.rgbd_points(z, method).num_points() == 0
            d = gpu.upload_rgbd(z, LEAF)
            assert d.n == 0 and len(d.pixel) == 0
    finally:
        gpu.set_option("RGBD_HOST", None)


def test_leaf_defaults_to_the_yaml_value_and_divisor_is_used(gpu):
    f = rc.frame("small")
    gpu.set_option("RGBD_HOST", 0)
    try:
        leaf = gpu.params.multiframe_downsample_voxel_size
        _assert_recipe_equal(gpu.upload_rgbd(f), rc.statement_recipe(f, leaf), "default leaf")
        for div in (5, 10):
            _assert_recipe_equal(gpu.upload_rgbd(f, 0.25, div), rc.statement_recipe(f, 0.25, div), div)
    finally:
        gpu.set_option("RGBD_HOST", None)


def _trace_equal(r1, r2):
    assert r1.iterations == r2.iterations and np.array_equal(r1.transform, r2.transform)
    assert len(r1.trace) == len(r2.trace) > 0
    for t1, t2 in zip(r1.trace, r2.trace):
        for name, _ in _capi.cvo_trace_t._fields_:
            x, y = getattr(t1, name), getattr(t2, name)
            assert (x == y) if isinstance(x, (int, float)) else (list(x) == list(y)), (t1.k, name)


@pytest.mark.parametrize("config", ["geometric_gpu", "intensity_gpu"])
def test_resident_cloud_is_an_upload_of_the_statement_rows(config):
    """Two views of the scene, the camera moved sideways: inner product and align on the clouds of upload_rgbd equal, bit
    for bit, those on upload(statement rows)."""
    p = cases.load_params(config)
    p.MAX_ITER = 40
    g = CvoGPU(params=p)
    try:
        g.set_option("RGBD_HOST", 0)
        fa, fb = rc.frame("textured"), rc.frame("textured", shift=3.0)
        da, db = g.upload_rgbd(fa, LEAF), g.upload_rgbd(fb, LEAF)
        ra, rb = rc.statement_recipe(fa, LEAF), rc.statement_recipe(fb, LEAF)
        _assert_recipe_equal(da, ra, "a")
        _assert_recipe_equal(db, rb, "b")
        assert da.n > 2000 and not np.array_equal(da.pixel, db.pixel)
        ua, ub = g.upload(_recipe_cloud(ra)), g.upload(_recipe_cloud(rb))
        assert np.array_equal(da.debug_order(), ua.debug_order()) and np.array_equal(db.debug_order(), ub.debug_order())
        init = np.eye(4, dtype=np.float32)
        it = 40
        _trace_equal(g.align(da, db, init, max_iterations=it, trace_capacity=it, trace_dense=it),
                     g.align(ua, ub, init, max_iterations=it, trace_capacity=it, trace_dense=it))
        ip1, ip2 = g.inner_product_gpu(da, db, init, 0.3), g.inner_product_gpu(ua, ub, init, 0.3)
        assert ip1 == ip2 and ip1 > 0
    finally:
        g.close()


def test_multiframe_on_rgbd_uploaded_frames():
    from test_gpu_multiframe import _mf_params
    g = CvoGPU(params=_mf_params(max_iters=8))
    try:
        g.set_option("RGBD_HOST", 0)
        frames = [rc.frame("textured", shift=2.0 * k) for k in range(4)]
        dev = [g.upload_rgbd(f, 0.2) for f in frames]
        host = [g.upload(_recipe_cloud(rc.statement_recipe(f, 0.2))) for f in frames]
        X0 = np.tile(np.eye(4)[:3].reshape(12), (4, 1))
        for k in range(1, 4):
            X0[k, 3] = 0.01 * k  # a small sideways offset per frame
        edges = [0, 1, 1, 2, 2, 3, 0, 2]
        hold = [1, 0, 0, 0]
        cap = 12
        rc1, P1, i1, rows1, n1 = g.multiframe_align_raw(dev, X0, hold, edges, trace_capacity=cap)
        rc2, P2, i2, rows2, n2 = g.multiframe_align_raw(host, X0, hold, edges, trace_capacity=cap)
        assert rc1 == rc2 == 0 and n1 == n2 > 0 and i1.solves == i2.solves > 0
        assert np.array_equal(P1, P2) and not np.array_equal(P1, np.asarray(X0).reshape(-1))
        for k in range(n1):
            for name, _ in _capi.cvo_multiframe_trace_t._fields_:
                assert getattr(rows1[k], name) == getattr(rows2[k], name), (k, name)
    finally:
        g.close()


def test_refusals_and_their_messages_leave_the_context_usable(gpu):
    f = rc.frame("small")
    before = gpu.upload_rgbd(f, LEAF).pixel
    for field, value, text in (("rows", 0, "rows and cols"), ("cols", -1, "rows and cols"), ("channels", 2, "channels must be 1 or 3"),
                               ("image", None, "image is NULL"), ("depth", None, "depth is NULL"), ("depth_type", 5, "depth_type"),
                               ("fx", 0.0, "fx and fy"), ("fy", float("nan"), "fx and fy"), ("fx", float("inf"), "fx and fy"),
                               ("scaling_factor", -5000.0, "scaling_factor"), ("num_classes", 3, "semantic")):
        fs = f.c_struct()
        setattr(fs, field, value)
        px = np.full(2 * f.rows * f.cols, -7, np.int32)
        n = C.c_int(-7)
        h = C.c_void_p(0)
        ipp = C.POINTER(C.c_int)
        r = gpu.L.cvo_rgbd_points(gpu.ctx, C.byref(fs), FULL, px.ctypes.data_as(ipp), C.byref(n), None, None, None, None)
        assert r == _capi.CVO_E_INVALID and text in gpu.L.cvo_last_error(gpu.ctx).decode(), (field, gpu.L.cvo_last_error(gpu.ctx))
        r = gpu.L.cvo_cloud_upload_rgbd(gpu.ctx, C.byref(fs), 0.1, 4.0, C.byref(h), px.ctypes.data_as(ipp), None, C.byref(n))
        assert r == _capi.CVO_E_INVALID and text in gpu.L.cvo_last_error(gpu.ctx).decode(), field
        assert n.value == -7 and np.all(px == -7) and not h.value  # nothing written
    for leaf in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(CvoError, match="leaf"):
            gpu.upload_rgbd(f, leaf)
    for div in (0.0, -4.0, float("nan"), float("inf")):
        with pytest.raises(CvoError, match="edge_divisor"):
            gpu.upload_rgbd(f, 0.1, div)
    for method in (0, 5, 6):  # CV_FAST, CANNY_EDGES, EDGES_ONLY
        with pytest.raises(CvoError, match="error -5.*not supported"):
            gpu.rgbd_points(f, method)
    wide = RGBDFrame(np.zeros((36, 3210), np.uint8), np.ones((36, 3210), np.uint16), 500, 500, 1600, 18, 5000)
    with pytest.raises(CvoError, match="error -5.*threshold index"):
        gpu.upload_rgbd(wide, 0.1)
    # the voxel contract's refusals pass through: a depth that puts a point beyond |k| < 2^20 voxels
    far = RGBDFrame(f.image, np.full((f.rows, f.cols), 3.0e6, np.float32), f.fx, f.fy, f.cx, f.cy, 1.0)
    for route in (0, 1):
        gpu.set_option("RGBD_HOST", route)
        try:
            with pytest.raises(CvoError, match=r"point \d+: [xyz] = .*1048576"):
                gpu.upload_rgbd(far, 1.0)
        finally:
            gpu.set_option("RGBD_HOST", None)
    assert np.array_equal(gpu.upload_rgbd(f, LEAF).pixel, before)
