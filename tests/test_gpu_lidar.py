"""LiDAR front end on the MI355X: cvo_lidar_select / cvo_cloud_upload_lidar against the numpy statement (np_lidar.py), the CPU
twin and an ordinary upload of the statement's rows.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import cases
import lidar_cases as lc
import np_lidar
from unified_cvo_amd import CvoGPU, CvoPointCloud, CvoError, LidarRand, LidarScan, _capi

pytestmark = pytest.mark.gpu

HOST_BELOW = 12000  # scans with fewer points take the CPU twin unless LIDAR_HOST says otherwise
COUNTS = lc.COUNTS
_same_resident = lc.same_resident


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    yield g
    g.close()


@pytest.mark.parametrize("name", lc.CASES)
def test_kernels_equal_the_statement(gpu, name):
    """LIDAR_HOST=0: the kernels on every case, the small ones included; the intermediate counts are the statement's."""
    scan, cfg = lc.case(name)
    want = lc.statement(name)
    gpu.set_option("LIDAR_HOST", 0)
    try:
        rand, after = LidarRand(1), LidarRand(1)
        index, is_edge = gpu.lidar_select(scan, cfg, rand)
        assert np.array_equal(index, want["index"]) and np.array_equal(is_edge, want["is_edge"]), name
        st = gpu.debug_lidar_stats()
        assert st["on_device"] and {k: st[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, (name, st)
        for _ in range(want["draws"]):
            after.next()
        assert rand.state() == after.state(), name
        d = gpu.upload_lidar(scan, cfg, LidarRand(1))
        assert np.array_equal(d.pixel, want["index"])
        r = np_lidar.rows(scan.xyzi, want["index"], scan.semantic, scan.num_classes)
        _same_resident(gpu, d, CvoPointCloud.from_arrays(r["xyz"], r["feat"], r.get("label"), r["geotype"]))
        d.free()
    finally:
        gpu.set_option("LIDAR_HOST", None)


def test_routes_agree_and_repeats_are_identical(gpu):
    for name in ("room16", "semantic", "hdl64"):
        scan, cfg = lc.case(name)
        res = {}
        for route in (0, 1, None):
            gpu.set_option("LIDAR_HOST", route)
            try:
                rand = LidarRand(7)
                index, is_edge = gpu.lidar_select(scan, cfg, rand)
                assert gpu.debug_lidar_stats()["on_device"] == (route == 0 or (route is None and scan.n >= HOST_BELOW)), (name, route)
                d = gpu.upload_lidar(scan, cfg, rand)  # the second frame of a chain
                res[route] = [index, is_edge, d.pixel, d.debug_order(), np.array(rand.state()[0])]
                d.free()
            finally:
                gpu.set_option("LIDAR_HOST", None)
        for route in (1, None):
            for a, b in zip(res[0], res[route]):
                assert np.array_equal(a, b), (name, route)
    gpu.set_option("LIDAR_HOST", 0)
    try:
        for name in ("room16", "hdl64"):
            scan, cfg = lc.case(name)
            first = gpu.lidar_select(scan, cfg, LidarRand(1))
            for _ in range(10):
                again = gpu.lidar_select(scan, cfg, LidarRand(1))
                assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1]), name
    finally:
        gpu.set_option("LIDAR_HOST", None)


def test_refusals_and_their_messages_leave_the_context_usable(gpu):
    scan, cfg = lc.case("room16")
    gpu.set_option("LIDAR_HOST", 0)
    try:
        before = gpu.lidar_select(scan, cfg, LidarRand(1))[0]
        ipp = C.POINTER(C.c_int)

        def refused(s, c, code, text):
            rand = LidarRand(1)
            index, n = np.full(2 * scan.n, -7, np.int32), C.c_int(-7)
            calls = (lambda h: gpu.L.cvo_lidar_select(gpu.ctx, C.byref(s), C.byref(c), C.byref(rand.c), index.ctypes.data_as(ipp), None, C.byref(n)),
                     lambda h: gpu.L.cvo_cloud_upload_lidar(gpu.ctx, C.byref(s), C.byref(c), C.byref(rand.c), C.byref(h), index.ctypes.data_as(ipp), C.byref(n)))
            for call in calls:
                h = C.c_void_p(0)
                assert call(h) == code and text in gpu.L.cvo_last_error(gpu.ctx).decode(), (text, gpu.L.cvo_last_error(gpu.ctx))
                assert n.value == -7 and np.all(index == -7) and not h.value and rand.state() == LidarRand(1).state()  # nothing written, no draw

        for field, value, text in (("n_scan", 129, "n_scan"), ("horizon_scan", 4097, "horizon_scan"), ("ground_scan_ind", 16, "ground_scan_ind"),
                                   ("sensor_min_range", 0.0, "sensor_min_range"), ("segment_theta", 1.6, "segment_theta"),
                                   ("edge_threshold", 0.0, "edge_threshold"), ("distance_bound", -1.0, "distance_bound"), ("beam_num", 0, "beam_num")):
            bad = lc.small_config()
            setattr(bad.c, field, value)
            _capi.lib().cvo_lidar_config_derive(C.byref(bad.c))
            refused(scan.c_struct(), bad.c, _capi.CVO_E_INVALID, text)
        stale = lc.small_config()
        stale.c.segment_theta = 0.9
        refused(scan.c_struct(), stale.c, _capi.CVO_E_INVALID, "derived fields")
        for field, value, text in (("xyzi", None, "xyzi is NULL"), ("n", 0, "n must be"), ("num_classes", 2, "semantic")):
            s = scan.c_struct()
            setattr(s, field, value)
            refused(s, cfg.c, _capi.CVO_E_INVALID, text)
        rand, index, n = LidarRand(1), np.full(2 * scan.n, -7, np.int32), C.c_int(-7)
        s = scan.c_struct()
        for args, text in (((None, C.byref(cfg.c), C.byref(rand.c)), "scan is NULL"), ((C.byref(s), None, C.byref(rand.c)), "config is NULL"),
                           ((C.byref(s), C.byref(cfg.c), None), "rand is NULL")):
            h = C.c_void_p(0)
            for rc in (gpu.L.cvo_lidar_select(gpu.ctx, *args, index.ctypes.data_as(ipp), None, C.byref(n)),
                       gpu.L.cvo_cloud_upload_lidar(gpu.ctx, *args, C.byref(h), index.ctypes.data_as(ipp), C.byref(n))):
                assert rc == _capi.CVO_E_INVALID and text in gpu.L.cvo_last_error(gpu.ctx).decode(), text
            assert n.value == -7 and np.all(index == -7) and not h.value and rand.state() == LidarRand(1).state()
        rc = gpu.L.cvo_lidar_select(gpu.ctx, C.byref(s), C.byref(cfg.c), C.byref(rand.c), None, None, C.byref(n))
        assert rc == _capi.CVO_E_INVALID and "index and n are required" in gpu.L.cvo_last_error(gpu.ctx).decode() and rand.state() == LidarRand(1).state()
        h = C.c_void_p(0)
        rc = gpu.L.cvo_cloud_upload_lidar(gpu.ctx, C.byref(s), C.byref(cfg.c), C.byref(rand.c), None, index.ctypes.data_as(ipp), C.byref(n))
        assert rc == _capi.CVO_E_INVALID and "out is NULL" in gpu.L.cvo_last_error(gpu.ctx).decode() and n.value == -7
        unseeded = LidarRand(1)
        unseeded.c.front = 31
        refused_rand = gpu.L.cvo_lidar_select(gpu.ctx, C.byref(s), C.byref(cfg.c), C.byref(unseeded.c), index.ctypes.data_as(ipp), None, C.byref(n))
        assert refused_rand == _capi.CVO_E_INVALID and "not seeded" in gpu.L.cvo_last_error(gpu.ctx).decode() and np.all(index == -7)
        labels = np.zeros(scan.n, np.int32)
        labels[5] = 3
        refused(LidarScan(scan.xyzi, labels, 3).c_struct(), cfg.c, _capi.CVO_E_INVALID, "semantic[5]")
        nan = LidarScan(scan.xyzi.copy())
        nan.xyzi[100, 2] = np.nan
        refused(nan.c_struct(), cfg.c, _capi.CVO_E_INVALID, "non-finite")
        big = scan.c_struct()
        big.n = (1 << 24) + 1
        refused(big, cfg.c, _capi.CVO_E_UNSUPPORTED, "2^24")
        with pytest.raises(CvoError, match="error -2.*non-finite"):
            gpu.lidar_select(nan, cfg, LidarRand(1))
        assert np.array_equal(gpu.lidar_select(scan, cfg, LidarRand(1))[0], before)
    finally:
        gpu.set_option("LIDAR_HOST", None)
