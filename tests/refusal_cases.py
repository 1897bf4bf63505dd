"""Deliberately bad calls of the front ends' entry points, through ctypes: one case per refusal branch, the two-fault cases
that pin the order in which competing refusals win, and the calls of the stats-survival check.  Shared by
scripts/make_refusal_golden.py (which records what the library answers: tests/golden/frontend_refusals.json) and by
test_frontend_refusals.py / test_gpu_frontend_refusals.py (which replay the cases against the record, exactly).

A case is (name, entry point, needs a context, arguments after the context).  Frames are 8 x 8, the cloud has 16 points, the
scan is the smallest of lidar_cases.py; a size fault names a size only, every pointer stays at its small array: each refusal
here comes before anything is read or launched."""
import collections
import ctypes as C
import math

import numpy as np

import lidar_cases
import sgm_cases
from unified_cvo_amd import _capi

Case = collections.namedtuple("Case", "name fn ctx args")

NAN, INF = float("nan"), float("inf")
CV_FAST, DSO, FULL = _capi.CVO_SELECT_CV_FAST, _capi.CVO_SELECT_DSO_EDGES, _capi.CVO_SELECT_FULL
R = 8  # the frames' side

_rng = np.random.default_rng(7)
IMG1 = _rng.integers(0, 256, (R, R), dtype=np.uint8)
IMG3 = _rng.integers(0, 256, (R, R, 3), dtype=np.uint8)
RIGHT = _rng.integers(0, 256, (R, R), dtype=np.uint8)
DEPTH = np.full((R, R), 2.0, np.float32)
DISP = np.full((R, R), 3.0, np.float32)
XYZ = _rng.uniform(-1, 1, (16, 3)).astype(np.float32)
XYZ_NAN, XYZ_FAR = XYZ.copy(), XYZ.copy()
XYZ_NAN[3, 1] = NAN
XYZ_FAR[5, 2] = 1e9
MAP_NAN, MAP_NEAR = DISP.copy(), DISP.copy()
MAP_NAN[2, 2] = INF
MAP_NEAR[1, 1] = -0.5  # negative, but not below -speckle_sim_threshold = -1
SCAN, SCAN_CFG = lidar_cases.case("n1")
SCAN_NAN, SCAN_INTENSITY, SCAN_HUGE = (SCAN.xyzi.copy() for _ in range(3))
SCAN_NAN[0, 0] = NAN
SCAN_INTENSITY[0, 3] = INF
SCAN_HUGE[0, 2] = 1e15
SCAN_SEM = np.array([5], np.int32)

# outputs no refused call writes
_PIX, _EDGE = np.zeros(4 * R * R, np.int32), np.zeros(4 * R * R, np.uint8)
_F = np.zeros(16 * R * R, np.float32)
_N, _T, _CLOUD = C.c_int(), C.c_int(), C.c_void_p()
_OUT8 = np.zeros((R, R), np.float32)

ipp, fpp, bpp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
pix, edge, fout = _PIX.ctypes.data_as(ipp), _EDGE.ctypes.data_as(bpp), _F.ctypes.data_as(fpp)
n_out, t_out, cloud = C.byref(_N), C.byref(_T), C.byref(_CLOUD)


def _u8(a):
    return a.ctypes.data_as(bpp)


def _f32(a):
    return a.ctypes.data_as(fpp)


def rgbd(**kw):
    f = dict(rows=R, cols=R, channels=1, image=IMG1.ctypes.data, gray=None, depth=DEPTH.ctypes.data, depth_type=_capi.CVO_DEPTH_F32,
             fx=50.0, fy=50.0, cx=4.0, cy=4.0, scaling_factor=1.0, num_classes=0, semantic=None)
    f.update(kw)
    return C.byref(_capi.cvo_rgbd_frame_t(**f))


def stereo(**kw):
    f = dict(rows=R, cols=R, channels=1, image=IMG1.ctypes.data, gray=None, disparity=DISP.ctypes.data, fx=50.0, fy=50.0, cx=4.0, cy=4.0,
             baseline=0.5, num_classes=0, semantic=None)
    f.update(kw)
    return C.byref(_capi.cvo_stereo_frame_t(**f))


def schedule(*v):
    return C.byref(_capi.cvo_fast_schedule_t(*(v or _capi.CVO_FAST_STEREO)))


def sgm(**kw):
    f = dict(max_disparity=64, p1=10, p2=120, uniqueness=5, lr_max_diff=1, paths=8)
    f.update(kw)
    return C.byref(_capi.cvo_sgm_config_t(**f))


def dfilter(**kw):
    f = dict(speckle_sim_threshold=1.0, speckle_size=200, ipol_gap_width=3, adaptive_mean=1)
    f.update(kw)
    return C.byref(_capi.cvo_dfilter_config_t(**f))


def scan(**kw):
    f = dict(n=SCAN.n, xyzi=SCAN.xyzi.ctypes.data, semantic=None, num_classes=0)
    f.update(kw)
    return C.byref(_capi.cvo_lidar_scan_t(**f))


def lidar_config(derive=True, **kw):
    c = _capi.cvo_lidar_config_t.from_buffer_copy(SCAN_CFG.c)
    for k, v in kw.items():
        setattr(c, k, v)
    if derive:
        _capi.lib().cvo_lidar_config_derive(C.byref(c))
    return C.byref(c)


def lidar_rand(front=None):
    r = _capi.cvo_lidar_rand_t()
    _capi.lib().cvo_lidar_rand_seed(C.byref(r), 1)
    if front is not None:
        r.front = front
    return C.byref(r)


BIG = 4097  # BIG x BIG: one row and one column above 2^24 pixels
WIDE = 10000  # 8 x WIDE: the DSO selector's threshold index leaves its table

# (what, overrides) of a frame the RGB-D and the stereo front end refuse alike, in the order of frame_validate
FRAME_FAULTS = [("rows 0", dict(rows=0)), ("cols -1", dict(cols=-1)), ("channels 2", dict(channels=2)), ("image NULL", dict(image=None)),
                ("classes without semantic", dict(num_classes=3)), ("classes -1", dict(num_classes=-1)), ("2^24 pixels", dict(rows=BIG, cols=BIG))]
RGBD_FAULTS = FRAME_FAULTS + [("depth NULL", dict(depth=None)), ("depth_type 7", dict(depth_type=7)), ("fx 0", dict(fx=0.0)), ("fy inf", dict(fy=INF)),
                              ("fx -1", dict(fx=-1.0)), ("scaling_factor 0", dict(scaling_factor=0.0)), ("scaling_factor nan", dict(scaling_factor=NAN)),
                              ("depth NULL and classes -1", dict(depth=None, num_classes=-1)), ("image NULL and fx 0", dict(image=None, fx=0.0))]
STEREO_FAULTS = FRAME_FAULTS + [("disparity NULL", dict(disparity=None)), ("fx 0", dict(fx=0.0)), ("fy inf", dict(fy=INF)), ("fy nan", dict(fy=NAN)),
                                ("baseline 0", dict(baseline=0.0)), ("baseline nan", dict(baseline=NAN)),
                                ("disparity NULL and classes -1", dict(disparity=None, num_classes=-1)), ("image NULL and fx 0", dict(image=None, fx=0.0))]
SGM_FAULTS = [("D 100", dict(max_disparity=100)), ("p1 -1", dict(p1=-1)), ("p1 above p2", dict(p1=121)), ("p2 194", dict(p2=194)),
              ("uniqueness -1", dict(uniqueness=-1)), ("uniqueness 100", dict(uniqueness=100)), ("paths 5", dict(paths=5)),
              ("D 100 and paths 5", dict(max_disparity=100, paths=5))]
DFILTER_FAULTS = [("sim nan", dict(speckle_sim_threshold=NAN)), ("sim -1", dict(speckle_sim_threshold=-1.0)), ("speckle_size -1", dict(speckle_size=-1)),
                  ("gap -1", dict(ipol_gap_width=-1)), ("sim nan and gap -1", dict(speckle_sim_threshold=NAN, ipol_gap_width=-1))]
LIDAR_CONFIG_FAULTS = [
    ("n_scan 0", dict(n_scan=0)), ("n_scan 129", dict(n_scan=129)), ("horizon_scan 0", dict(horizon_scan=0)), ("horizon_scan 4097", dict(horizon_scan=4097)),
    ("ground_scan_ind -1", dict(ground_scan_ind=-1)), ("ground_scan_ind n_scan", dict(ground_scan_ind=16)), ("ang_res_x 0", dict(ang_res_x=0.0)),
    ("ang_res_x nan", dict(ang_res_x=NAN)), ("sensor_min_range 0", dict(sensor_min_range=0.0)), ("mount 50", dict(sensor_mount_angle=50.0)),
    ("mount nan", dict(sensor_mount_angle=NAN)), ("theta 0", dict(segment_theta=0.0)), ("theta 2", dict(segment_theta=2.0)),
    ("alpha_x 0", dict(segment_alpha_x=0.0)), ("alpha_y 2", dict(segment_alpha_y=2.0)), ("valid_point_num 0", dict(segment_valid_point_num=0)),
    ("valid_line_num 0", dict(segment_valid_line_num=0)), ("edge_threshold 0", dict(edge_threshold=0.0)), ("surf_threshold nan", dict(surf_threshold=NAN)),
    ("intensity_bound 0", dict(intensity_bound=0.0)), ("depth_bound inf", dict(depth_bound=INF)), ("distance_bound -1", dict(distance_bound=-1.0)),
    ("beam_num 0", dict(beam_num=0)), ("n_scan 0 and beam_num 0", dict(n_scan=0, beam_num=0))]


def _voxel(add):
    xyz, kept = _f32(XYZ), pix
    for fn, ctx in (("cvo_voxel_select_host", False), ("cvo_voxel_select", True)):
        for what, a in [("n -1", (-1, xyz, 0.1, kept, n_out)), ("xyz NULL", (16, None, 0.1, kept, n_out)), ("kept NULL", (16, xyz, 0.1, None, n_out)),
                        ("n_kept NULL", (16, xyz, 0.1, kept, None)), ("n 0 n_kept NULL", (0, None, 0.1, None, None)),
                        ("2^24 points", ((1 << 24) + 1, xyz, 0.1, kept, n_out)), ("size 0", (16, xyz, 0.0, kept, n_out)), ("size nan", (16, xyz, NAN, kept, n_out)),
                        ("size -1", (16, xyz, -1.0, kept, n_out)), ("n 0 size 0", (0, None, 0.0, None, n_out)), ("point nan", (16, _f32(XYZ_NAN), 0.1, kept, n_out)),
                        ("point outside the grid", (16, _f32(XYZ_FAR), 0.1, kept, n_out)), ("2^24 points and size 0", ((1 << 24) + 1, xyz, 0.0, kept, n_out)),
                        ("xyz NULL and size 0", (16, None, 0.0, kept, n_out)), ("point nan and size nan", (16, _f32(XYZ_NAN), NAN, kept, n_out))]:
            add(fn, ctx, what, a)
    for what, a in [("out NULL", (16, xyz, None, None, None, 0.1, None, kept, n_out)), ("n -1", (-1, xyz, None, None, None, 0.1, cloud, kept, n_out)),
                    ("xyz NULL", (16, None, None, None, None, 0.1, cloud, kept, n_out)), ("2^24 points", ((1 << 24) + 1, xyz, None, None, None, 0.1, cloud, kept, n_out)),
                    ("size 0", (16, xyz, None, None, None, 0.0, cloud, kept, n_out)), ("size inf", (16, xyz, None, None, None, INF, cloud, kept, n_out)),
                    ("point nan", (16, _f32(XYZ_NAN), None, None, None, 0.1, cloud, kept, n_out)),
                    ("point outside the grid", (16, _f32(XYZ_FAR), None, None, None, 0.1, cloud, kept, n_out)),
                    ("out NULL and size 0", (16, xyz, None, None, None, 0.0, None, kept, n_out))]:
        add("cvo_cloud_upload_voxel", True, what, a)


def _rgbd(add):
    for fn, ctx in (("cvo_rgbd_points_host", False), ("cvo_rgbd_points", True)):
        tail = (fout, fout, None, fout)
        add(fn, ctx, "frame NULL", (None, FULL, pix, n_out) + tail)
        for what, kw in RGBD_FAULTS:
            add(fn, ctx, what, (rgbd(**kw), FULL, pix, n_out) + tail)
        for what, method in [("method CV_FAST", CV_FAST), ("method 5", 5), ("method 99", 99), ("method -1", -1)]:
            add(fn, ctx, what, (rgbd(), method, pix, n_out) + tail)
        add(fn, ctx, "threshold index", (rgbd(cols=WIDE), DSO, pix, n_out) + tail)
        add(fn, ctx, "threshold index is DSO's alone", (rgbd(cols=WIDE), FULL, None, n_out) + tail)
        add(fn, ctx, "pixel NULL", (rgbd(), FULL, None, n_out) + tail)
        add(fn, ctx, "n NULL", (rgbd(), DSO, pix, None) + tail)
        add(fn, ctx, "fx 0 and method 99", (rgbd(fx=0.0), 99, pix, n_out) + tail)
        add(fn, ctx, "method 99 and pixel NULL", (rgbd(), 99, None, n_out) + tail)
    fn = "cvo_cloud_upload_rgbd"
    add(fn, True, "frame NULL", (None, 0.1, 4.0, cloud, pix, edge, n_out))
    for what, kw in RGBD_FAULTS:
        add(fn, True, what, (rgbd(**kw), 0.1, 4.0, cloud, pix, edge, n_out))
    for what, a in [("threshold index", (rgbd(cols=WIDE), 0.1, 4.0, cloud)), ("out NULL", (rgbd(), 0.1, 4.0, None)), ("leaf 0", (rgbd(), 0.0, 4.0, cloud)),
                    ("leaf nan", (rgbd(), NAN, 4.0, cloud)), ("divisor 0", (rgbd(), 0.1, 0.0, cloud)), ("divisor inf", (rgbd(), 0.1, INF, cloud)),
                    ("leaf over divisor 0", (rgbd(), 1e-30, 1e30, cloud)), ("out NULL and leaf 0", (rgbd(), 0.0, 4.0, None)),
                    ("leaf 0 and divisor 0", (rgbd(), 0.0, 0.0, cloud)), ("fx 0 and out NULL", (rgbd(fx=0.0), 0.1, 4.0, None))]:
        add(fn, True, what, a + (pix, edge, n_out))


def _fast(add):
    gray = _u8(IMG1)
    for fn, ctx in (("cvo_fast_select_host", False), ("cvo_fast_select", True)):
        for what, a in [("rows 0", (0, R, gray, schedule(), pix, n_out)), ("cols 0", (R, 0, gray, schedule(), pix, n_out)), ("gray NULL", (R, R, None, schedule(), pix, n_out)),
                        ("2^24 pixels", (BIG, BIG, gray, schedule(), pix, n_out)), ("schedule NULL", (R, R, gray, None, pix, n_out)),
                        ("thresh -1", (R, R, gray, schedule(-1, 100, 10, 50), pix, n_out)), ("thresh 256", (R, R, gray, schedule(256, 100, 10, 50), pix, n_out)),
                        ("num_want -1", (R, R, gray, schedule(4, -1, -2, 50), pix, n_out)), ("num_min -1", (R, R, gray, schedule(4, 100, -1, 50), pix, n_out)),
                        ("num_min above num_want", (R, R, gray, schedule(4, 10, 11, 50), pix, n_out)), ("break_thresh -1", (R, R, gray, schedule(4, 100, 10, -1), pix, n_out)),
                        ("pixel NULL", (R, R, gray, schedule(), None, n_out)), ("n NULL", (R, R, gray, schedule(), pix, None)),
                        ("gray NULL and schedule NULL", (R, R, None, None, pix, n_out)), ("schedule NULL and pixel NULL", (R, R, gray, None, None, n_out))]:
            add(fn, ctx, what, a + (t_out,))


def _stereo(add):
    tail = (fout, fout, None, fout)
    methods = [("method 5", 5), ("method 99", 99), ("method -1", -1)]
    for fn, ctx in (("cvo_stereo_points_host", False), ("cvo_stereo_points", True)):
        add(fn, ctx, "frame NULL", (None, FULL, pix, n_out) + tail)
        for what, kw in STEREO_FAULTS:
            add(fn, ctx, what, (stereo(**kw), FULL, pix, n_out) + tail)
        for what, method in methods:
            add(fn, ctx, what, (stereo(), method, pix, n_out) + tail)
        add(fn, ctx, "threshold index", (stereo(cols=WIDE), DSO, pix, n_out) + tail)
        add(fn, ctx, "threshold index is DSO's alone", (stereo(cols=WIDE), CV_FAST, None, n_out) + tail)
        add(fn, ctx, "pixel NULL", (stereo(), FULL, None, n_out) + tail)
        add(fn, ctx, "n NULL", (stereo(), CV_FAST, pix, None) + tail)
        add(fn, ctx, "fx 0 and method 99", (stereo(fx=0.0), 99, pix, n_out) + tail)
        add(fn, ctx, "method 99 and pixel NULL", (stereo(), 99, None, n_out) + tail)
    fn = "cvo_cloud_upload_stereo"
    add(fn, True, "frame NULL", (None, FULL, cloud, pix, n_out))
    for what, kw in STEREO_FAULTS:
        add(fn, True, what, (stereo(**kw), FULL, cloud, pix, n_out))
    for what, method in methods:
        add(fn, True, what, (stereo(), method, cloud, pix, n_out))
    add(fn, True, "threshold index", (stereo(cols=WIDE), DSO, cloud, pix, n_out))
    add(fn, True, "out NULL", (stereo(), FULL, None, pix, n_out))
    add(fn, True, "method 99 and out NULL", (stereo(), 99, None, pix, n_out))
    fn = "cvo_cloud_upload_stereo_recipe"
    add(fn, True, "frame NULL", (None, 0.1, 5.0, cloud, pix, edge, n_out))
    for what, kw in STEREO_FAULTS:
        add(fn, True, what, (stereo(**kw), 0.1, 5.0, cloud, pix, edge, n_out))
    for what, a in [("threshold index", (stereo(cols=WIDE), 0.1, 5.0, cloud)), ("out NULL", (stereo(), 0.1, 5.0, None)), ("leaf 0", (stereo(), 0.0, 5.0, cloud)),
                    ("leaf inf", (stereo(), INF, 5.0, cloud)), ("divisor 0", (stereo(), 0.1, 0.0, cloud)), ("divisor nan", (stereo(), 0.1, NAN, cloud)),
                    ("leaf over divisor 0", (stereo(), 1e-30, 1e30, cloud)), ("out NULL and leaf 0", (stereo(), 0.0, 5.0, None)),
                    ("leaf 0 and divisor 0", (stereo(), 0.0, 0.0, cloud))]:
        add(fn, True, what, a + (pix, edge, n_out))


def _lidar(add):
    entries = [("cvo_lidar_select_host", False, lambda *a: a + (pix, edge, n_out)), ("cvo_lidar_select", True, lambda *a: a + (pix, edge, n_out)),
               ("cvo_cloud_upload_lidar", True, lambda *a: a + (cloud, pix, n_out))]
    for fn, ctx, full in entries:
        add(fn, ctx, "scan NULL", full(None, lidar_config(), lidar_rand()))
        add(fn, ctx, "config NULL", full(scan(), None, lidar_rand()))
        add(fn, ctx, "rand NULL", full(scan(), lidar_config(), None))
        add(fn, ctx, "scan NULL and config NULL", full(None, None, lidar_rand()))
        for what, kw in [("xyzi NULL", dict(xyzi=None)), ("n 0", dict(n=0)), ("classes -1", dict(num_classes=-1)), ("classes without semantic", dict(num_classes=2)),
                         ("semantic without classes", dict(semantic=SCAN_SEM.ctypes.data)), ("2^24 points", dict(n=(1 << 24) + 1)),
                         ("point nan", dict(xyzi=SCAN_NAN.ctypes.data)), ("intensity inf", dict(xyzi=SCAN_INTENSITY.ctypes.data)),
                         ("point 1e15", dict(xyzi=SCAN_HUGE.ctypes.data)), ("semantic outside", dict(semantic=SCAN_SEM.ctypes.data, num_classes=5)),
                         ("xyzi NULL and n 0", dict(xyzi=None, n=0))]:
            add(fn, ctx, what, full(scan(**kw), lidar_config(), lidar_rand()))
        add(fn, ctx, "rand not seeded", full(scan(), lidar_config(), lidar_rand(front=31)))
        add(fn, ctx, "rand not seeded and n_scan 0", full(scan(), lidar_config(n_scan=0), lidar_rand(front=31)))
        for what, kw in LIDAR_CONFIG_FAULTS:
            add(fn, ctx, what, full(scan(), lidar_config(**kw), lidar_rand()))
        add(fn, ctx, "derived fields", full(scan(), lidar_config(derive=False, segment_theta=0.5), lidar_rand()))
        add(fn, ctx, "2^24 points and n_scan 0", full(scan(n=(1 << 24) + 1), lidar_config(n_scan=0), lidar_rand()))
    add("cvo_lidar_select_host", False, "index NULL", (scan(), lidar_config(), lidar_rand(), None, edge, n_out))
    add("cvo_lidar_select_host", False, "n NULL", (scan(), lidar_config(), lidar_rand(), pix, edge, None))
    add("cvo_lidar_select_host", False, "n_scan 0 and index NULL", (scan(), lidar_config(n_scan=0), lidar_rand(), None, edge, n_out))
    add("cvo_lidar_select", True, "index NULL", (scan(), lidar_config(), lidar_rand(), None, edge, n_out))
    add("cvo_lidar_select", True, "n NULL", (scan(), lidar_config(), lidar_rand(), pix, edge, None))
    add("cvo_lidar_select", True, "n_scan 0 and index NULL", (scan(), lidar_config(n_scan=0), lidar_rand(), None, edge, n_out))
    add("cvo_cloud_upload_lidar", True, "out NULL", (scan(), lidar_config(), lidar_rand(), None, pix, n_out))
    add("cvo_cloud_upload_lidar", True, "n_scan 0 and out NULL", (scan(), lidar_config(n_scan=0), lidar_rand(), None, pix, n_out))


def _matcher(add):
    left, right, out = _u8(IMG1), _u8(RIGHT), _f32(_OUT8)
    sizes = [("rows 0", 0, R, {}), ("cols 0", R, 0, {}), ("2^24 pixels", BIG, BIG, {}), ("2 GiB of sums", 4096, 4096, dict(max_disparity=128)),
             ("rows 0 and D 100", 0, R, dict(max_disparity=100)), ("2^24 pixels and paths 5", BIG, BIG, dict(paths=5))]
    for fn, ctx, extra in (("cvo_stereo_disparity_host", False, ()), ("cvo_stereo_disparity", True, ()), ("cvo_stereo_disparity_filtered", True, (dfilter(),))):
        for what, a in [("left NULL", (R, R, None, right, sgm()) + extra + (out,)), ("right NULL", (R, R, left, None, sgm()) + extra + (out,)),
                        ("config NULL", (R, R, left, right, None) + extra + (out,)), ("disparity NULL", (R, R, left, right, sgm()) + extra + (None,)),
                        ("left NULL and rows 0", (0, R, None, right, sgm()) + extra + (out,))]:
            add(fn, ctx, what, a)
        for what, rows, cols, kw in sizes:
            add(fn, ctx, what, (rows, cols, left, right, sgm(**kw)) + extra + (out,))
        for what, kw in SGM_FAULTS:
            add(fn, ctx, what, (R, R, left, right, sgm(**kw)) + extra + (out,))
    fn = "cvo_stereo_disparity_filtered"
    add(fn, True, "filter config NULL", (R, R, left, right, sgm(), None, out))
    for what, kw in DFILTER_FAULTS + [("marker not below -sim", dict(speckle_sim_threshold=10.0))]:
        add(fn, True, "filter " + what, (R, R, left, right, sgm(), dfilter(**kw), out))
    add(fn, True, "D 100 and filter sim nan", (R, R, left, right, sgm(max_disparity=100), dfilter(speckle_sim_threshold=NAN), out))
    add(fn, True, "disparity NULL and filter config NULL", (R, R, left, right, sgm(), None, None))
    add(fn, True, "2 GiB of sums and filter gap -1", (4096, 4096, left, right, sgm(max_disparity=128), dfilter(ipol_gap_width=-1), out))


def _filter(add):
    m, out = _f32(DISP), _f32(_OUT8)
    for fn, ctx in (("cvo_disparity_filter_host", False), ("cvo_disparity_filter", True)):
        for what, a in [("in NULL", (R, R, None, dfilter(), out)), ("out NULL", (R, R, m, dfilter(), None)), ("config NULL", (R, R, m, None, out)),
                        ("rows 0", (0, R, m, dfilter(), out)), ("cols -1", (R, -1, m, dfilter(), out)), ("2^24 pixels", (BIG, BIG, m, dfilter(), out)),
                        ("map inf", (R, R, _f32(MAP_NAN), dfilter(), out)), ("map negative within sim", (R, R, _f32(MAP_NEAR), dfilter(), out)),
                        ("in NULL and config NULL", (R, R, None, None, out)), ("2^24 pixels and sim nan", (BIG, BIG, m, dfilter(speckle_sim_threshold=NAN), out)),
                        ("map inf and gap -1", (R, R, _f32(MAP_NAN), dfilter(ipol_gap_width=-1), out))]:
            add(fn, ctx, what, a)
        for what, kw in DFILTER_FAULTS:
            add(fn, ctx, what, (R, R, m, dfilter(**kw), out))


def _pair(add):
    right = _u8(RIGHT)
    bad_sgm, bad_filter = dict(max_disparity=100), dict(speckle_sim_threshold=NAN)
    for fn, filtered in (("cvo_cloud_upload_stereo_pair", False), ("cvo_cloud_upload_stereo_pair_filtered", True)):
        def call(frame, r=right, cfg=None, flt=None, method=FULL, out=cloud, sgm_null=False, flt_null=False):
            a = (frame, r, None if sgm_null else sgm(**(cfg or {})))
            if filtered:
                a += (None if flt_null else dfilter(**(flt or {})),)
            return a + (method, out, pix, n_out)

        add(fn, True, "frame NULL", call(None))
        add(fn, True, "out NULL", call(stereo(disparity=None), out=None))
        add(fn, True, "right NULL", call(stereo(disparity=None), r=None))
        add(fn, True, "matcher config NULL", call(stereo(disparity=None), sgm_null=True))
        add(fn, True, "image NULL", call(stereo(disparity=None, image=None)))
        add(fn, True, "image NULL with a gray plane", call(stereo(disparity=None, image=None, gray=IMG1.ctypes.data)))
        for what, kw in [("rows 0", dict(rows=0)), ("cols 0", dict(cols=0)), ("2^24 pixels", dict(rows=BIG, cols=BIG))]:
            add(fn, True, what, call(stereo(disparity=None, **kw)))
        add(fn, True, "2 GiB of sums", call(stereo(disparity=None, rows=4096, cols=4096), cfg=dict(max_disparity=128)))
        for what, kw in SGM_FAULTS:
            add(fn, True, "matcher " + what, call(stereo(disparity=None), cfg=kw))
        # the front end's refusals (the matcher is content): the frame's disparity pointer is not looked at
        for what, kw in [("channels 2", dict(channels=2)), ("fx 0", dict(fx=0.0)), ("fy nan", dict(fy=NAN)), ("baseline 0", dict(baseline=0.0)),
                         ("classes without semantic", dict(num_classes=3)), ("classes -1", dict(num_classes=-1))]:
            add(fn, True, what, call(stereo(disparity=None, **kw)))
        add(fn, True, "fx 0 with a disparity", call(stereo(fx=0.0)))
        for what, method in [("method 5", 5), ("method 99", 99), ("method -1", -1)]:
            add(fn, True, what, call(stereo(disparity=None), method=method))
        add(fn, True, "threshold index", call(stereo(disparity=None, cols=WIDE), method=DSO))
        # two faults: which one is reported
        add(fn, True, "bad matcher config and fx 0", call(stereo(disparity=None, fx=0.0), cfg=bad_sgm))
        add(fn, True, "bad matcher config and method 99", call(stereo(disparity=None), cfg=bad_sgm, method=99))
        add(fn, True, "frame NULL and bad matcher config", call(None, cfg=bad_sgm))
        add(fn, True, "out NULL and bad matcher config", call(stereo(disparity=None), cfg=bad_sgm, out=None))
        add(fn, True, "out NULL and fx 0", call(stereo(disparity=None, fx=0.0), out=None))
        add(fn, True, "right NULL and channels 2", call(stereo(disparity=None, channels=2), r=None))
        if not filtered:
            continue
        add(fn, True, "filter config NULL", call(stereo(disparity=None), flt_null=True))
        for what, kw in DFILTER_FAULTS + [("marker not below -sim", dict(speckle_sim_threshold=10.0))]:
            add(fn, True, "filter " + what, call(stereo(disparity=None), flt=kw))
        add(fn, True, "bad matcher config and bad filter config", call(stereo(disparity=None), cfg=bad_sgm, flt=bad_filter))
        add(fn, True, "bad filter config and fx 0", call(stereo(disparity=None, fx=0.0), flt=bad_filter))
        add(fn, True, "bad filter config and method 99", call(stereo(disparity=None), flt=bad_filter, method=99))
        add(fn, True, "filter config NULL and fx 0", call(stereo(disparity=None, fx=0.0), flt_null=True))
        add(fn, True, "frame NULL and bad filter config", call(None, flt=bad_filter))
        add(fn, True, "out NULL and bad filter config", call(stereo(disparity=None), flt=bad_filter, out=None))
        add(fn, True, "out NULL and both configs bad", call(stereo(disparity=None), cfg=bad_sgm, flt=bad_filter, out=None))
        add(fn, True, "2 GiB of sums and bad filter config", call(stereo(disparity=None, rows=4096, cols=4096), cfg=dict(max_disparity=128), flt=bad_filter))


def cases():
    """Every case, in a fixed order; names are unique.  Each context entry point also gets the call without a context."""
    out, seen = [], set()

    def add(fn, ctx, what, args):
        name = f"{fn}: {what}"
        assert name not in seen, name
        seen.add(name)
        out.append(Case(name, fn, ctx, tuple(args)))

    for part in (_voxel, _rgbd, _fast, _stereo, _lidar, _matcher, _filter, _pair):
        part(add)
    # without a context: the bare code, nothing to store a message in (the arguments are another case's, all bad or all good)
    first = {}
    for c in out:
        if c.ctx:
            first.setdefault(c.fn, c)
    return out + [Case(f"{fn}: context NULL", fn, False, (None,) + c.args) for fn, c in first.items()]


def run(L, ctx, case):
    """-> {"rc", "error"}: the code and - with a context - what cvo_last_error holds afterwards.  Before a context case a
    refusal of another front end (the denoiser's, which no case calls) is stored, so that a refusal which stores no message
    of its own cannot pass for one that does."""
    if not case.ctx:
        return dict(rc=int(getattr(L, case.fn)(*case.args)), error=None)
    assert L.cvo_nlm_denoise(ctx, 0, 0, 0, None, None, None) != 0
    rc = int(getattr(L, case.fn)(ctx, *case.args))
    return dict(rc=rc, error=L.cvo_last_error(ctx).decode())


# ---- stats survival: a successful pair call on a 16 x 24 frame, then refused calls; the three stats stay ----
SURVIVAL_ROWS, SURVIVAL_COLS = 16, 24
SURVIVAL_REFUSED = ("cvo_cloud_upload_stereo_pair_filtered: fx 0", "cvo_cloud_upload_stereo_pair_filtered: filter sim nan",
                    "cvo_cloud_upload_stereo_pair: matcher D 100", "cvo_cloud_upload_stereo_pair: method 99", "cvo_stereo_disparity_filtered: filter gap -1",
                    "cvo_stereo_disparity: paths 5", "cvo_disparity_filter: map inf", "cvo_cloud_upload_stereo: method 99", "cvo_stereo_points: fx 0",
                    "cvo_fast_select: schedule NULL", "cvo_cloud_upload_stereo_recipe: leaf over divisor 0")


def stats(L, ctx):
    """what cvo_debug_sgm_stats, cvo_debug_dfilter_stats and cvo_debug_stereo_stats report, as plain lists"""
    i = [C.c_int() for _ in range(8)]
    lines = (C.c_int * 8)()
    assert L.cvo_debug_sgm_stats(ctx, C.byref(i[0]), C.byref(i[1]), C.byref(i[2]), lines, *(C.byref(v) for v in i[3:7])) == 0
    out = dict(sgm=[v.value for v in i[:7]] + list(lines))
    counts = (C.c_ulonglong * 3)()
    assert L.cvo_debug_dfilter_stats(ctx, *(C.byref(v) for v in i[:5]), counts, None, None, None) == 0
    out["dfilter"] = [v.value for v in i[:5]] + list(counts)
    tried, count, hist = (C.c_int * 64)(), (C.c_int * 64)(), (C.c_uint * 257)()
    cand, kept = C.c_ulonglong(), C.c_ulonglong()
    assert L.cvo_debug_stereo_stats(ctx, 64, C.byref(i[0]), tried, count, C.byref(i[1]), hist, C.byref(cand), C.byref(kept), C.byref(i[2])) == 0
    k = min(i[0].value, 64)
    out["stereo"] = [i[0].value, i[1].value, i[2].value, cand.value, kept.value] + list(tried[:k]) + list(count[:k]) + list(hist)
    return out


def survival(L, ctx):
    """-> {"after_success", "after_refusals"}: the stats after the pair call that succeeds and after the refused calls behind it"""
    left, right, _ = sgm_cases.two_planes(SURVIVAL_ROWS, SURVIVAL_COLS, 3, d_top=2, d_bottom=5)
    left = np.ascontiguousarray(left)
    frame = _capi.cvo_stereo_frame_t(rows=SURVIVAL_ROWS, cols=SURVIVAL_COLS, channels=1, image=left.ctypes.data, gray=None, disparity=None, fx=50.0, fy=50.0,
                                     cx=12.0, cy=8.0, baseline=0.5, num_classes=0, semantic=None)
    h = C.c_void_p()
    keep = np.zeros(SURVIVAL_ROWS * SURVIVAL_COLS, np.int32)
    rc = L.cvo_cloud_upload_stereo_pair_filtered(ctx, C.byref(frame), _u8(np.ascontiguousarray(right)), sgm(), dfilter(speckle_size=4), FULL, C.byref(h),
                                                 keep.ctypes.data_as(ipp), n_out)
    assert rc == 0, (rc, L.cvo_last_error(ctx).decode())
    L.cvo_cloud_free(h)
    after_success = stats(L, ctx)
    by_name = {c.name: c for c in cases()}
    for name in SURVIVAL_REFUSED:
        assert run(L, ctx, by_name[name])["rc"] != 0, name
    return dict(after_success=after_success, after_refusals=stats(L, ctx))
