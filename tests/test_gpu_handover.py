"""The hand-over frame of the entry points that make a resident cloud of rows on the device (handover_call, cvo_frontend.hip),
per entry point: a call the library refuses on the host, before any launch, leaves *out NULL and its counts zero, and the next
valid call on the same context succeeds with the cloud the same call makes on a fresh context - equal bytes of every array
cvo_cloud_download brings down.  The inputs are refusal_cases.py's: the 16-point cloud, the 8 x 8 frame.  No test provokes a
fault."""
import ctypes as C

import numpy as np
import pytest

import cases
import refusal_cases as rc
from unified_cvo_amd import _capi

pytestmark = pytest.mark.gpu

vp = C.c_void_p
SENTINEL = 0x5A5A5A50  # what *out holds before a refused call: written over with NULL, never read through
FRONT = (rc.XYZ + np.float32([0, 0, 3])).astype(np.float32)  # the cloud in front of a camera at the origin: depths in (2, 4)
EYE = np.eye(4, dtype=np.float32)
KERNEL = (np.eye(3, dtype=np.float32) * np.float32(0.01)).ravel()


def f32(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Ctx:
    """A context, what was made with it (freed before it, in reverse order) and the calls every case shares."""

    def __init__(self, **options):
        self.L, self.h, self.undo = _capi.lib(), vp(), []
        assert self.L.cvo_ctx_create(0, C.byref(self.h)) == 0
        for k, v in options.items():
            assert self.L.cvo_ctx_set_option(self.h, k.encode(), str(v).encode()) == 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for fn, h in reversed(self.undo):
            fn(h)
        self.L.cvo_ctx_destroy(self.h)

    def error(self):
        return self.L.cvo_last_error(self.h).decode()

    def own(self, cloud):
        self.undo.append((self.L.cvo_cloud_free, cloud))
        return cloud

    def upload(self, xyz):
        h = vp()
        assert self.L.cvo_cloud_upload(self.h, len(xyz), f32(xyz), None, None, None, C.byref(h)) == 0, self.error()
        return self.own(h)

    def place(self, a):
        d = vp()
        assert self.L.cvo_debug_device_buffer(self.h, a.nbytes, a.ctypes.data_as(vp), C.byref(d)) == 0, self.error()
        self.undo.append((lambda p: self.L.cvo_debug_device_release(self.h, p), d))
        return d.value

    def download(self, cloud):
        n = self.L.cvo_cloud_size(cloud)
        arrays = [np.full((max(n, 1), w), 7, np.float32) for w in (3, 5, 19, 2)]
        present = C.c_int(-1)
        assert self.L.cvo_cloud_download(self.h, cloud, *(f32(a) for a in arrays), C.byref(present)) == 0, self.error()
        return (n, present.value) + tuple(a[:n].tobytes() for a in arrays)


def refused(rc_code, out, *counts):
    assert rc_code != 0
    assert out.value is None
    assert [c.value for c in counts] == [0] * len(counts)


def from_device(c, refuse):
    L, xyz = c.L, c.place(rc.XYZ)
    rows = _capi.cvo_device_rows_t(n=16, n_records=16, xyz=xyz, xyz_stride=12)
    if refuse:  # a stride below the row's size: check_device_rows, inside the frame
        bad, out = _capi.cvo_device_rows_t(n=16, n_records=16, xyz=xyz, xyz_stride=8), vp(SENTINEL)
        refused(L.cvo_cloud_from_device(c.h, C.byref(bad), C.byref(out)), out)
        assert "a stride of 8 bytes" in c.error()
    out = vp()
    assert L.cvo_cloud_from_device(c.h, C.byref(rows), C.byref(out)) == 0, c.error()
    return c.download(c.own(out))


def merge(c, refuse):
    L = c.L
    a, b = c.upload(rc.XYZ), c.upload(FRONT)
    if refuse:  # a cloud of another context: the entry point's own check
        with Ctx() as other:
            pair, out, nk = (vp * 2)(a.value, other.upload(FRONT).value), vp(SENTINEL), C.c_int(77)
            refused(L.cvo_cloud_merge(c.h, 2, pair, None, 0.0, C.byref(out), None, C.byref(nk)), out, nk)
            assert "belongs to another context" in c.error()
    pair, out, nk = (vp * 2)(a.value, b.value), vp(), C.c_int(77)
    assert L.cvo_cloud_merge(c.h, 2, pair, None, 0.0, C.byref(out), None, C.byref(nk)) == 0, c.error()
    assert nk.value == 32
    return c.download(c.own(out))


def depth_finish(c, refuse):
    L = c.L
    kf, frame, df = c.upload(FRONT), c.upload(FRONT), vp()
    assert L.cvo_depth_filter_open(c.h, kf, C.byref(df)) == 0, c.error()
    c.undo.append((L.cvo_depth_filter_close, df))
    p = cases.load_params("geometric_gpu").to_ctypes()
    assert L.cvo_depth_filter_add(df, C.byref(p), frame, f32(EYE), f32(EYE), f32(KERNEL)) == 0, c.error()
    if refuse:
        out, nk, nf = vp(SENTINEL), C.c_int(77), C.c_int(77)
        refused(L.cvo_depth_filter_finish(df, -1, C.byref(out), None, None, C.byref(nk), C.byref(nf)), out, nk, nf)
        assert "min_count < 0" in c.error()
    out, nk, nf = vp(), C.c_int(77), C.c_int(77)
    assert L.cvo_depth_filter_finish(df, 0, C.byref(out), None, None, C.byref(nk), C.byref(nf)) == 0, c.error()
    assert (nk.value, nf.value) == (16, 0)  # every point meets itself at the identity: one observation each
    return c.download(c.own(out))


def from_rgbd_device(c, refuse):
    L = c.L
    image, depth = c.place(rc.IMG1), c.place(rc.DEPTH)
    f = dict(rows=rc.R, cols=rc.R, channels=1, image=image, gray=None, depth=depth, depth_type=_capi.CVO_DEPTH_F32, fx=50.0, fy=50.0, cx=4.0, cy=4.0,
             scaling_factor=1.0, num_classes=0, semantic=None)
    if refuse:  # the depth plane in host memory: classified inside the frame, before anything reads through it
        bad, out, n = _capi.cvo_rgbd_device_frame_t(**dict(f, depth=rc.DEPTH.ctypes.data)), vp(SENTINEL), C.c_int(77)
        refused(L.cvo_cloud_from_rgbd_device(c.h, C.byref(bad), rc.FULL, C.byref(out), C.byref(n), None), out, n)
        assert "depth is not device memory" in c.error()
    out, n = vp(), C.c_int(77)
    assert L.cvo_cloud_from_rgbd_device(c.h, C.byref(_capi.cvo_rgbd_device_frame_t(**f)), rc.FULL, C.byref(out), C.byref(n), None) == 0, c.error()
    assert n.value == rc.R * rc.R
    return c.download(c.own(out))


def map_resident(c, refuse):
    L, cfg, m = c.L, _capi.cvo_map_config_t(), vp()
    L.cvo_map_config_default(C.byref(cfg))
    assert L.cvo_map_open(c.h, C.byref(cfg), 0, C.byref(m)) == 0, c.error()
    c.undo.append((L.cvo_map_close, m))
    origin = np.zeros(3, np.float32)
    assert L.cvo_map_insert(m, 16, f32(FRONT), None, None, f32(origin)) == 0, c.error()
    if refuse:  # a map without a context has no resident cloud to give
        hm, out, n = vp(), vp(SENTINEL), C.c_longlong(77)
        assert L.cvo_map_open_host(C.byref(cfg), C.byref(hm)) == 0
        refused(L.cvo_map_cloud_resident(hm, C.byref(out), C.byref(n)), out, n)
        L.cvo_map_close_host(hm)
    out, n = vp(), C.c_longlong(77)
    assert L.cvo_map_cloud_resident(m, C.byref(out), C.byref(n)) == 0, c.error()
    assert 1 <= n.value <= 16 and L.cvo_cloud_size(out) == n.value
    return c.download(c.own(out))


ENTRIES = [("cvo_cloud_from_device", from_device, {}), ("cvo_cloud_merge", merge, {}), ("cvo_depth_filter_finish", depth_finish, {}),
           ("cvo_cloud_from_rgbd_device", from_rgbd_device, {}), ("cvo_map_cloud_resident, device side", map_resident, dict(BKI_HOST=0)),
           ("cvo_map_cloud_resident, host side", map_resident, dict(BKI_HOST=1))]


@pytest.mark.parametrize("name,scenario,options", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_refused_call_hands_nothing_over_and_the_next_call_is_a_fresh_one(name, scenario, options):
    with Ctx(**options) as used, Ctx(**options) as fresh:
        got, want = scenario(used, True), scenario(fresh, False)
    assert got[0] > 0
    assert got == want
