"""cvo_cloud_from_rgbd_device / _recipe on the MI355X: the resident cloud of an RGB-D frame whose planes are already in device
memory is the cloud the host-frame route makes of the frame's host copy - upload(rgbd_points(f, method)) and upload_rgbd(f) under
RGBD_HOST=0.  The planes are placed with cvo_debug_device_buffer (no second HIP runtime in the process) and released before the
cloud is used, so every comparison is a lifetime check too.  Every comparison is equality: indices, bit patterns of rows and
scores, the bytes of trace records.  No test provokes a fault: what is refused is decided on the host before any launch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
import np_rgbd_device as nd
import rgbd_cases as rc
import rgbd_device_cases as dc
from test_gpu_ingest import Placed
from unified_cvo_amd import CvoGPU, DeviceRGBDFrame, RGBDFrame, _capi, rgbd_points_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DSO_EDGES, FULL = dc.DSO_EDGES, dc.FULL
EYE = np.eye(4, dtype=np.float32)
LEAF = 0.1


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    g.set_option("RGBD_HOST", 0)   # the host-frame route every cloud is compared with: the kernels at every size
    yield g
    g.close()


@pytest.fixture(scope="module")
def target(gpu):
    """A fixed 1024-point cloud in front of the camera: 1024 evenly spaced FULL points of the `small` frame."""
    t = gpu.upload(target_points())
    yield t
    t.free()


def target_points():
    pc = rgbd_points_host(rc.frame("small"), FULL)
    idx = np.unique(np.linspace(0, pc.num_points() - 1, 1024).astype(np.int64))
    assert len(idx) == 1024
    return pc.select(idx)


def odd_frame(depth):
    """33 x 31, a corner of the `small` frame: a ragged edge on both axes, 1023 pixels."""
    f = rc.frame("small", depth)
    return RGBDFrame(np.ascontiguousarray(f.image[60:93, 90:121]), np.ascontiguousarray(f.depth[60:93, 90:121]), 25.0, 27.0, 15.5, 16.0, f.scaling_factor)


def get_frame(name, depth="u16"):
    return odd_frame(depth) if name == "odd" else rc.frame(name, depth)


class OnDevice:
    """The planes of a host RGBDFrame placed in device memory -> a DeviceRGBDFrame over them; released on exit.
    presentation: how the class scores are laid out (rgbd_device_cases.presentations)."""

    def __init__(self, g, f, presentation="hwc"):
        self.g, self.f, self.presentation, self.placed = g, f, presentation, Placed(g)

    def __enter__(self):
        p, f = self.placed, self.f
        self.image, self.depth = p.put(f.image), p.put(f.depth)
        self.gray = None if f.gray is None else p.put(f.gray)
        sem = None
        if f.semantic is not None:
            base, view, layout = dc.presentations(f.semantic)[self.presentation]
            strides, classes = dc.strides_of(view, layout)
            self.semantic_base = p.put(base)
            self.semantic_bytes = base.nbytes
            sem = (self.semantic_base + (view.ctypes.data - base.ctypes.data), classes) + tuple(strides)
        self.frame = DeviceRGBDFrame((self.image, f.rows, f.cols, f.channels), (self.depth, "u16" if f.depth.dtype == np.uint16 else "f32"),
                                     f.fx, f.fy, f.cx, f.cy, f.scaling_factor, gray=None if self.gray is None else (self.gray,), semantic=sem)
        return self

    def overwrite(self):
        """Other bytes over every plane (the planes are about to be released: a cloud must not depend on them)."""
        f = self.f
        self.g.debug_device_buffer(np.full(f.image.shape, 255, np.uint8), into=self.image)
        self.g.debug_device_buffer(np.full(f.depth.shape, 1, f.depth.dtype), into=self.depth)
        if f.semantic is not None:
            self.g.debug_device_buffer(np.full(self.semantic_bytes // 4, 1e9, np.float32), into=self.semantic_base)

    def __exit__(self, *exc):
        return self.placed.__exit__(*exc)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rows_of(cloud):
    d = cloud.download()
    return dict(present=d.present, xyz=bits(d.positions_), feat=bits(d.features_), label=bits(d.labels_), geo=bits(d.geometric_types_))


def solved(g, cloud, target, iters=8):
    """One inner product and one short traced align against the target, in comparable form (a refusal compares as its text)."""
    try:
        ip = int(np.float32(g.inner_product_gpu(cloud, target, EYE, 0.3)).view(np.uint32))
        r = g.align(cloud, target, EYE, max_iterations=iters, trace_capacity=iters, trace_dense=iters)
        return (ip, r.ret, r.iterations, r.transform.tobytes(), [bytes(t) for t in r.trace])
    except Exception as e:   # noqa: BLE001 - both clouds must then be refused in the same words
        return str(e)


def assert_same_cloud(g, d, h, target, what):
    assert d.n == h.n, what
    if d.n == 0:
        return None
    rd, rh = rows_of(d), rows_of(h)
    for k in rh:
        assert np.array_equal(rd[k], rh[k]), (what, k)
    assert np.array_equal(d.debug_order(), h.debug_order()), what
    assert d.debug_order_route() == h.debug_order_route(), what
    sd, sh = solved(g, d, target), solved(g, h, target)
    assert sd == sh, what
    return sd


class NoCloud:
    """In the place of upload() of a CvoPointCloud without points."""
    n = 0

    def free(self):
        pass


def host_points(g, f, method):
    """The host-frame route: (cloud, pixel, stats)."""
    pc = g.rgbd_points(f, method)
    st = g.debug_rgbd_stats()
    return (g.upload(pc) if pc.num_points() else NoCloud()), pc.pixel, st


def device_points(g, f, method, presentation="hwc", want_pixel=True):
    with OnDevice(g, f, presentation) as on:
        d = g.upload_rgbd_points_device(on.frame, method, want_pixel=want_pixel)
        st = g.debug_rgbd_stats()
    return d, st


def device_recipe(g, f, leaf=LEAF, divisor=4, presentation="hwc", want_pixel=True):
    with OnDevice(g, f, presentation) as on:
        d = g.upload_rgbd_device(on.frame, leaf, divisor, want_pixel=want_pixel)
        st = g.debug_rgbd_stats()
    return d, st


def check_points(g, f, method, target, what, presentation="hwc"):
    h, pixel, st_h = host_points(g, f, method)
    d, st_d = device_points(g, f, method, presentation)
    try:
        assert st_d == st_h and st_d["on_device"], (what, st_d, st_h)
        assert np.array_equal(d.pixel, pixel), what
        return assert_same_cloud(g, d, h, target, what), d.n
    finally:
        d.free()
        h.free()


def check_recipe(g, f, target, what, leaf=LEAF, divisor=4, presentation="hwc"):
    h = g.upload_rgbd(f, leaf, divisor)
    st_h = g.debug_rgbd_stats()
    d, st_d = device_recipe(g, f, leaf, divisor, presentation)
    try:
        assert st_d == st_h and st_d["on_device"], (what, st_d, st_h)
        assert np.array_equal(d.pixel, h.pixel) and np.array_equal(d.is_edge, h.is_edge) and d.n_edge == int(h.is_edge.sum()), what
        return assert_same_cloud(g, d, h, target, what), d.n, d.n_edge
    finally:
        d.free()
        h.free()


# ---- equality with the host-frame route ----

@pytest.mark.parametrize("depth", rc.DEPTHS)
@pytest.mark.parametrize("name", ["tiny", "small", "mono", "semantic", "odd"])
def test_equals_the_host_frame_route(gpu, target, name, depth):
    f = get_frame(name, depth)
    sizes = {}
    for mname, method in (("dso", DSO_EDGES), ("full", FULL)):
        _, sizes[mname] = check_points(gpu, f, method, target, (name, depth, mname))
    _, n, n_edge = check_recipe(gpu, f, target, (name, depth, "recipe"))
    print(f"{name} {depth}: dso {sizes['dso']} full {sizes['full']} recipe {n} ({n_edge} edges)")
    if name == "small":
        assert sizes["full"] > 16384    # the host orders it and k_cloud_gather runs
    if name == "semantic":
        with_depth = np.count_nonzero(f.depth) if depth == "u16" else np.count_nonzero((f.depth != 0) & ~np.isnan(f.depth))
        assert 0 < sizes["full"] < with_depth    # the rule excludes some pixels that have a depth


def test_statement_rows(gpu):
    """... and the rows are the numpy statement's, not only the host route's."""
    f = rc.frame("semantic")
    for method in (DSO_EDGES, FULL):
        want = dc.statement_points(f, method)
        d, st = device_points(gpu, f, method)
        got = d.download()
        assert np.array_equal(d.pixel, want["pixel"])
        dc.assert_rows_equal(dict(xyz=got.positions_, feat=got.features_, label=got.labels_, geotype=got.geometric_types_), want, method)
        if method == FULL:
            assert st["with_depth"] == want["with_depth"] > st["surface_points"] == len(want["pixel"])   # counted on the device
        d.free()
    r = dc.statement_recipe(f, LEAF)
    d, st = device_recipe(gpu, f)
    got = d.download()
    assert np.array_equal(d.pixel, r["pixel"]) and np.array_equal(d.is_edge, r["is_edge"].astype(bool)) and not got.present & 2
    dc.assert_rows_equal(dict(xyz=got.positions_, feat=got.features_, label=None, geotype=got.geometric_types_), r, "recipe", labels=False)
    assert st["with_depth"] == r["stats"]["with_depth"]
    d.free()


def test_wide_ordering(target):
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    try:
        g.set_option("RGBD_HOST", 0)
        g.set_option("ORDER", "wide")
        t = g.upload(target_points())
        f = rc.frame("small")
        h, pixel, _ = host_points(g, f, FULL)
        d, _ = device_points(g, f, FULL)
        assert d.debug_order_route() == h.debug_order_route() == 2
        assert np.array_equal(d.pixel, pixel)
        assert_same_cloud(g, d, h, t, "ORDER=wide")
    finally:
        g.close()


def test_repeats_are_identical_and_pixel_is_optional(gpu, target):
    f = rc.frame("semantic", "f32")
    first, _ = device_points(gpu, f, DSO_EDGES)
    again, _ = device_points(gpu, f, DSO_EDGES, want_pixel=False)
    assert not hasattr(again, "pixel") and np.array_equal(rows_of(first)["xyz"], rows_of(again)["xyz"])
    assert_same_cloud(gpu, again, first, target, "repeat")
    r1, _ = device_recipe(gpu, f)
    r2, _ = device_recipe(gpu, f, want_pixel=False)
    assert r2.n_edge == r1.n_edge and not hasattr(r2, "pixel")
    assert_same_cloud(gpu, r2, r1, target, "repeat of the recipe")
    for c in (first, again, r1, r2):
        c.free()


# ---- layouts ----

def test_three_layouts_give_the_same_cloud(gpu, target):
    f = rc.frame("semantic")
    seen = []
    for presentation in dc.LAYOUTS:
        for method in (DSO_EDGES, FULL):
            seen.append((presentation, method, check_points(gpu, f, method, target, (presentation, method), presentation)))
        seen.append((presentation, "recipe", check_recipe(gpu, f, target, (presentation, "recipe"), presentation=presentation)))
    for k in range(3):
        assert seen[k][2] == seen[3 + k][2] == seen[6 + k][2], seen[k][:2]


# ---- the exclusion rule's and the rows' edges, through the kernels ----

@pytest.mark.parametrize("name", sorted(dc.RULE_CASES))
def test_exclusion_rule_edges(gpu, name):
    f = dc.rule_frame(name)
    want = dc.statement_points(f, FULL)
    for presentation in dc.LAYOUTS:
        d, st = device_points(gpu, f, FULL, presentation)
        got = d.download()
        assert np.array_equal(d.pixel, want["pixel"]), (name, presentation)
        dc.assert_rows_equal(dict(xyz=got.positions_, feat=got.features_, label=got.labels_, geotype=got.geometric_types_), want, (name, presentation))
        assert st["with_depth"] == dc.H * dc.W and st["surface_points"] == len(want["pixel"])
        assert (len(want["pixel"]) < dc.H * dc.W) == dc.RULE_EXCLUDES[name]
        d.free()


def test_nan_scores_follow_the_existing_host_entry_point(gpu):
    """Compared with cvo_rgbd_points_host only (np.argmax treats a NaN differently; upstream's behaviour there is not pinned)."""
    f = dc.nan_frame()
    pc = rgbd_points_host(f, FULL)
    d, _ = device_points(gpu, f, FULL)
    got = d.download()
    assert np.array_equal(d.pixel, pc.pixel) and 0 < d.n < dc.H * dc.W
    assert np.array_equal(bits(got.labels_), bits(nd.pad(pc.labels(), nd.CLASSES))) and np.array_equal(bits(got.positions_), bits(pc.positions()))
    d.free()


def test_last_pixel_border_pixels_and_own_gray(gpu, target):
    f = dc.rule_frame("classes_19")
    d, _ = device_points(gpu, f, FULL)
    assert dc.H * dc.W - 1 in d.pixel.tolist() and dc.border(d.pixel).any()
    d.free()
    every = RGBDFrame(rc.frame("tiny").image, np.ones_like(rc.frame("tiny").depth), 30.0, 30.0, 20.0, 10.0, 1.0)   # every pixel kept: all four borders
    want = dc.statement_points(every, FULL)
    d, _ = device_points(gpu, every, FULL)
    got = d.download()
    assert d.n == every.rows * every.cols and np.array_equal(d.pixel, want["pixel"])
    dc.assert_rows_equal(dict(xyz=got.positions_, feat=got.features_, label=None, geotype=got.geometric_types_), want, "every pixel")
    d.free()
    own = rc.own_gray(rc.frame("small"))
    check_points(gpu, own, DSO_EDGES, target, "own gray")
    check_recipe(gpu, own, target, "own gray recipe")
    plain, _ = device_points(gpu, rc.frame("small"), DSO_EDGES)
    mine, _ = device_points(gpu, own, DSO_EDGES)
    assert not np.array_equal(plain.pixel, mine.pixel)   # the plane is what the selection looks at
    plain.free()
    mine.free()


# ---- degenerate results ----

def test_zero_depth_gives_an_empty_cloud(gpu, target):
    for depth in rc.DEPTHS:
        z = rc.zero_depth(rc.frame("small", depth))
        for method in (DSO_EDGES, FULL):
            _, n = check_points(gpu, z, method, target, ("zero depth", depth, method))
            assert n == 0
        _, n, n_edge = check_recipe(gpu, z, target, ("zero depth", depth, "recipe"))
        assert n == 0 and n_edge == 0


def test_every_candidate_excluded(gpu, target):
    f = rc.frame("semantic")
    sem = np.full_like(f.semantic, 0.01)
    sem[..., 10] = 0.9
    g = RGBDFrame(f.image, f.depth, f.fx, f.fy, f.cx, f.cy, f.scaling_factor, semantic=sem)
    for method in (DSO_EDGES, FULL):
        _, n = check_points(gpu, g, method, target, ("all excluded", method))
        assert n == 0
    st = gpu.debug_rgbd_stats()
    assert st["surface_points"] == 0 and st["with_depth"] == np.count_nonzero(f.depth) > 0
    _, n, _ = check_recipe(gpu, g, target, "all excluded, recipe")
    assert n == 0 and gpu.debug_rgbd_stats()["with_depth"] == np.count_nonzero(f.depth)


def test_recipe_without_edges_and_with_one_voxel(gpu, target):
    f = rc.frame("small")
    flat = RGBDFrame(np.full_like(f.image, 97), f.depth, f.fx, f.fy, f.cx, f.cy, f.scaling_factor)   # no gradient: nothing is selected
    _, n, n_edge = check_recipe(gpu, flat, target, "no edges")
    assert n_edge == 0 and n > 0
    _, n, n_edge = check_recipe(gpu, f, target, "one voxel", leaf=1000.0)
    assert (n, n_edge) == (2, 1)    # one voxel survives per set


# ---- lifetime ----

def test_cloud_outlives_its_planes(gpu, target):
    f = rc.frame("semantic")
    h, _, _ = host_points(gpu, f, DSO_EDGES)
    with OnDevice(gpu, f, "chw") as on:
        d = gpu.upload_rgbd_points_device(on.frame, DSO_EDGES)
        r = gpu.upload_rgbd_device(on.frame, LEAF)
        on.overwrite()
    hr = gpu.upload_rgbd(f, LEAF)
    assert_same_cloud(gpu, d, h, target, "after release")
    assert_same_cloud(gpu, r, hr, target, "recipe after release")
    for c in (d, h, r, hr):
        c.free()


# ---- refusals: a message, *out NULL, nothing allocated, the context usable afterwards ----

def _loaded_hip(device_address):
    """The HIP runtime the library has ALREADY loaded - no second runtime: of the libamdhip64 objects mapped into the process
    (torch brings a copy of its own when a test has imported it) the one that knows an allocation the library made."""
    paths = []
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path and path not in paths:
            paths.append(path)
    for path in paths:
        hip = C.CDLL(path)
        hip.hipPointerGetAttributes.argtypes = [C.c_void_p, C.c_void_p]
        if hip.hipPointerGetAttributes(C.create_string_buffer(256), C.c_void_p(device_address)) == 0:
            return hip
    raise AssertionError(f"no mapped libamdhip64 knows the library's allocation: {paths}")


class Pinned:
    """Pinned host memory from the library's own runtime; device_address: any allocation the library made."""

    def __init__(self, nbytes, device_address):
        self.hip, self.p = _loaded_hip(device_address), C.c_void_p()
        self.hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        self.hip.hipHostFree.argtypes = [C.c_void_p]
        assert self.hip.hipHostMalloc(C.byref(self.p), nbytes, 0) == 0

    def __enter__(self):
        return self.p.value

    def __exit__(self, *exc):
        self.hip.hipHostFree(self.p)
        return False


def _refused(g, fs, text, code=_capi.CVO_E_INVALID, method=DSO_EDGES, recipe=(LEAF, 4.0), calls=("points", "recipe")):
    free0 = g.debug_device_memory()[0]
    msgs = []
    for call in calls:
        h, n = C.c_void_p(12345), C.c_int(-7)
        if call == "points":
            rc_ = g.L.cvo_cloud_from_rgbd_device(g.ctx, C.byref(fs), method, C.byref(h), C.byref(n), None)
        else:
            rc_ = g.L.cvo_cloud_from_rgbd_device_recipe(g.ctx, C.byref(fs), recipe[0], recipe[1], C.byref(h), C.byref(n), None, None)
        msg = g.L.cvo_last_error(g.ctx).decode()
        assert rc_ == code and text in msg and h.value is None and n.value == 0, (call, rc_, msg, h.value)
        msgs.append(msg)
    assert g.debug_device_memory()[0] == free0
    return msgs


def test_refusals(gpu, target):
    f = rc.frame("semantic", "f32")
    np_ = f.rows * f.cols
    with OnDevice(gpu, f) as on, Pinned(f.semantic.nbytes, on.image) as pinned:
        ok = gpu.upload_rgbd_points_device(on.frame, DSO_EDGES)   # (the regions exist from here on: a refusal must not grow anything)
        before = rows_of(ok)
        ok.free()
        host = {"image": f.image.ctypes.data, "gray": f.image.ctypes.data, "depth": f.depth.ctypes.data, "semantic": f.semantic.ctypes.data}
        for plane in ("image", "gray", "depth", "semantic"):
            for where, address in (("host", host[plane]), ("pinned", pinned)):
                fs = on.frame.c_struct()
                setattr(fs, plane, address)
                _refused(gpu, fs, plane + " is not device memory")
        # an extent that leaves its allocation by one byte: image, depth, and the scores through each stride
        with Placed(gpu) as p:
            fs = on.frame.c_struct()
            fs.image = p.put(f.image.reshape(-1)[:-1])
            _refused(gpu, fs, "image: ")
            fs = on.frame.c_struct()
            fs.depth = p.put(f.depth.view(np.uint8).reshape(-1)[:-1])
            _refused(gpu, fs, "depth: ")
            for presentation in dc.LAYOUTS:
                base, view, layout = dc.presentations(f.semantic)[presentation]
                (rs, ps, cs), classes = dc.strides_of(view, layout)
                off = view.ctypes.data - base.ctypes.data
                need = (f.rows - 1) * rs + (f.cols - 1) * ps + (classes - 1) * cs + 4
                fs = on.frame.c_struct()
                fs.semantic = p.put(base.view(np.uint8).reshape(-1)[:off + need - 1]) + off
                fs.semantic_row_stride, fs.semantic_pixel_stride, fs.semantic_class_stride = rs, ps, cs
                msg = _refused(gpu, fs, "semantic: ")[0]
                assert f"need {need} bytes, the allocation ends after {need - 1}" in msg, msg
                fs.semantic = p.put(base.view(np.uint8).reshape(-1)[:off + need]) + off     # exactly enough: accepted
                h = C.c_void_p()
                assert gpu.L.cvo_cloud_from_rgbd_device(gpu.ctx, C.byref(fs), DSO_EDGES, C.byref(h), None, None) == 0
                gpu.L.cvo_cloud_free(h)
        for field in ("semantic_row_stride", "semantic_pixel_stride", "semantic_class_stride"):
            for bad in (0, 6):
                fs = on.frame.c_struct()
                setattr(fs, field, bad)
                _refused(gpu, fs, field + ": a stride of " + str(bad))
        fs = on.frame.c_struct()
        fs.num_classes = 20
        _refused(gpu, fs, "num_classes 20", _capi.CVO_E_UNSUPPORTED)
        with Placed(gpu) as p:
            fs = on.frame.c_struct()
            fs.depth = p.put(np.zeros(np_ + 1, np.float32)) + 2
            _refused(gpu, fs, "depth is not 4-byte aligned")
        _refused(gpu, on.frame.c_struct(), "is not supported", _capi.CVO_E_UNSUPPORTED, method=_capi.CVO_SELECT_CV_FAST, calls=("points",))
        # cvo_rgbd_points' refusals, in its words
        for field, value, text in (("rows", 0, "rows and cols"), ("channels", 2, "channels must be 1 or 3"), ("image", None, "image is NULL"),
                                   ("depth", None, "depth is NULL"), ("fx", 0.0, "fx and fy"), ("scaling_factor", float("nan"), "scaling_factor"),
                                   ("semantic", None, "needs the semantic image")):
            fs = on.frame.c_struct()
            setattr(fs, field, value)
            _refused(gpu, fs, text)
        _refused(gpu, on.frame.c_struct(), "leaf", recipe=(0.0, 4.0), calls=("recipe",))
        _refused(gpu, on.frame.c_struct(), "edge_divisor", recipe=(LEAF, -4.0), calls=("recipe",))
        again = gpu.upload_rgbd_points_device(on.frame, DSO_EDGES)   # the context is as usable as before
        after = rows_of(again)
        assert all(np.array_equal(before[k], after[k]) for k in before)
        again.free()


# ---- downstream ----

def test_multiframe_over_device_built_recipe_clouds():
    from test_gpu_multiframe import _mf_params
    g = CvoGPU(params=_mf_params(max_iters=6))
    try:
        g.set_option("RGBD_HOST", 0)
        frames = [rc.frame("semantic", shift=2.0 * k) for k in range(4)]
        dev = [device_recipe(g, f, 0.2)[0] for f in frames]
        host = [g.upload_rgbd(f, 0.2) for f in frames]
        X0 = np.tile(np.eye(4)[:3].reshape(12), (4, 1))
        for k in range(1, 4):
            X0[k, 3] = 0.01 * k
        edges, hold, cap = [0, 1, 1, 2, 2, 3, 0, 2], [1, 0, 0, 0], 10
        rc1, P1, i1, rows1, n1 = g.multiframe_align_raw(dev, X0, hold, edges, trace_capacity=cap)
        rc2, P2, i2, rows2, n2 = g.multiframe_align_raw(host, X0, hold, edges, trace_capacity=cap)
        assert rc1 == rc2 == 0 and n1 == n2 > 0 and i1.solves == i2.solves > 0
        assert np.array_equal(P1, P2) and not np.array_equal(P1, np.asarray(X0).reshape(-1))
        for k in range(n1):
            for name, _ in _capi.cvo_multiframe_trace_t._fields_:
                assert getattr(rows1[k], name) == getattr(rows2[k], name), (k, name)
    finally:
        g.close()


def test_semantic_map_insert_of_a_device_built_cloud(gpu):
    import bki_cases as bc
    import np_bki
    import unified_cvo_amd as u
    f = rc.frame("semantic")
    h, _, _ = host_points(gpu, f, DSO_EDGES)
    d, _ = device_points(gpu, f, DSO_EDGES)
    cfg = np_bki.Config(resolution=0.1, num_classes=19, free_resolution=1e4)
    T = np.array([[1, 0, 0, 0.5], [0, 1, 0, -0.25], [0, 0, 1, 0.125]], np.float32)
    gpu.set_option("BKI_HOST", 0)
    try:
        A, B = gpu.map_open(u.MapConfig(**cfg.kwargs())), gpu.map_open(u.MapConfig(**cfg.kwargs()))
        A.insert_cloud(d, pose=T)
        B.insert_cloud(h, pose=T)
        sa, sb = A.debug_stats(readback=True), B.debug_stats(readback=True)
        assert sa["voxels"] == sb["voxels"] > 0 and bc.first_difference(sa, (sb["keys"], sb["ms"], sb["fs"])) is None
        A.close()
        B.close()
    finally:
        gpu.set_option("BKI_HOST", None)
        d.free()
        h.free()


# ---- torch tensors: one child process, torch first and the library afterwards, as bench.py does ----

TORCH_CHILD = r"""
import sys
import numpy as np
import torch
if not torch.cuda.is_available():
    print("NO_DEVICE")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
from unified_cvo_amd import CvoGPU, DeviceRGBDFrame, RGBDFrame
import cases
import rgbd_cases as rc
f = rc.frame("semantic", "f32")
dev = torch.device("cuda", 0)
logits = torch.log(torch.from_numpy(np.ascontiguousarray(np.moveaxis(f.semantic, 2, 0))).to(dev))
scores = torch.softmax(logits, dim=0)                       # C x H x W, as a network leaves it
host = RGBDFrame(f.image, f.depth, f.fx, f.fy, f.cx, f.cy, f.scaling_factor, semantic=scores.permute(1, 2, 0).contiguous().cpu().numpy())
g = CvoGPU(params=cases.load_params("geometric_gpu"))
g.set_option("RGBD_HOST", 0)
frame = DeviceRGBDFrame(torch.from_numpy(f.image).to(dev), torch.from_numpy(f.depth).to(dev), f.fx, f.fy, f.cx, f.cy, f.scaling_factor,
                        semantic=scores, layout="chw")
out = []
for method in (2, 8):
    h = g.upload(g.rgbd_points(host, method))
    d = g.upload_rgbd_points_device(frame, method, want_pixel=True)
    a, b = h.download(), d.download()
    same = all(np.array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32))
               for x, y in ((a.positions_, b.positions_), (a.features_, b.features_), (a.labels_, b.labels_), (a.geometric_types_, b.geometric_types_)))
    out.append((h.n, d.n, same and np.array_equal(h.debug_order(), d.debug_order())))
hr, dr = g.upload_rgbd(host, 0.1), g.upload_rgbd_device(frame, 0.1, want_pixel=True)
out.append((hr.n, dr.n, np.array_equal(hr.pixel, dr.pixel) and np.array_equal(hr.debug_order(), dr.debug_order())))
print("RESULT", " ".join(f"{a}:{b}:{int(c)}" for a, b, c in out))
"""


def test_torch_tensors_in_a_child_process(tmp_path):
    script = tmp_path / "torch_child.py"
    script.write_text(TORCH_CHILD)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=240, env=env)
    if "NO_DEVICE" in out.stdout:
        pytest.skip("torch sees no device")
    assert out.returncode == 0, out.stdout + out.stderr
    parts = [p.split(":") for p in [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()[1:]]
    assert len(parts) == 3
    for a, b, same in parts:
        assert a == b and int(a) > 0 and same == "1", parts
