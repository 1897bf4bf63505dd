"""cvo_cloud_merge / cvo_cloud_download (cvo_merge.hip, cvo_k_merge.h) on the MI355X.

Download first, against the caller's own arrays, for every route that makes a cloud.  Then merge: the expected cloud is built
from code that was there before - every input moved by CvoGPU.transformed and read back, the rows concatenated in numpy and
handed to upload_voxel (voxel size 0: upload) - and "equal" means: download() bitwise equal in every array and in `present`,
the same spatial order and ordering route, the same bits of an inner product against a fixed 500-point probe, and one
30-iteration align against that probe ending in the same 16 floats after the same number of iterations.  No tolerance but
one: a transformed cloud's coordinates against numpy's statement of the same float arithmetic, within 1 ulp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cases
import np_voxel
from test_gpu_ingest import Placed
from unified_cvo_amd import CvoGPU, CvoPointCloud, _capi, synth
from unified_cvo_amd.api import cvo_points_from_pointcloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
EYE12 = np.eye(4)[:3].reshape(12)
ELL = 0.3
LEAF = 0.5
NC, FD = synth.NUM_CLASSES, 5


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("semantic_img_gpu0"))
    yield g
    g.close()


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def rows(n, seed, mix="full", soft_row=None):
    """(xyz, feat, label, geo) of n points; mix: "xyz", "colour" or "full" (colour, one-hot labels, geometric types)."""
    rs = np.random.default_rng(1000 + seed)
    xyz = np.ascontiguousarray(synth.semantic_pair(max(n, 1), seed)[0][:n], np.float32)
    feat = rs.uniform(0, 1, (n, FD)).astype(np.float32) if mix in ("colour", "full") else None
    label = geo = None
    if mix == "full":
        label = np.zeros((n, NC), np.float32)
        label[np.arange(n), rs.integers(0, NC, n)] = 1.0
        if soft_row is not None and n > soft_row:
            label[soft_row] = np.float32(1.0 / NC)
        geo = np.zeros((n, 2), np.float32)
        geo[np.arange(n), rs.integers(0, 2, n)] = 1.0
    return xyz, feat, label, geo


def upload_raw(g, arrs):
    """cvo_cloud_upload of exactly these arrays (None stays NULL)."""
    h = C.c_void_p()
    g._check(g.L.cvo_cloud_upload(g.ctx, arrs[0].shape[0], *[_fp(a) for a in arrs], C.byref(h)))
    return g._adopt(h, arrs[0].shape[0])


def upload_voxel_raw(g, arrs, s):
    n = arrs[0].shape[0]
    kept, nk, h = np.zeros(max(n, 1), np.int32), C.c_int(), C.c_void_p()
    g._check(g.L.cvo_cloud_upload_voxel(g.ctx, n, *[_fp(a) for a in arrs], float(s), C.byref(h),
                                        kept.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nk)))
    return g._adopt(h, nk.value), kept[:nk.value].copy()


def downloaded(cloud):
    """(xyz, feat, label, geo, present) of a resident cloud; an attribute it does not hold is None."""
    pc = cloud.download()
    has = pc.present
    return (pc.positions_, pc.features_ if has & 1 else None, pc.labels_ if has & 2 else None,
            pc.geometric_types_.reshape(-1, 2) if has & 4 else None, has)


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_rows(cloud, want):
    got = downloaded(cloud)
    for k, name in enumerate(("xyz", "feat", "label", "geo")):
        assert same_bits(got[k], want[k]), name
    assert got[4] == sum(bit for bit, a in zip((1, 2, 4), want[1:]) if a is not None and cloud.n > 0)


def rigid(rs, angle=0.4, shift=1.0):
    """A 3x4 rigid pose in doubles (Rodrigues)."""
    w = rs.normal(size=3)
    w *= rs.uniform(0.05, angle) / np.linalg.norm(w)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    return np.concatenate([R, rs.uniform(-shift, shift, (3, 1))], axis=1).reshape(12)


def np_transform(pose12, xyz):
    """transform_point_pose_vec in numpy: fma(T0, x, T1 * y) + fma(T2, z, T3) per row, float32 (a product of two floats is
    exact in a double; the fused sums are rounded once from the double)."""
    T = np.asarray(pose12, np.float64).astype(np.float32).reshape(3, 4)
    x, y, z = (xyz[:, k].astype(np.float32) for k in range(3))
    out = np.zeros_like(xyz, dtype=np.float32)
    for r in range(3):
        p1 = (T[r, 1] * y).astype(np.float32)
        a = (np.float64(T[r, 0]) * x.astype(np.float64) + p1.astype(np.float64)).astype(np.float32)
        b = (np.float64(T[r, 2]) * z.astype(np.float64) + np.float64(T[r, 3])).astype(np.float32)
        out[:, r] = a + b
    return out


def ulp_apart(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(2 ** 31) - ia, ia), np.where(ib < 0, -(2 ** 31) - ib, ib)
    return int(np.abs(ia - ib).max()) if a.size else 0


# ---- download alone: every route that makes a cloud, against the caller's arrays ----

ROUTES = ("upload", "upload_aos192", "upload_many", "upload_device", "transformed", "upload_voxel")
SIZES = (1, 7, 8, 257, 16400)


def _download_case(g, route, n):
    arrs = rows(n, 3)
    pc = CvoPointCloud.from_arrays(*arrs)
    want = arrs
    if route == "upload":
        c = upload_raw(g, arrs)
    elif route == "upload_aos192":
        c = g.upload_aos192(cvo_points_from_pointcloud(pc))
    elif route == "upload_many":
        other = CvoPointCloud.from_arrays(*rows(9, 4))
        extra, c = g.upload_many([other, pc])
        extra.free()
    elif route == "upload_device":
        with Placed(g) as p:
            c = g.upload_device(*[p.rows(a) for a in arrs])
    elif route == "transformed":
        pose = rigid(np.random.default_rng(n))
        src = upload_raw(g, arrs)
        c = g.transformed(src, pose.reshape(3, 4))
        src.free()
        got = downloaded(c)
        d = ulp_apart(np.ascontiguousarray(got[0]), np_transform(pose, arrs[0]))
        print(f"transformed n={n}: coordinates {d} ulp from numpy")
        assert d <= 1
        want = (got[0],) + arrs[1:]  # (the coordinates are checked above; the attributes must be the caller's)
    else:
        c, kept = upload_voxel_raw(g, arrs, LEAF)
        assert np.array_equal(kept, np_voxel.reference(arrs[0], LEAF)) and (n < 257 or kept.shape[0] < n)
        want = tuple(a[kept] for a in arrs)
    try:
        assert c.n == want[0].shape[0]
        assert_rows(c, want)
    finally:
        c.free()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("route", ROUTES)
def test_download_returns_the_uploaded_rows(gpu, route, n):
    _download_case(gpu, route, n)


@pytest.mark.parametrize("route", ROUTES)
def test_download_under_the_wide_ordering(route):
    g = CvoGPU(params=cases.load_params("semantic_img_gpu0"))
    try:
        g.set_option("ORDER", "wide")
        _download_case(g, route, 16400)
    finally:
        g.close()


def test_download_absent_attributes_and_special_values(gpu):
    xyz = rows(9, 5)[0].copy()
    u = xyz.view(np.uint32)
    u[2, 0], u[4, 1], u[6, 2], u[7, 0] = 0x80000000, 0x7F800000, 0x7FC01234, 0xFF800000  # -0.0, +inf, a NaN with a payload, -inf
    c = upload_raw(gpu, (xyz, None, None, None))
    t = upload_raw(gpu, rows(500, 9))
    try:
        assert c.debug_order_route() == 0
        assert_rows(c, (xyz, None, None, None))
        f = upload_raw(gpu, rows(300, 6, "colour"))
        gpu.inner_product_gpu(f, t, EYE, ELL)  # attaches zeroed labels / types to f: still absent
        assert_rows(f, rows(300, 6, "colour"))
        pc = f.download()
        assert pc.present == 1 and pc.labels_.shape == (300, 0) and not pc.geometric_types_.any()
        assert gpu.download(f).positions_.tobytes() == pc.positions_.tobytes()
        f.free()
        e = upload_raw(gpu, rows(0, 1))
        assert e.download().num_points() == 0 and e.download().present == 0
        e.free()
    finally:
        c.free()
        t.free()


# ---- merge ----

LISTS = {"forward": (0, 1, 7, 8, 255, 256, 257, 1000), "reversed": (1000, 257, 256, 255, 8, 7, 1, 0), "single": (257,),
         "empty": (0, 0, 0)}
MIXES = ("xyz", "colour", "full")


@pytest.fixture(scope="module")
def probe(gpu):
    t = upload_raw(gpu, rows(500, 77))
    yield t
    t.free()


def make_inputs(g, sizes, soft=False, labelled=False):
    """Inputs of the given sizes: xyz only, colour, colour + one-hot labels + geometric types in turn (labelled: every input
    the last kind, so that the merged cloud is one-hot as a whole); soft: row 3 of every labelled input is not one-hot."""
    arrs = [rows(n, 10 + k, "full" if labelled else MIXES[k % 3], soft_row=3 if soft else None) for k, n in enumerate(sizes)]
    return arrs, [upload_raw(g, a) for a in arrs]


def expected_rows(g, clouds, poses):
    """The host route: every input moved by CvoGPU.transformed and read back, concatenated; an attribute some input holds
    is zeros for the inputs that do not."""
    parts = []
    for k, c in enumerate(clouds):
        m = c if poses is None else g.transformed(c, np.asarray(poses[k]).reshape(3, 4))
        parts.append(downloaded(m))
        if m is not c:
            m.free()
    out = [np.concatenate([p[0] for p in parts])]
    for k, w in ((1, FD), (2, NC), (3, 2)):
        if any(p[k] is not None for p in parts):
            out.append(np.ascontiguousarray(np.concatenate(
                [p[k] if p[k] is not None else np.zeros((p[0].shape[0], w), np.float32) for p in parts]), np.float32))
        else:
            out.append(None)
    return tuple(out)


def assert_equal_clouds(g, got, want, probe):
    assert got.n == want.n
    a, b = downloaded(got), downloaded(want)
    for k, name in enumerate(("xyz", "feat", "label", "geo")):
        assert same_bits(a[k], b[k]), name
    assert a[4] == b[4]
    assert np.array_equal(got.debug_order(), want.debug_order()) and got.debug_order_route() == want.debug_order_route()
    def outcome(fn):  # (an empty cloud may be refused by a solver: then both must be refused alike)
        try:
            return fn()
        except Exception as e:
            return ("refused", type(e).__name__, str(e))

    ip = [outcome(lambda: int(np.float32(g.inner_product_gpu(c, probe, EYE, ELL)).view(np.uint32))) for c in (got, want)]
    assert ip[0] == ip[1], ip

    def solve(c):
        r = g.align(c, probe, EYE, max_iterations=30)
        return r.ret, r.iterations, r.transform.tobytes()

    ra, rb = outcome(lambda: solve(got)), outcome(lambda: solve(want))
    assert ra == rb
    assert got.n == 0 or (ra[0] != "refused" and isinstance(ip[0], int))
    assert downloaded(got)[4] == a[4]  # (the calls above may have attached zero slabs: still absent)


def merge_case(g, probe, sizes, pose_kind, s, soft=False, clouds=None, labelled=False):
    arrs, made = (None, None) if clouds is not None else make_inputs(g, sizes, soft, labelled)
    clouds = clouds if clouds is not None else made
    rs = np.random.default_rng(5)
    poses = {"none": None, "identity": np.tile(EYE12, (len(clouds), 1)),
             "rigid": np.stack([rigid(rs) for _ in clouds])}[pose_kind]
    if pose_kind == "rigid":
        assert (poses.astype(np.float32).astype(np.float64) != poses).any()
    want_rows = expected_rows(g, clouds, poses)
    total = want_rows[0].shape[0]
    if s > 0:
        want, want_kept = upload_voxel_raw(g, want_rows, s)
        assert np.array_equal(want_kept, np_voxel.reference(want_rows[0], s))
    else:
        want, want_kept = upload_raw(g, want_rows), np.arange(total, dtype=np.int32)
    got, kept = g.merge_clouds(clouds, poses, s, return_kept=True)
    try:
        assert np.array_equal(kept, want_kept)
        assert_equal_clouds(g, got, want, probe)
        plain = g.merge_clouds(clouds, poses, s)  # (without kept: the same cloud)
        assert plain.n == got.n and np.array_equal(plain.debug_order(), got.debug_order())
        plain.free()
        return want_rows, kept
    finally:
        got.free()
        want.free()
        for c in made or []:
            c.free()


@pytest.mark.parametrize("s", [0.0, LEAF])
@pytest.mark.parametrize("pose_kind", ["none", "identity", "rigid"])
@pytest.mark.parametrize("name", list(LISTS))
def test_merge_equals_the_host_route(gpu, probe, name, pose_kind, s):
    want_rows, kept = merge_case(gpu, probe, LISTS[name], pose_kind, s)
    if name in ("forward", "reversed"):
        assert want_rows[1] is not None and want_rows[2] is not None and want_rows[3] is not None
        if s > 0:  # several voxels hold points of different clouds, and the selection thins
            start = np.cumsum((0,) + LISTS[name])
            owner = np.searchsorted(start, np.arange(want_rows[0].shape[0]), side="right")
            keys = np_voxel.voxel_keys(want_rows[0], s)
            _, inv = np.unique(keys, axis=0, return_inverse=True)
            mixed = sum(1 for v in range(inv.max() + 1) if np.unique(owner[inv.reshape(-1) == v]).shape[0] > 1)
            assert mixed >= 3 and kept.shape[0] < want_rows[0].shape[0]
    if name == "empty":
        assert kept.shape[0] == 0


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("s", [0.0, LEAF])
@pytest.mark.parametrize("pose_kind", ["none", "rigid"])
def test_merge_of_labelled_clouds(gpu, probe, pose_kind, s, soft):
    """Every input with one-hot labels: the merged cloud holds class ids, as the host-built one does; with one soft row per
    input it must not (a mixed list never does: the inputs without labels contribute zero rows).  Which path the kernels
    take shows in the results assert_equal_clouds compares.  The mixed list with a soft row rides along."""
    merge_case(gpu, probe, (7, 256, 300), pose_kind, s, soft=soft, labelled=True)
    if soft:
        merge_case(gpu, probe, LISTS["forward"], pose_kind, s, soft=True)


def test_merge_of_one_handle_twice_keeps_the_first_copy(gpu, probe):
    c = upload_raw(gpu, rows(257, 21, "full"))
    try:
        _, kept = merge_case(gpu, probe, None, "identity", LEAF, clouds=[c, c])
        assert kept.shape[0] > 0 and kept.max() < 257
    finally:
        c.free()


# ---- refusals: the code, a message, *out NULL, no device memory kept ----

def _refused(g, handles, code, s=0.0, n=None):
    arr = (C.c_void_p * max(len(handles), 1))(*handles)
    free0 = g.debug_device_memory()[0]
    h = C.c_void_p(12345)
    rc = g.L.cvo_cloud_merge(g.ctx, len(handles) if n is None else n, arr, None, float(s), C.byref(h), None, None)
    msg = g.L.cvo_last_error(g.ctx).decode()
    assert rc == code and msg and h.value is None, (rc, msg, h.value)
    assert g.debug_device_memory()[0] == free0
    return msg


def test_refusals(gpu):
    a, one, big = upload_raw(gpu, rows(300, 31)), upload_raw(gpu, rows(1, 32)), upload_raw(gpu, rows(4097, 33))
    bad = rows(300, 34)[0].copy()
    bad[123, 1] = np.nan
    nan = upload_raw(gpu, (bad, None, None, None))
    other = CvoGPU(params=cases.load_params("geometric_gpu"))
    foreign = upload_raw(other, rows(50, 35))
    try:
        gpu.merge_clouds([a, a], None, LEAF).free()  # (the context's regions exist from here on: refusals must not grow anything)
        INV, UNS = _capi.CVO_E_INVALID, _capi.CVO_E_UNSUPPORTED
        _refused(gpu, [a.handle], INV, n=0)
        assert "NULL" in _refused(gpu, [a.handle, None], INV)
        assert "another context" in _refused(gpu, [a.handle, foreign.handle], INV)
        for s in (-1.0, float("nan")):
            assert "voxel size" in _refused(gpu, [a.handle], INV, s=s)
        assert "non-finite" in _refused(gpu, [a.handle, nan.handle], INV, s=LEAF)
        assert "4096 clouds" in _refused(gpu, [one.handle] * 4097, UNS)
        assert "2^24" in _refused(gpu, [big.handle] * 4096, UNS)
        ok = gpu.merge_clouds([a, nan], None, 0.0)  # no selection: non-finite rows are no error; the context is as usable as before
        assert ok.n == 600 and ok.debug_order_route() == 0
        ok.free()
    finally:
        for c in (a, one, big, nan, foreign):
            c.free()
        other.close()


# ---- end to end: the poses of a multi-frame solve go straight into the merge ----

def test_multiframe_poses_chain_into_merge():
    from test_gpu_multiframe import _mf_params, _sequence
    P = _mf_params(max_iters=6)
    xyz, gt, X0 = _sequence(3, 300, seed=6)
    g = CvoGPU(params=P)
    try:
        clouds = [upload_raw(g, (np.ascontiguousarray(x, np.float32), None, None, None)) for x in xyz]
        rc, X, info, _, _ = g.multiframe_align_raw(clouds, X0, [1, 0, 0], [0, 1, 1, 2, 0, 2])
        assert rc == 0 and info.outer_iterations > 0 and not np.array_equal(X, np.asarray(X0).reshape(-1))
        leaf = float(P.multiframe_downsample_voxel_size)
        t = upload_raw(g, rows(500, 77))
        want_rows = expected_rows(g, clouds, X.reshape(3, 12))
        want, want_kept = upload_voxel_raw(g, want_rows, leaf / 2)
        got, kept = g.merge_clouds(clouds, X.reshape(3, 12), leaf / 2, return_kept=True)
        assert np.array_equal(kept, want_kept) and 0 < got.n <= 900
        assert_equal_clouds(g, got, want, t)
        for c in clouds + [t, want, got]:
            c.free()
    finally:
        g.close()


# ---- the C++ veneer: CvoGPU::merge / download ----

def test_cpp_veneer_merges_and_downloads():
    """host/cvo_merge_check: two tiny clouds through CvoGPU::merge / download against CvoPointCloud::transform + operator+:
    coordinates within 1 ulp, attributes exactly, kept(0) filled."""
    drv = os.path.join(ROOT, "host", "cvo_merge_check")
    out = subprocess.run([drv, os.path.join(cases.CONFIGS, "outdoor.yaml")], capture_output=True, text=True, timeout=120)
    print(out.stdout + out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = {w[0]: w for w in (line.split() for line in out.stdout.strip().splitlines()) if len(w) == 7}
    assert set(lines) == {"download", "concat", "voxel"}, out.stdout
    for name, points in (("download", 9), ("concat", 14), ("voxel", 1)):
        w = lines[name]
        assert int(w[2]) == points and 0 <= int(w[4]) <= 1 and w[6] == "equal", out.stdout
