"""cvo_cloud_from_device / _many / _aos192 (cvo_ingest.hip, cvo_k_ingest.h) on the MI355X: a cloud built from rows that are
already in device memory is the cloud cvo_cloud_upload makes of the same rows.

Every cloud is built twice - from host arrays, and from the same bytes placed in device memory through
cvo_debug_device_buffer (no second HIP runtime in the process) - and every comparison is equality: orders as integer arrays,
scores as float32 bit patterns, traces as the bytes of their records.  No tolerance anywhere.

The source buffers of every device-built cloud are released before the cloud is used: each comparison is a lifetime check
too; test_cloud_outlives_its_source_arrays overwrites them first."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cases
from test_gpu_kd_order import _gather_case
from unified_cvo_amd import CvoGPU, CvoPointCloud, _capi, synth
from unified_cvo_amd.api import CVO_POINT_DTYPE, cvo_points_from_pointcloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 4097, 16384, 16385)
EYE = np.eye(4, dtype=np.float32)
ELL = 0.3


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    yield g
    g.close()


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def host_cloud(g, xyz, feat=None, label=None, geo=None):
    """cvo_cloud_upload of exactly these arrays (None stays NULL)."""
    arrs = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (xyz, feat, label, geo)]
    h = C.c_void_p()
    g._check(g.L.cvo_cloud_upload(g.ctx, arrs[0].shape[0], *[_fp(a) for a in arrs], C.byref(h)))
    return g._adopt(h, arrs[0].shape[0])


class Placed:
    """Host arrays placed in device memory; released on exit."""

    def __init__(self, g):
        self.g, self.addr = g, []

    def put(self, a):
        self.addr.append(self.g.debug_device_buffer(a))
        return self.addr[-1]

    def rows(self, a):
        """(address, records, stride in bytes) of a 2-D float32 array whose rows are its records."""
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.float32)
        return (self.put(a), a.shape[0], a.strides[0])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.addr:
            self.g.debug_device_release(d)
        self.addr = []
        return False


def device_cloud(g, xyz, feat=None, label=None, geo=None):
    """cvo_cloud_from_device of the same bytes; the source buffers are gone when this returns."""
    with Placed(g) as p:
        if np.asarray(xyz).shape[0] == 0:
            return g.upload_device((0, 0, 12))
        return g.upload_device(p.rows(xyz), p.rows(feat), p.rows(label), p.rows(geo))


def arrays_of(pc):
    """(xyz, feat, label, geo) as CvoPointCloud hands them to an upload."""
    return pc.device_arrays()


def bits(v):
    return np.float32(v).view(np.uint32)


def trace_bytes(res):
    return [bytes(t) for t in res.trace]


NUDGE = synth.warm_start_delta().astype(np.float32)  # (the attribute cases' clouds overlap at the identity: start next to it)


def traced(g, src, tgt, iters=40, init=EYE):
    """Everything a traced align returns, in comparable form; at least three trace rows, or the comparison says little."""
    r = g.align(src, tgt, init, max_iterations=iters, trace_capacity=iters, trace_dense=iters)
    assert len(r.trace) >= 3, len(r.trace)
    return (r.ret, r.iterations, r.transform.tobytes(), trace_bytes(r))


def both(g, arrs):
    return host_cloud(g, *arrs), device_cloud(g, *arrs)


def free(*clouds):
    for c in clouds:
        c.free()


# ---- size classes: the edges of the route rule (8, KD_MAX_POINTS), of a wave, of KD_THREADS / the ingest block ----

@pytest.fixture(scope="module")
def target1024(gpu):
    t = host_cloud(gpu, synth.geometric_pair(1024, 7)[1])
    yield t
    t.free()


@pytest.mark.parametrize("n", SIZES)
def test_size_classes(gpu, target1024, n):
    gpu.write_params(cases.load_params("geometric_gpu"))
    src, tgt, _ = synth.geometric_pair(max(n, 1), 7)
    src = src[:n]
    h, d = both(gpu, (src, None, None, None))
    try:
        assert d.n == h.n == n
        assert np.array_equal(d.debug_order(), h.debug_order())
        if 8 <= n <= 16384:
            assert not np.array_equal(d.debug_order(), np.arange(n))  # (the device did order it)
        ip_h, ip_d = gpu.inner_product_gpu(h, target1024, EYE, ELL), gpu.inner_product_gpu(d, target1024, EYE, ELL)
        print(f"n={n}: inner product host {ip_h!r} device {ip_d!r}")
        assert bits(ip_h) == bits(ip_d)
        if n >= 1023:
            assert ip_h > 0
        if n in (1025, 16385):
            t = host_cloud(gpu, tgt)
            try:
                th, td = traced(gpu, h, t), traced(gpu, d, t)
                assert len(th[3]) == 40 and th == td
            finally:
                t.free()
    finally:
        free(h, d)


# ---- attribute mixes at n = 1025 ----

def _mix(kind):
    """(params, source arrays, target arrays) of an attribute mix; the arrays a mix leaves out are None."""
    n = 1025
    base = {"xyz": "geotype", "feat": "colour", "onehot": "onehot", "soft": "soft", "geotype": "geotype", "onehot_but_one": "onehot"}[kind]
    P, a, b = _gather_case(base, n)
    sa, sb = list(arrays_of(a)), list(arrays_of(b))
    if kind == "xyz":
        P = cases.load_params("geometric_gpu")
        sa[3] = sb[3] = None
    if kind in ("feat", "onehot", "soft", "onehot_but_one"):
        sa[3] = sb[3] = None
    if kind == "onehot_but_one":
        sa[2] = sa[2].copy()
        sa[2][500] = np.float32(1.0 / synth.NUM_CLASSES)
    return P, tuple(sa), tuple(sb)


def _mix_results(g, P, sa, sb, device):
    g.write_params(P)
    make = device_cloud if device else host_cloud
    s, t = make(g, *sa), make(g, *sb)
    try:
        return traced(g, s, t, 20, NUDGE), int(bits(g.function_angle(s, t, EYE, ELL, is_approximate=False)))
    finally:
        free(s, t)


@pytest.mark.parametrize("kind", ["xyz", "feat", "onehot", "soft", "geotype", "onehot_but_one"])
def test_attribute_mixes(gpu, kind):
    P, sa, sb = _mix(kind)
    want = _mix_results(gpu, P, sa, sb, device=False)
    got = _mix_results(gpu, P, sa, sb, device=True)
    assert got == want
    if kind == "onehot":  # the class-id path and the 19-float path: one result, on both routes
        g2 = CvoGPU(params=P)
        try:
            g2.set_option("NO_ONEHOT", "1")
            assert _mix_results(g2, P, sa, sb, device=False) == want
            assert _mix_results(g2, P, sa, sb, device=True) == want
        finally:
            g2.close()


# ---- layouts ----

def _full_case(n=1025, seed=5):
    """A source with every attribute (one-hot labels) and its target, as CvoPointClouds, under the semantic parameters."""
    P, a, b = _gather_case("onehot", n)
    rs = np.random.default_rng(seed)
    ga = np.where(rs.random((n, 1)) < 0.5, [[1.0, 0.0]], [[0.3, 0.9]]).astype(np.float32)
    xyz, feat, label, _ = arrays_of(a)
    return P, (xyz, feat, label, ga), b


def _equal_clouds(g, h, d, tgt):
    assert np.array_equal(d.debug_order(), h.debug_order())
    assert bits(g.inner_product_gpu(h, tgt, EYE, ELL)) == bits(g.inner_product_gpu(d, tgt, EYE, ELL))
    assert traced(g, h, tgt, 10, NUDGE) == traced(g, d, tgt, 10, NUDGE)


def test_aos192_records(gpu):
    P, sa, b = _full_case()
    gpu.write_params(P)
    rec = cvo_points_from_pointcloud(CvoPointCloud.from_arrays(*sa))
    assert rec.dtype == CVO_POINT_DTYPE and rec.dtype.itemsize == 192
    tgt = gpu.upload(b)
    h = gpu.upload_aos192(rec)
    with Placed(gpu) as p:
        d = gpu.upload_device_aos192(p.put(rec), rec.shape[0])
    try:
        _equal_clouds(gpu, h, d, tgt)
    finally:
        free(h, d, tgt)


def test_padded_strides(gpu):
    """xyz rows of 16 bytes, label rows of 80: the padding holds values that must not be read."""
    P, (xyz, feat, label, geo), b = _full_case()
    gpu.write_params(P)
    n = xyz.shape[0]
    x4 = np.full((n, 4), 7.5, np.float32)
    x4[:, :3] = xyz
    l20 = np.full((n, 20), 0.25, np.float32)
    l20[:, :19] = label
    tgt = gpu.upload(b)
    h = host_cloud(gpu, xyz, feat, label, geo)
    with Placed(gpu) as p:
        d = gpu.upload_device((p.put(x4), n, 16), p.rows(feat), (p.put(l20), n, 80), p.rows(geo))
    try:
        _equal_clouds(gpu, h, d, tgt)
    finally:
        free(h, d, tgt)


def test_rows_subset_with_duplicates(gpu):
    P, _, b = _full_case()
    gpu.write_params(P)
    n_records, n = 3000, 1025
    _, a3000, _ = _gather_case("onehot", n_records)
    xyz, feat, label, geo = arrays_of(a3000)
    idx = np.random.default_rng(9).integers(0, n_records, n).astype(np.int32)
    assert len(np.unique(idx)) < n and idx.max() > n                              # duplicates, and records beyond n
    tgt = gpu.upload(b)
    h = host_cloud(gpu, xyz[idx], feat[idx], label[idx], geo[idx])
    with Placed(gpu) as p:
        d = gpu.upload_device(p.rows(xyz), p.rows(feat), p.rows(label), p.rows(geo), rows=(p.put(idx), n), n_records=n_records)
    try:
        assert d.n == n
        _equal_clouds(gpu, h, d, tgt)
    finally:
        free(h, d, tgt)


# ---- non-finite coordinates: no error; ordered on the host (the identity), refused by the solver ----

def _align_rc(g, s, t):
    p, out, info = g.params.to_ctypes(), np.zeros(16, np.float32), _capi.cvo_align_info_t()
    init = np.ascontiguousarray(EYE.T).reshape(16)
    return g.L.cvo_align(g.ctx, C.byref(p), s.handle, t.handle, _fp(init), _fp(out), C.byref(info))


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_coordinates(gpu, target1024, bad):
    gpu.write_params(cases.load_params("geometric_gpu"))
    x = synth.geometric_pair(200, 3)[0].copy()
    x[117, 1] = bad
    h, d = both(gpu, (x, None, None, None))
    try:
        assert np.array_equal(h.debug_order(), np.arange(200)) and np.array_equal(d.debug_order(), h.debug_order())
        rh, rd = _align_rc(gpu, h, target1024), _align_rc(gpu, d, target1024)
        assert rh == rd and rh <= _capi.CVO_E_INVALID
    finally:
        free(h, d)


# ---- route switches ----

@pytest.mark.parametrize("opt,val", [("ORDER", "host"), ("ORDER", "virtual"), ("NO_SORT", "1")])
def test_route_switches(opt, val):
    P, sa, b = _full_case(n=700)
    g = CvoGPU(params=P)
    try:
        g.set_option(opt, val)
        tgt = g.upload(b)
        h, d = both(g, sa)
        assert np.array_equal(d.debug_order(), h.debug_order())
        assert np.array_equal(h.debug_order(), np.arange(700)) == (opt == "NO_SORT")
        assert bits(g.inner_product_gpu(h, tgt, EYE, ELL)) == bits(g.inner_product_gpu(d, tgt, EYE, ELL))
        free(h, d, tgt)
    finally:
        g.close()


# ---- _many ----

def _many_cases():
    """Five clouds: empty, below the route rule, a small one with every attribute, KD_MAX_POINTS with colour, one above it
    with soft labels."""
    rs = np.random.default_rng(41)
    x = {n: synth.geometric_pair(n, 30 + k)[0] for k, n in enumerate((7, 300, 16384, 16385))}
    col = lambda a: synth.colour_features(a, rs).astype(np.float32)
    soft = lambda a: (0.9 * synth.checkerboard_labels(a) + 0.1 / synth.NUM_CLASSES).astype(np.float32)
    geo = lambda n: np.where(rs.random((n, 1)) < 0.5, [[1.0, 0.0]], [[0.3, 0.9]]).astype(np.float32)
    return [
        (np.zeros((0, 3), np.float32), None, None, None),
        (x[7], None, None, None),
        (x[300], col(x[300]), synth.checkerboard_labels(x[300]).astype(np.float32), geo(300)),
        (x[16384], col(x[16384]), None, None),
        (x[16385], col(x[16385]), soft(x[16385]), None),
    ]


def test_many_equals_single_calls(gpu, target1024):
    P = cases.load_params("semantic_img_gpu0")
    gpu.write_params(P)
    clouds = _many_cases()
    with Placed(gpu) as p:
        specs = [((0, 0, 12),) if c[0].shape[0] == 0 else tuple(p.rows(a) for a in c) for c in clouds]
        many = gpu.upload_device_many(specs)
    assert [m.n for m in many] == [0, 7, 300, 16384, 16385]
    for c, m in zip(clouds, many):
        one, h = device_cloud(gpu, *c), host_cloud(gpu, *c)
        try:
            assert np.array_equal(m.debug_order(), one.debug_order()) and np.array_equal(m.debug_order(), h.debug_order())
            want = bits(gpu.inner_product_gpu(h, target1024, EYE, ELL))
            assert bits(gpu.inner_product_gpu(m, target1024, EYE, ELL)) == want
            assert bits(gpu.inner_product_gpu(one, target1024, EYE, ELL)) == want
        finally:
            free(one, h, m)


def test_align_batch_over_device_built_clouds(gpu):
    gpu.write_params(cases.load_params("geometric_gpu"))
    pairs = [synth.geometric_pair(n, 50 + k)[:2] for k, n in enumerate((900, 1025, 2000))]
    with Placed(gpu) as p:
        dev = gpu.upload_device_many([(p.rows(a),) for pr in pairs for a in pr])
    host = [host_cloud(gpu, a) for pr in pairs for a in pr]
    try:
        rd = gpu.align_batch(dev[0::2], dev[1::2], [EYE] * 3, max_iterations=30)
        rh = gpu.align_batch(host[0::2], host[1::2], [EYE] * 3, max_iterations=30)
        for a, b in zip(rd, rh):
            assert a.iterations == b.iterations == 30 and a.ret == b.ret
            assert a.transform.tobytes() == b.transform.tobytes()
    finally:
        free(*dev, *host)


# ---- refusals: CVO_E_INVALID, a message, *out NULL, no device memory kept ----

def _refused(g, d):
    free0 = g.debug_device_memory()[0]
    h = C.c_void_p(12345)
    rc = g.L.cvo_cloud_from_device(g.ctx, C.byref(d), C.byref(h))
    msg = g.L.cvo_last_error(g.ctx).decode()
    assert rc == _capi.CVO_E_INVALID and msg and h.value is None, (rc, msg, h.value)
    assert g.debug_device_memory()[0] == free0
    return msg


def _rows_t(n, n_records, xyz, stride=12, rows=None):
    return _capi.cvo_device_rows_t(n, n_records, xyz, stride, None, 0, None, 0, None, 0, rows)


def test_refusals(gpu):
    n = 300
    x = synth.geometric_pair(n, 2)[0]
    with Placed(gpu) as p:
        dx = p.put(x)
        ok = gpu.upload_device((dx, n, 12))  # (the context's ingest region exists from here on: refusals must not grow anything)
        ok.free()
        keep = np.ascontiguousarray(x)
        assert "not device memory" in _refused(gpu, _rows_t(n, n, keep.ctypes.data))          # a host pointer
        assert "aligned" in _refused(gpu, _rows_t(n - 1, n - 1, dx + 2))                      # a misaligned pointer
        assert "stride" in _refused(gpu, _rows_t(n, n, dx, stride=8))
        assert "n_records" in _refused(gpu, _rows_t(n, n - 1, dx))
        assert "allocation" in _refused(gpu, _rows_t(n + 100000, n + 100000, dx))             # records beyond the buffer's end
        # a row index outside [0, n_records): found by the kernel, which clamps the read BEFORE the load - nothing out of
        # bounds is touched, which is why this case is safe to run
        for bad in (n, -1):
            idx = np.arange(n, dtype=np.int32)[::-1].copy()
            idx[41] = bad
            msg = _refused(gpu, _rows_t(n, n, dx, rows=p.put(idx)))
            assert "rows[41]" in msg, msg
        again = gpu.upload_device((dx, n, 12))  # the context is as usable as before
        assert again.n == n
        again.free()


# ---- lifetime ----

def test_cloud_outlives_its_source_arrays(gpu):
    P, sa, b = _full_case()
    gpu.write_params(P)
    tgt = gpu.upload(b)
    h = host_cloud(gpu, *sa)
    with Placed(gpu) as p:
        specs = [p.rows(a) for a in sa]
        d = gpu.upload_device(*specs)
        for (addr, _, _), a in zip(specs, sa):
            gpu.debug_device_buffer(np.full(a.shape, 1e9, np.float32), into=addr)           # overwritten, then released
    try:
        assert traced(gpu, d, tgt, 20, NUDGE) == traced(gpu, h, tgt, 20, NUDGE)
    finally:
        free(h, d, tgt)


# ---- a downstream consumer: 3-frame multi-frame align at 600 points ----

def test_multiframe_over_device_built_clouds():
    from test_gpu_multiframe import _mf_params, _sequence
    P = _mf_params(max_iters=6)
    xyz, gt, X0 = _sequence(3, 600, seed=6)
    g = CvoGPU(params=P)
    try:
        host = [host_cloud(g, x) for x in xyz]
        dev = [device_cloud(g, x) for x in xyz]
        edges = [0, 1, 1, 2, 0, 2]
        rc_h, X_h, info_h, _, _ = g.multiframe_align_raw(host, X0, [1, 0, 0], edges)
        rc_d, X_d, info_d, _, _ = g.multiframe_align_raw(dev, X0, [1, 0, 0], edges)
        assert rc_h == rc_d == 0 and info_h.outer_iterations == info_d.outer_iterations > 0
        assert not np.array_equal(X_h, np.asarray(X0).reshape(-1)) and X_h.tobytes() == X_d.tobytes()
        free(*host, *dev)
    finally:
        g.close()


# ---- the C++ veneer: CvoGPU::upload_device / upload_device_aos192 ----

def test_cpp_veneer_matches_the_pcl_overload(tmp_path):
    """host/cvo_device_rows_check: the demo clouds as CvoPoint records, uploaded from host memory (the pcl overload), from
    device memory as records and as four strided arrays: one inner product, three times the same bits."""
    from test_cpp_host import _write_pcd
    drv = os.path.join(ROOT, "host", "cvo_device_rows_check")
    sx, sr, tx, tr = cases.demo_clouds()
    _write_pcd(tmp_path / "source.pcd", sx, sr)
    _write_pcd(tmp_path / "target.pcd", tx, tr)
    out = subprocess.check_output([drv, str(tmp_path / "source.pcd"), str(tmp_path / "target.pcd"),
                                   os.path.join(cases.CONFIGS, "outdoor.yaml"), "2.5"], text=True, timeout=120)
    rows = {w[0]: (float(w[1]), w[2]) for w in (line.split() for line in out.strip().splitlines())}
    assert set(rows) == {"host", "aos192", "strided"}, out
    assert rows["host"][0] > 0 and rows["aos192"][1] == rows["host"][1] and rows["strided"][1] == rows["host"][1], out


# ---- torch tensors: one child process, torch first and the library afterwards, as bench.py does ----

TORCH_CHILD = r"""
import sys
import numpy as np
import torch
if not torch.cuda.is_available():
    print("NO_DEVICE")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
from unified_cvo_amd import CvoGPU, CvoPointCloud, synth
import cases
n = 1500
P = cases.load_params("semantic_img_gpu0")
src, fsrc, lsrc, tgt, ftgt, ltgt = synth.semantic_pair(n, 3)
lsrc = (0.8 * lsrc + 0.2 / synth.NUM_CLASSES).astype(np.float32)
g = CvoGPU(params=P)
t = g.upload(CvoPointCloud.from_arrays(tgt, ftgt, ltgt))
h = g.upload(CvoPointCloud.from_arrays(src, fsrc, lsrc))
dev = torch.device("cuda", 0)
wide = torch.zeros((n, 32), dtype=torch.float32, device=dev)
wide[:, 5:24] = torch.from_numpy(np.ascontiguousarray(lsrc, np.float32)).to(dev)
label = wide[:, 5:24]                                     # a column slice: row stride 128 bytes, not contiguous
assert not label.is_contiguous()
geo = torch.from_numpy(CvoPointCloud.from_arrays(src, fsrc, lsrc).device_arrays()[3]).to(dev)
d = g.upload_device(torch.from_numpy(src).to(dev), torch.from_numpy(np.ascontiguousarray(fsrc, np.float32)).to(dev), label, geo)
eye = np.eye(4, dtype=np.float32)
a, b = np.float32(g.inner_product_gpu(h, t, eye, 0.3)), np.float32(g.inner_product_gpu(d, t, eye, 0.3))
print("RESULT", int(a.view(np.uint32)), int(b.view(np.uint32)), float(a))
"""


def test_torch_tensors_in_a_child_process(tmp_path):
    script = tmp_path / "torch_child.py"
    script.write_text(TORCH_CHILD)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    out = subprocess.run([sys.executable, str(script), ROOT], capture_output=True, text=True, timeout=240, env=env)
    if "NO_DEVICE" in out.stdout:
        pytest.skip("torch sees no device")
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()
    assert line[1] == line[2] and float(line[3]) > 0, line
