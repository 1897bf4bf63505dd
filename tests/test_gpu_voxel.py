"""Voxel-grid downsampling on the MI355X: cvo_voxel_select / cvo_cloud_upload_voxel against the numpy statement
(np_voxel.py) and against an ordinary upload of the kept rows.  Every comparison is exact."""
import os
import subprocess
import warnings

import numpy as np
import pytest

import cases
import np_voxel
from unified_cvo_amd import CvoGPU, CvoPointCloud, CvoError, _capi, read_cvo_params_yaml, synth

pytestmark = pytest.mark.gpu

CASES = np_voxel.cpu_cases()
LARGE = {"scene307200-0.05", "scene307200-0.1", "scene307200-0.25", "scene1000000-0.1", "scan307200-0.1", "own-voxel"}


def _gpu_cases():
    out = list(CASES)
    out.append(("scene1000000-0.1", np_voxel.scene(1000000), 0.1))
    out.append(("scan307200-0.1", np_voxel.scan_order(np_voxel.scene(307200)), 0.1))
    out.append(("scan307200-0.25", np_voxel.scan_order(np_voxel.scene(307200)), 0.25))
    return out


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    yield g
    g.close()


@pytest.mark.parametrize("prepass", [1, 0])
def test_voxel_select_equals_numpy(gpu, prepass):
    """The kernels on every cloud, the small ones included (VOXEL_HOST=0: by default frames below 4096 points take the CPU twin)."""
    gpu.set_option("VOXEL_PREPASS", prepass)
    gpu.set_option("VOXEL_HOST", 0)
    try:
        for name, xyz, s in _gpu_cases():
            want = np_voxel.reference(xyz, s)
            kept = gpu.voxel_select(xyz, s)
            assert kept.dtype == np.int32 and np.array_equal(kept, want), name
            st = gpu.debug_voxel_stats()
            if xyz.shape[0] == 0:
                continue
            assert st["occupied"] == len(kept), (name, st)
            assert st["capacity"] >= 2 * xyz.shape[0] and st["capacity"] & (st["capacity"] - 1) == 0, (name, st)
            assert len(kept) <= st["entered"] <= xyz.shape[0] and st["probes_total"] >= st["entered"], (name, st)
            if not prepass:
                assert st["entered"] == xyz.shape[0], (name, st)
            if name in LARGE:
                assert st["probe_longest"] > 1, (name, st)  # the probing path ran
    finally:
        gpu.set_option("VOXEL_PREPASS", None)
        gpu.set_option("VOXEL_HOST", None)


def test_default_route_by_size(gpu):
    """Unset, VOXEL_HOST sends frames of fewer than 4096 points to the CPU twin (no table) and larger ones to the kernels."""
    for name, xyz, s in _gpu_cases():
        kept = gpu.voxel_select(xyz, s)
        assert np.array_equal(kept, np_voxel.reference(xyz, s)), name
        st = gpu.debug_voxel_stats()
        if xyz.shape[0] < 4096:
            assert st["capacity"] == 0 and st["occupied"] == 0, (name, st)
        else:
            assert st["capacity"] >= 2 * xyz.shape[0] and st["occupied"] == len(kept), (name, st)
    for n in (4095, 4096):
        x = np_voxel.scene(n)
        assert np.array_equal(gpu.voxel_select(x, 0.25), np_voxel.reference(x, 0.25))
        assert (gpu.debug_voxel_stats()["capacity"] == 0) == (n == 4095)


def test_prepass_thins_scan_ordered_frames(gpu):
    """In scan order neighbours share voxels: the block-local table sends a fraction of the points to the table in HBM."""
    x = np_voxel.scan_order(np_voxel.scene(307200))
    kept = gpu.voxel_select(x, 0.25)
    st = gpu.debug_voxel_stats()
    assert len(kept) <= st["entered"] < x.shape[0] // 2, st


def test_host_switch_and_repeats_change_nothing(gpu):
    x = np_voxel.scene(307200)
    first = gpu.voxel_select(x, 0.1)
    for _ in range(10):
        assert np.array_equal(gpu.voxel_select(x, 0.1), first)
    gpu.set_option("VOXEL_HOST", 1)
    try:
        assert np.array_equal(gpu.voxel_select(x, 0.1), first)
        assert gpu.debug_voxel_stats()["capacity"] == 0
        d = gpu.upload_voxel(CvoPointCloud.from_xyz(x), 0.1)
        assert np.array_equal(d.kept, first)
        d.free()
    finally:
        gpu.set_option("VOXEL_HOST", None)


def _clouds(kind, n):
    """A pair of raw frames of one kind, with the parameters that use their attributes."""
    if kind == "xyz":
        p, a, b, init = cases.scene(n)
    elif kind == "colour":
        p, a, b, init = cases.scene_colour(n)
    else:
        p = cases.load_params("semantic_img_gpu0")
        src, fsrc, tgt, ftgt = synth.scene_colour_pair(n)
        ls, lt = synth.checkerboard_labels(src), synth.checkerboard_labels(tgt)
        if kind == "soft":  # rows that are distributions, not one-hot
            ls, lt = (0.9 * ls + 0.1 / synth.NUM_CLASSES).astype(np.float32), (0.9 * lt + 0.1 / synth.NUM_CLASSES).astype(np.float32)
        geo = np.tile(np.array([[0.0, 1.0]], np.float32), (n, 1))
        a, b = CvoPointCloud.from_arrays(src, fsrc, ls, geo), CvoPointCloud.from_arrays(tgt, ftgt, lt, geo)
        init = np.eye(4, dtype=np.float32)
    return p, a, b, init


def _same_results(g, va, vb, ua, ub, init, iterations=40):
    assert np.array_equal(va.debug_order(), ua.debug_order()) and np.array_equal(vb.debug_order(), ub.debug_order())
    r1 = g.align(va, vb, init, max_iterations=iterations, trace_capacity=iterations, trace_dense=iterations)
    r2 = g.align(ua, ub, init, max_iterations=iterations, trace_capacity=iterations, trace_dense=iterations)
    assert r1.iterations == r2.iterations and np.array_equal(r1.transform, r2.transform)
    assert len(r1.trace) == len(r2.trace) > 0
    for t1, t2 in zip(r1.trace, r2.trace):
        for name, _ in _capi.cvo_trace_t._fields_:
            x, y = getattr(t1, name), getattr(t2, name)
            assert (x == y) if isinstance(x, (int, float)) else (list(x) == list(y)), (t1.k, name)
    assert g.inner_product_gpu(va, vb, init, 0.3) == g.inner_product_gpu(ua, ub, init, 0.3)
    c1, c2 = g.compute_association_gpu(va, vb, init, 0.3), g.compute_association_gpu(ua, ub, init, 0.3)
    for x, y in zip(c1, c2):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kind,n,s", [("xyz", 100000, 0.25), ("colour", 100000, 0.25), ("soft", 50000, 0.25),
                                      ("onehot", 50000, 0.25),
                                      ("xyz", 307200, 0.1),   # more than 16 384 survivors: ordered on the host
                                      ("colour", 40, 20.0)])  # fewer than 8: identity order
def test_upload_voxel_is_an_upload_of_the_kept_rows(kind, n, s):
    p, a, b, init = _clouds(kind, n)
    g = CvoGPU(params=p)
    try:
        va, vb = g.upload_voxel(a, s), g.upload_voxel(b, s)
        for v, pc in ((va, a), (vb, b)):
            assert np.array_equal(v.kept, np_voxel.reference(pc.positions(), s)) and v.n == len(v.kept)
        if n == 307200:
            assert va.n > 16384
        if n == 40:
            assert 0 < va.n < 8 and 0 < vb.n < 8
        ua, ub = g.upload(a.select(va.kept)), g.upload(b.select(vb.kept))
        _same_results(g, va, vb, ua, ub, init)
    finally:
        g.close()


def test_multiframe_on_voxel_uploaded_frames():
    from test_gpu_multiframe import _mf_params, _sequence
    xyz, gt, X0 = _sequence(4, 100000, seed=2)
    g = CvoGPU(params=_mf_params(max_iters=8))
    try:
        pcs = [CvoPointCloud.from_xyz(x) for x in xyz]
        vox = [g.upload_voxel(pc, 0.25) for pc in pcs]
        sub = [g.upload(pc.select(np_voxel.reference(pc.positions(), 0.25))) for pc in pcs]
        edges = [0, 1, 1, 2, 2, 3, 0, 2]
        hold = [1, 0, 0, 0]
        cap = 12
        rc1, P1, i1, rows1, n1 = g.multiframe_align_raw(vox, X0, hold, edges, trace_capacity=cap)
        rc2, P2, i2, rows2, n2 = g.multiframe_align_raw(sub, X0, hold, edges, trace_capacity=cap)
        assert rc1 == rc2 == 0 and n1 == n2 > 0 and i1.solves == i2.solves > 0
        assert np.array_equal(P1, P2) and not np.array_equal(P1, np.asarray(X0).reshape(-1))
        for k in range(n1):
            for name, _ in _capi.cvo_multiframe_trace_t._fields_:
                assert getattr(rows1[k], name) == getattr(rows2[k], name), (k, name)
    finally:
        g.close()


def test_voxel_size_defaults_to_the_yaml_value():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P = read_cvo_params_yaml(os.path.join(cases.GOLDEN, "cvo_params", "cvo_intensity_params_irls_tum.yaml"))
    assert P.multiframe_downsample_voxel_size == pytest.approx(0.1)
    g = CvoGPU(params=P)
    try:
        x = np_voxel.scene(50000)
        want = np_voxel.reference(x, np.float32(0.1))
        assert np.array_equal(g.voxel_select(x), want)
        d = g.upload_voxel(CvoPointCloud.from_xyz(x))
        assert np.array_equal(d.kept, want)
    finally:
        g.close()


def test_refusals_leave_the_context_usable():
    p, a, b, init = cases.config2(n=2000)
    g = CvoGPU(params=p)
    try:
        before = g.align(a, b, init, max_iterations=30)
        x0 = np_voxel.scene(100000)
        n = x0.shape[0]
        for where in (0, n // 2, n - 1):
            for value in (np.nan, np.inf):
                x = x0.copy()
                x[where, 1] = value
                with pytest.raises(CvoError, match=f"point {where} has a non-finite"):
                    g.voxel_select(x, 0.25)
                with pytest.raises(CvoError, match="non-finite"):
                    g.upload_voxel(CvoPointCloud.from_xyz(x), 0.25)
        for axis, letter in enumerate("xyz"):
            x = x0.copy()
            x[777, axis] = (2.0 ** 20) * 0.25
            with pytest.raises(CvoError, match=f"point 777: {letter} = .*1048576"):
                g.voxel_select(x, 0.25)
        for s in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(CvoError, match="voxel size"):
                g.voxel_select(x0, s)
        # nothing is written on a refusal
        L = g.L
        import ctypes as C
        x = x0.copy()
        x[5, 0] = np.nan
        kept = np.full(n, -7, np.int32)
        nk = C.c_int(-7)
        h = C.c_void_p(0)
        ipp = C.POINTER(C.c_int)
        fp = C.POINTER(C.c_float)
        rc = L.cvo_voxel_select(g.ctx, n, x.ctypes.data_as(fp), 0.25, kept.ctypes.data_as(ipp), C.byref(nk))
        assert rc == _capi.CVO_E_INVALID and nk.value == -7 and np.all(kept == -7)
        rc = L.cvo_cloud_upload_voxel(g.ctx, n, x.ctypes.data_as(fp), None, None, None, 0.25, C.byref(h), kept.ctypes.data_as(ipp), C.byref(nk))
        assert rc == _capi.CVO_E_INVALID and nk.value == -7 and np.all(kept == -7) and not h.value
        rc = L.cvo_voxel_select(g.ctx, 2 ** 24 + 1, x.ctypes.data_as(fp), 0.25, kept.ctypes.data_as(ipp), C.byref(nk))
        assert rc == _capi.CVO_E_UNSUPPORTED and nk.value == -7
        # empty cloud: accepted
        e = g.upload_voxel(CvoPointCloud.from_xyz(np.zeros((0, 3), np.float32)), 0.25)
        assert e.n == 0 and len(e.kept) == 0 and len(g.voxel_select(np.zeros((0, 3), np.float32), 0.25)) == 0
        after = g.align(a, b, init, max_iterations=30)
        assert np.array_equal(before.transform, after.transform)
        assert np.array_equal(g.voxel_select(x0, 0.25), np_voxel.reference(x0, 0.25))
    finally:
        g.close()


def test_upload_voxel_while_a_queue_is_open():
    pairs = [cases.config2(n=3000, pair_id=k) for k in range(4)]
    g = CvoGPU(params=pairs[0][0])
    try:
        solo = [g.align(a, b, init, max_iterations=200).transform for _, a, b, init in pairs]
        src = [g.upload(a) for _, a, _, _ in pairs]
        tgt = [g.upload(b) for _, _, b, _ in pairs]
        raw = CvoPointCloud.from_xyz(np_voxel.scene(307200))
        q = g.open_queue(4, 3000, 3000, max_iterations=200)
        try:
            for k in range(4):
                q.submit(src[k], tgt[k], pairs[k][3])
            q.poll(wait=0)
            v = g.upload_voxel(raw, 0.25)  # between submit and poll, same thread
            assert np.array_equal(v.kept, np_voxel.reference(raw.positions(), 0.25))
            res = []
            while q.pending():
                res.extend(q.poll(wait=2))
        finally:
            q.close()
        assert [r.ticket for r in res] == [0, 1, 2, 3]
        for r, T in zip(res, solo):
            assert np.array_equal(r.transform, T)
        u = g.upload(raw.select(v.kept))
        assert np.array_equal(u.debug_order(), v.debug_order())
    finally:
        g.close()


def test_device_memory_returns_after_close():
    import gc
    probe = CvoGPU(params=cases.load_params("geometric_gpu"))  # (hipMemGetInfo through the C-ABI)
    pc = CvoPointCloud.from_xyz(np_voxel.scene(1000000))
    seen = []

    def cycle():
        g = CvoGPU(params=cases.load_params("geometric_gpu"))
        d = g.upload_voxel(pc, 0.1)
        seen.append(probe.debug_device_memory()[0])
        d.free()
        g.close()
        del g, d
        gc.collect()

    try:
        for _ in range(2):  # (the runtime's own pools and the stream pool come up during the first cycles)
            cycle()
        free0 = probe.debug_device_memory()[0]
        for _ in range(3):
            cycle()
            assert seen[-1] < free0 - 30 * pc.num_points()  # the scratch region (~44 bytes per point) was resident
            assert probe.debug_device_memory()[0] == free0
    finally:
        probe.close()


def test_multiframe_driver_voxel_matches_python(tmp_path):
    from test_cpp_host import _write_pcd, HOST
    from test_gpu_multiframe import _sequence
    xyz, gt, X0 = _sequence(4, 60000, seed=11)
    rgb = np.full((60000, 3), 128, np.uint8)
    yaml = tmp_path / "mf.yaml"
    text = open(os.path.join(cases.CONFIGS, "geometric_gpu.yaml")).read()
    yaml.write_text(text + "\nmultiframe_ell_init: 0.3\nmultiframe_ell_min: 0.1\nmultiframe_ell_decay_rate: 0.7\n"
                    "multiframe_num_neighbors: 64\nmultiframe_max_iters: 6\nmultiframe_iterations_per_ell: 3\n"
                    "multiframe_iterations_per_solve: 8\nmultiframe_min_nonzeros: 300\nmultiframe_downsample_voxel_size: 0.3\n")
    hold = [1, 0, 0, 0]
    lines = []
    for f in range(4):
        _write_pcd(tmp_path / f"f{f}.pcd", xyz[f], rgb)
        lines.append(f"{tmp_path / f'f{f}.pcd'} {hold[f]} " + " ".join(repr(float(v)) for v in X0[f]))
    (tmp_path / "frames.txt").write_text("\n".join(lines) + "\n")
    edges = [(0, 1), (1, 2), (2, 3), (0, 2)]
    (tmp_path / "edges.txt").write_text("".join(f"{a} {b}\n" for a, b in edges))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        P = read_cvo_params_yaml(str(yaml))
    for args, size in ((["--voxel"], None), (["--voxel", "0.25"], 0.25)):
        out = subprocess.check_output([os.path.join(HOST, "cvo_multiframe_align"), str(yaml), str(tmp_path / "frames.txt"),
                                       str(tmp_path / "edges.txt")] + args, text=True, timeout=300)
        cpp = np.array([[float(v) for v in l.split()[2:]] for l in out.splitlines() if l.startswith("pose ")])
        cpp_kept = [int(l.split()[2]) for l in out.splitlines() if l.startswith("kept ")]
        g = CvoGPU(params=P)
        try:
            pcs = [CvoPointCloud.from_xyzrgb(x, rgb) for x in xyz]
            vox = [g.upload_voxel(pc, size) for pc in pcs]
            assert cpp_kept == [v.n for v in vox]
            rc, X, info, _, _ = g.multiframe_align_raw(vox, X0, hold, [i for e in edges for i in e])
            assert rc == 0 and info.solves > 0
            assert np.array_equal(cpp.reshape(-1), X)
        finally:
            g.close()
