"""The read side of the semantic voxel map on the device: k_bki_query, k_bki_raycast and k_bki_render (cvo_k_bki_query.h)
against the statement (np_bki_query.py), bit for bit, on every case of bki_query_cases.py, on maps filled by the device
inserts (BKI_HOST=0); cvo_map_query_cloud against cvo_map_query of the downloaded, host-moved rows; a map of the host side
under a device context; the table untouched by any number of reads; the same bits on every run; the refusals."""
import ctypes as C

import numpy as np
import pytest

import bki_cases as bc
import bki_query_cases as qc
import cases
import np_bki_query as nq
import unified_cvo_amd as u
from unified_cvo_amd import CvoGPU, CvoPointCloud, _capi

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))  # one context across the cases
    g.set_option("BKI_HOST", 0)
    yield g
    g.close()


def device_map(gpu, name):
    c = qc.case(name)
    return qc.fill(gpu.map_open(u.MapConfig(**qc.config_kwargs(c.cfg)), initial_voxels=c.initial_voxels), c)


def pose(a=0.3, t=(0.5, -0.25, 0.125)):
    return np.array([[np.cos(a), -np.sin(a), 0, t[0]], [np.sin(a), np.cos(a), 0, t[1]], [0, 0, 1, t[2]]], F32)


def raw_keys(gpu, m):
    """the table's key array slot by slot (cvo_debug_map_stats)"""
    cap = m.debug_stats()["capacity"]
    keys = np.zeros(cap, np.uint64)
    gpu._check(gpu.L.cvo_debug_map_stats(m.handle, None, None, keys.ctypes.data_as(C.POINTER(C.c_ulonglong)), None, None))
    return keys


# ---- 1. the kernels equal the statement ----
@pytest.mark.parametrize("name", qc.names())
def test_kernels_equal_the_statement(gpu, name):
    m = device_map(gpu, name)
    stats = m.debug_stats()
    assert stats["on_device"] == (1 if qc.case(name).frames else 0), name
    assert stats["voxels"] == len(qc.expected(name)["map"].voxels)
    diff = qc.differences(m, name)
    m.close()
    assert not diff, "\n".join(diff)


def test_probe_chains_wrap_past_the_tables_end(gpu):
    m = device_map(gpu, "long_chains")
    stats = m.debug_stats()
    assert stats["capacity"] == 32 and stats["growths"] == 0 and stats["longest_probe"] >= 5
    keys = raw_keys(gpu, m)
    live = np.flatnonzero(keys != nq.NO_KEY)
    home = np.array([qc.key_mix(int(k)) & 31 for k in keys[live]])
    assert ((home == 31) & (live < 8)).sum() >= 4  # four of the five voxels of home slot 31 sit behind the table's end
    assert not qc.differences(m, "long_chains")
    m.close()


def test_growth_rehashes_and_the_answers_stay(gpu):
    c = qc.case("growth_after")
    m = gpu.map_open(u.MapConfig(**qc.config_kwargs(c.cfg)), initial_voxels=0)
    xyz, feat, label, origin = c.frames[0]
    m.insert((xyz, feat, label), origin=origin)
    assert not qc.differences(m, "growth_before")
    before = m.debug_stats()
    xyz, feat, label, origin = c.frames[1]
    m.insert((xyz, feat, label), origin=origin)
    after = m.debug_stats()
    assert after["growths"] > before["growths"] and after["capacity"] > before["capacity"]
    assert not qc.differences(m, "growth_after")
    m.close()


# ---- 2. a resident cloud's rows ----
def wide(label):
    out = np.zeros((label.shape[0], 19), F32)
    out[:, :label.shape[1]] = label
    return out


@pytest.mark.parametrize("with_labels", [True, False])
@pytest.mark.parametrize("T", [None, pose(), pose(-1.1, (3.0, 0.5, -2.0))])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_query_cloud_equals_query_of_the_moved_rows(gpu, n, T, with_labels):
    m = device_map(gpu, "classes_19")
    rng = np.random.default_rng(n)
    xyz = rng.uniform(-6, 6, (n, 3)).astype(F32)
    xyz[::4] = qc.case("classes_19").points[:len(xyz[::4])]
    feat, label = bc.rows(rng, n, 19)
    cloud = gpu.upload(CvoPointCloud.from_arrays(xyz, feat, wide(label)) if with_labels else CvoPointCloud.from_arrays(xyz))
    down = cloud.download().positions_
    assert np.array_equal(qc.raw(down), qc.raw(xyz))
    moved = down if T is None else nq.move(T, down)
    got, host_route = m.query(cloud, pose=T), m.query(moved)
    want = nq.query(qc.expected("classes_19")["map"], moved)
    assert qc.first_difference(got, want, qc.QUERY_FIELDS) is None and qc.first_difference(host_route, want, qc.QUERY_FIELDS) is None
    assert (got.found == nq.FOUND).sum() >= (n + 3) // 4 if T is None else True
    cloud.free()
    m.close()


def test_query_of_an_empty_cloud_and_of_no_points(gpu):
    m = device_map(gpu, "classes_1")
    cloud = gpu.upload(CvoPointCloud.from_arrays(np.zeros((0, 3), F32)))
    assert m.query(cloud, pose=pose()).found.shape == (0,) and m.query(np.zeros((0, 3), F32)).probs.shape == (0, 2)
    assert m.raycast(np.zeros((0, 3), F32), np.zeros((0, 3), F32)).status.shape == (0,)
    cloud.free()
    m.close()


# ---- 3. a map of the host side, an undecided map ----
def test_host_side_map_under_a_device_context():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    g.set_option("BKI_HOST", 1)
    for name in ("classes_19", "sparse", "wall", "room"):
        m = device_map(g, name)
        assert m.debug_stats()["on_device"] == 0
        assert not qc.differences(m, name)
        m.close()
    m = device_map(g, "classes_19")
    xyz = qc.case("classes_19").points[:300]
    cloud = g.upload(CvoPointCloud.from_arrays(xyz))
    for T in (None, pose()):
        moved = xyz if T is None else nq.move(T, xyz)
        assert qc.first_difference(m.query(cloud, pose=T), nq.query(qc.expected("classes_19")["map"], moved), qc.QUERY_FIELDS) is None
    cloud.free()
    m.close()
    g.close()


def test_an_undecided_map_answers_without_choosing_a_side():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    g.set_option("BKI_HOST", -1)
    for name in ("empty", "empty_prior"):
        m = device_map(g, name)
        assert not qc.differences(m, name)
        cloud = g.upload(CvoPointCloud.from_arrays(qc.case(name).points[:2]))
        assert qc.first_difference(m.query(cloud), nq.query(qc.expected(name)["map"], qc.case(name).points[:2]), qc.QUERY_FIELDS) is None
        cloud.free()
        stats = m.debug_stats()
        assert stats["capacity"] == 0 and stats["voxels"] == 0 and stats["on_device"] == 0
        m.close()
    # ... and its first insert still decides: 2500 training points take the device
    cfg, frames = bc.scattered(51, 2500, C=3, spread=20.0, free_resolution=1e4)
    m = g.map_open(u.MapConfig(**cfg.kwargs()))
    assert (m.query(frames[0][0]).found == nq.ABSENT).all()
    xyz, feat, label, origin = frames[0]
    m.insert((xyz, feat, label), origin=origin)
    assert m.debug_stats()["on_device"] == 1 and (m.query(xyz).found == nq.FOUND).all()
    m.close()
    g.close()


# ---- 4. reads leave the table alone; the same bits on every run ----
@pytest.mark.parametrize("name", ["classes_19", "sparse", "room"])
def test_reads_leave_the_table_alone_and_repeat(gpu, name):
    m, c = device_map(gpu, name), qc.case(name)
    before, before_keys = m.debug_stats(readback=True), raw_keys(gpu, m)
    first = (m.query(c.points), [m.raycast(o, e, stop=mask, max_steps=steps) for o, e, mask, steps in c.rays],
             [m.render(stop=v["stop_mask"], **{k: v[k] for k in v if k != "stop_mask"}) for v in c.views])
    for _ in range(3):
        again = (m.query(c.points), [m.raycast(o, e, stop=mask, max_steps=steps) for o, e, mask, steps in c.rays],
                 [m.render(stop=v["stop_mask"], **{k: v[k] for k in v if k != "stop_mask"}) for v in c.views])
        for a, b in zip([first[0]] + first[1] + first[2], [again[0]] + again[1] + again[2]):
            for x, y in zip(a, b):
                assert np.array_equal(qc.raw(x), qc.raw(y))
    after = m.debug_stats(readback=True)
    assert np.array_equal(before_keys, raw_keys(gpu, m))  # slot by slot
    for k in ("keys", "ms", "fs"):
        assert np.array_equal(qc.raw(before[k]), qc.raw(after[k])), k
    for k in ("capacity", "growths", "voxels"):
        assert before[k] == after[k]
    # an insert behind them still equals the statement (its counters started from zero)
    xyz, feat, label, origin = c.frames[0]
    m.insert((xyz, feat, label), origin=origin)
    stat = c.statement_map()
    stat.insert(xyz, feat, label, origin)
    assert bc.first_difference(m.debug_stats(readback=True), stat.table()) is None
    m.close()


def test_every_plane_null_in_turn(gpu):
    m, v = device_map(gpu, "room"), dict(qc.case("room").views[2])
    mask, want = v.pop("stop_mask"), qc.expected("room")["views"][2]
    for leave in qc.VIEW_FIELDS:
        view = m.render(stop=mask, planes=tuple(p for p in qc.VIEW_FIELDS if p != leave), **v)
        assert getattr(view, leave) is None and qc.first_difference(view, want, qc.VIEW_FIELDS) is None
    L, T = gpu.L, np.ascontiguousarray(v["pose"], F32)
    assert L.cvo_map_render(m.handle, T.ctypes.data_as(C.POINTER(C.c_float)), 8.0, 8.0, 3.5, 3.5, 7, 9, 6.0, 2, None) == 0
    q = _capi.cvo_map_query_out_t()
    centre = np.zeros((len(qc.case("room").points), 3), F32)
    q.centre = centre.ctypes.data
    pts = qc.case("room").points
    assert L.cvo_map_query(m.handle, len(pts), pts.ctypes.data_as(C.POINTER(C.c_float)), C.byref(q)) == 0
    assert np.array_equal(qc.raw(centre), qc.raw(qc.expected("room")["query"]["centre"]))
    m.close()
    # the ray cast's table: no output at all, then each output alone
    m, (o, e, mask, steps) = device_map(gpu, "wall"), qc.case("wall").rays[0]
    o, e = np.ascontiguousarray(np.broadcast_to(np.asarray(o, F32), np.shape(e))), np.ascontiguousarray(e, F32)
    fp, want = C.POINTER(C.c_float), m.raycast(o, e, stop=mask, max_steps=steps)
    assert qc.first_difference(want, qc.expected("wall")["rays"][0], qc.RAY_FIELDS) is None
    assert L.cvo_map_raycast(m.handle, len(e), o.ctypes.data_as(fp), e.ctypes.data_as(fp), mask, steps, None) == 0
    for field in qc.RAY_FIELDS:
        one, r = np.zeros_like(getattr(want, field)), _capi.cvo_map_ray_out_t()
        setattr(r, field, one.ctypes.data)
        assert L.cvo_map_raycast(m.handle, len(e), o.ctypes.data_as(fp), e.ctypes.data_as(fp), mask, steps, C.byref(r)) == 0
        assert np.array_equal(qc.raw(one), qc.raw(getattr(want, field))), field
    m.close()


# ---- 5. refusals ----
def test_refusals(gpu):
    L = gpu.L
    m = device_map(gpu, "one_hit_occupied")
    before = m.debug_stats(readback=True)
    xyz = bc.f32(0, 0, 0, 1, 1, 1).reshape(2, 3)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    inv = _capi.CVO_E_INVALID

    def text():
        return L.cvo_last_error(gpu.ctx).decode()

    assert L.cvo_map_query(None, 2, fp(xyz), None) == inv
    assert L.cvo_map_query(m.handle, -1, fp(xyz), None) == inv and text().startswith("cvo_map_query:")
    assert L.cvo_map_query(m.handle, 2, None, None) == inv and text().startswith("cvo_map_query:")
    assert L.cvo_map_query(m.handle, 0, None, None) == 0
    assert L.cvo_map_query_host(m.handle, 2, fp(xyz), None) == inv and text().startswith("cvo_map_query_host:")
    assert L.cvo_map_raycast(m.handle, 2, fp(xyz), fp(xyz), 2, 0, None) == inv and text().startswith("cvo_map_raycast:")
    assert L.cvo_map_raycast(m.handle, 2, fp(xyz), fp(xyz), 2, (1 << 20) + 1, None) == inv
    assert L.cvo_map_raycast(m.handle, 2, None, fp(xyz), 2, 10, None) == inv and L.cvo_map_raycast(m.handle, -2, fp(xyz), fp(xyz), 2, 10, None) == inv
    assert L.cvo_map_raycast_host(m.handle, 2, fp(xyz), fp(xyz), 2, 10, None) == inv and text().startswith("cvo_map_raycast_host:")
    T = qc.look_along_x()
    assert L.cvo_map_render(m.handle, fp(T), 8.0, 8.0, 3.5, 3.5, 0, 8, 3.0, 2, None) == inv and text().startswith("cvo_map_render:")
    assert L.cvo_map_render(m.handle, fp(T), 8.0, -8.0, 3.5, 3.5, 8, 8, 3.0, 2, None) == inv
    assert L.cvo_map_render(m.handle, fp(T), 8.0, 8.0, 3.5, 3.5, 8, 8, float("inf"), 2, None) == inv
    assert L.cvo_map_render(m.handle, fp(T), 8.0, 8.0, 3.5, 3.5, 4096, 4097, 3.0, 2, None) == _capi.CVO_E_UNSUPPORTED and "2^24" in text()
    bad = T.copy()
    bad[2, 1] = np.inf
    assert L.cvo_map_render(m.handle, fp(bad), 8.0, 8.0, 3.5, 3.5, 8, 8, 3.0, 2, None) == inv and "pose is not finite" in text()
    assert L.cvo_map_render_host(m.handle, fp(T), 8.0, 8.0, 3.5, 3.5, 8, 8, 3.0, 2, None) == inv
    # cvo_map_query_cloud: a cloud of another context, a host map, a pose that is not finite, a NULL cloud
    cloud = gpu.upload(CvoPointCloud.from_arrays(xyz))
    other = CvoGPU(params=cases.load_params("geometric_gpu"))
    foreign = other.upload(CvoPointCloud.from_arrays(xyz))
    assert L.cvo_map_query_cloud(m.handle, foreign.handle, None, None) == inv and "another context" in text() and text().startswith("cvo_map_query_cloud:")
    foreign.free()
    other.close()
    assert L.cvo_map_query_cloud(m.handle, None, None, None) == inv
    assert L.cvo_map_query_cloud(m.handle, cloud.handle, fp(bad), None) == inv and "pose is not finite" in text()
    host = u.map_open_host(u.MapConfig())
    assert L.cvo_map_query_cloud(host.handle, cloud.handle, None, None) == inv and L.cvo_map_query_cloud(None, cloud.handle, None, None) == inv
    host.close()
    assert L.cvo_map_query_cloud(m.handle, cloud.handle, None, None) == 0
    cloud.free()
    after = m.debug_stats(readback=True)
    for k in ("keys", "ms", "fs"):
        assert np.array_equal(qc.raw(before[k]), qc.raw(after[k])), k
    assert not qc.differences(m, "one_hit_occupied")
    m.close()
