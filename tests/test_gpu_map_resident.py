"""Resident clouds into the semantic voxel map and out of it on the device: cvo_map_insert_cloud (k_bki_stage in front of the
six insert kernels) against the host route - cvo_cloud_download, then cvo_map_insert_posed / cvo_map_insert - and against the
statement (np_bki.py), bit for bit on keys, ms and fs; cvo_map_cloud_resident (k_bki_rows at the ingest's padded stride, then
cvo_cloud_from_device's body) against the cloud cvo_map_cloud(..., &resident) uploads: rows, spatial order, scores, solves.
Row counts on both sides of the stage tile and of BKI_THREADS, every class count that changes the staged row, every kind of
resident cloud, the refusals, the side rule at its crossover, and the loop frame -> align -> insert -> read-out."""
import numpy as np
import pytest

import bki_cases as bc
import cases
import np_bki
import test_gpu_ingest as ing
import unified_cvo_amd as u
from unified_cvo_amd import CvoGPU, CvoPointCloud, _capi

pytestmark = pytest.mark.gpu

F32 = np.float32
HOST_BELOW = 2129  # BKI_HOST_BELOW (cvo_bki.hip): training points of a first insert below which the map takes the host side


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))  # one context across the cases
    g.set_option("BKI_HOST", 0)
    yield g
    g.close()


def pose(a=0.3, t=(0.5, -0.25, 0.125)):
    return np.array([[np.cos(a), -np.sin(a), 0, t[0]], [np.sin(a), np.cos(a), 0, t[1]], [0, 0, 1, t[2]]], F32)


def move(T, xyz):
    """fma(T0, x, T1 * y) + fma(T2, z, T3), as the cloud transform (test_gpu_bki.test_posed_insert_moves_the_rows)"""
    T = np.asarray(T, F32)[:3, :4]
    moved = np.empty_like(xyz)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(3):
            t = T[r].astype(np.float64)
            lo = (t[0] * xyz[:, 0].astype(np.float64) + (T[r, 1] * xyz[:, 1]).astype(np.float64)).astype(F32)
            hi = (t[2] * xyz[:, 2].astype(np.float64) + t[3]).astype(F32)
            moved[:, r] = lo + hi
    return moved


def wide(label, behind=None):
    """label rows of C columns as the 19 of a cloud; behind: a generator that fills the columns behind C"""
    if label is None:
        return None
    out = np.zeros((label.shape[0], 19), F32)
    if behind is not None:
        out[:] = behind.uniform(1.5, 2.0, out.shape)
    out[:, :label.shape[1]] = label
    return out


def host_rows(cloud, C):
    """what cvo_cloud_download returns for the cloud, as the rows of a host insert into a map of C classes"""
    d = cloud.download()
    return d.positions_, d.features_ if d.present & 1 else None, d.labels_[:, :C] if C and d.present & 2 else None


def open_map(gpu, cfg):
    return gpu.map_open(u.MapConfig(**cfg.kwargs()))


def same_tables(a, b, what):
    diff = bc.first_difference(a, (b["keys"], b["ms"], b["fs"]))
    assert diff is None, f"{what}: {diff}"
    for k in ("training", "members", "longest_run", "voxels"):
        assert a[k] == b[k], (what, k, a[k], b[k])


def insert_both(gpu, cfg, cloud, T=None, origin=None, on_device=1, statement=True, what=""):
    """Map A: insert_cloud; map B: insert of the downloaded rows; the statement on the moved rows.  Returns A's stats."""
    C = cfg.num_classes
    A, B = open_map(gpu, cfg), open_map(gpu, cfg)
    A.insert_cloud(cloud, pose=T, origin=origin)
    xyz, feat, label = host_rows(cloud, C)
    if T is not None and origin is None:
        B.insert((xyz, feat, label), pose=T)
    else:
        B.insert((xyz if T is None else move(T, xyz), feat, label), origin=origin)
    sa, sb = A.debug_stats(readback=True), B.debug_stats(readback=True)
    assert sa["on_device"] == on_device == sb["on_device"], what
    same_tables(sa, sb, what)
    if statement:
        stat = np_bki.Map(cfg)
        stat.insert(xyz if T is None else move(T, xyz), feat, label, np.asarray(T, F32)[:3, 3] if origin is None else np.asarray(origin, F32))
        diff = bc.first_difference(sa, stat.table())
        assert diff is None, f"{what}: against the statement: {diff}"
        assert (sa["training"], sa["members"], sa["longest_run"]) == (stat.last["training"], stat.last["members"], stat.last["longest_run"])
    A.close()
    B.close()
    return sa


# ---- 1. the insert equals the host route ----
SIZES = [1, 255, 256, 257, 513]  # both sides of the stage tile (256 rows) and of BKI_THREADS


@pytest.mark.parametrize("with_feat", [True, False])
@pytest.mark.parametrize("C", [0, 3, 19])
@pytest.mark.parametrize("n", SIZES)
def test_insert_equals_the_host_route(gpu, n, C, with_feat):
    cfg, frames = bc.scattered(700 + n, n, C=C)
    xyz, feat, label, _ = frames[0]
    cloud = gpu.upload(CvoPointCloud.from_arrays(xyz, feat if with_feat else None, wide(label)))
    assert (cloud.download().present & 1) == (1 if with_feat else 0)
    insert_both(gpu, cfg, cloud, T=pose(), what=f"n {n} C {C} feat {with_feat}")
    cloud.free()


@pytest.mark.parametrize("C", [3, 19])
@pytest.mark.parametrize("n", SIZES)
def test_one_hot_rows_insert_as_the_host_route(gpu, n, C):
    cfg, frames = bc.scattered(800 + n, n, C=C)
    xyz, feat, _, _ = frames[0]
    rng = np.random.default_rng(n + C)
    label = np.eye(C, dtype=F32)[rng.integers(0, C, n)]  # (the cloud then carries class ids next to the rows)
    cloud = gpu.upload(CvoPointCloud.from_arrays(xyz, feat, wide(label)))
    insert_both(gpu, cfg, cloud, T=pose(0.7, (0.25, 0.5, -0.375)), what=f"one-hot n {n} C {C}")
    cloud.free()


def test_label_tie_goes_to_the_first_maximum(gpu):
    kw, xyz, label, origin = bc.MICRO["label_tie"]
    cfg = np_bki.Config(**kw)
    cloud = gpu.upload(CvoPointCloud.from_arrays(bc.f32(*xyz), np.ones((1, 5), F32), wide(bc.f32(*label))))
    sa = insert_both(gpu, cfg, cloud, T=pose(), what="label_tie")
    assert sa["ms"][:, 2].sum() > sa["ms"][:, 3].sum()  # class 2 (the first 0.75), not class 3
    cloud.free()


def test_columns_behind_the_maps_classes_do_not_matter(gpu):
    cfg, frames = bc.scattered(901, 257, C=3)
    xyz, feat, label, _ = frames[0]
    plain = gpu.upload(CvoPointCloud.from_arrays(xyz, feat, wide(label)))
    noisy = gpu.upload(CvoPointCloud.from_arrays(xyz, feat, wide(label, behind=np.random.default_rng(5))))
    assert (noisy.download().labels_[:, 3:] > label.max()).all()  # (every hidden column would win the arg max)
    a = insert_both(gpu, cfg, plain, T=pose(), what="19 columns, zeros behind 3")
    b = insert_both(gpu, cfg, noisy, T=pose(), what="19 columns, noise behind 3")
    same_tables(a, b, "noise behind the third column")
    plain.free()
    noisy.free()


# ---- 2. every kind of resident cloud ----
def _frame300(seed=31, C=3):
    cfg, frames = bc.scattered(seed, 300, C=C)
    xyz, feat, label, _ = frames[0]
    return cfg, xyz, feat, wide(label)


def test_cloud_ordered_by_k_kd_order(gpu):
    cfg, xyz, feat, label = _frame300()
    cloud = gpu.upload(CvoPointCloud.from_arrays(xyz, feat, label))
    assert cloud.debug_order_route() == 1
    insert_both(gpu, cfg, cloud, T=pose(), what="upload")
    cloud.free()


@pytest.mark.parametrize("order", [None, "wide"])
def test_cloud_of_16385_points(gpu, order):
    cfg, frames = bc.scattered(41, 16385, C=3, spread=40.0, free_resolution=1e4)  # (no beam samples)
    xyz, feat, label, _ = frames[0]
    gpu.set_option("ORDER", order)
    try:
        cloud = gpu.upload(CvoPointCloud.from_arrays(xyz, feat, wide(label)))
        assert cloud.debug_order_route() == (2 if order else 0)
        sa = insert_both(gpu, cfg, cloud, T=pose(), what=f"16385 points, ORDER={order}")
        assert sa["training"] == 16386
        cloud.free()
    finally:
        gpu.set_option("ORDER", None)


def test_cloud_from_device_rows(gpu):
    cfg, xyz, feat, label = _frame300(32)
    cloud = ing.device_cloud(gpu, xyz, feat, label)
    insert_both(gpu, cfg, cloud, T=pose(), what="upload_device")
    cloud.free()


def test_merged_cloud(gpu):
    cfg, xyz, feat, label = _frame300(33)
    parts = [gpu.upload(CvoPointCloud.from_arrays(xyz[:140], feat[:140], label[:140])),
             gpu.upload(CvoPointCloud.from_arrays(xyz[140:], feat[140:], label[140:]))]
    poses = np.stack([pose(0.1).astype(np.float64).reshape(12), pose(-0.2, (1.0, 0.5, 0.0)).astype(np.float64).reshape(12)])
    merged = gpu.merge_clouds(parts, poses, voxel_size=0.7)
    assert 50 < merged.n <= 300
    insert_both(gpu, cfg, merged, T=pose(), what="merge_clouds")
    for c in parts + [merged]:
        c.free()


def test_another_maps_resident_cloud(gpu):
    cfg, frames = bc.three_inserts(C=3)
    src = open_map(gpu, cfg)
    for xyz, feat, label, origin in frames:
        src.insert((xyz, feat, label), origin=origin)
    cloud = src.resident_cloud()
    assert cloud.n > 50 and cloud.download().present == 3
    insert_both(gpu, cfg, cloud, T=pose(), what="another map's resident cloud")
    cloud.free()
    src.close()


# ---- 3. no pose, an origin ----
def test_stored_bits_with_an_origin(gpu):
    cfg, xyz, feat, label = _frame300(34)
    xyz = xyz.copy()
    xyz[::7, 0] = F32(-0.0)
    xyz[3] = bc.f32(-0.0, -0.0, -0.0)
    cloud = gpu.upload(CvoPointCloud.from_arrays(xyz, feat, label))
    assert np.array_equal(bc.bits(cloud.download().positions_), bc.bits(xyz))
    insert_both(gpu, cfg, cloud, origin=(0.125, 0.25, -0.125), what="pose None")
    insert_both(gpu, cfg, cloud, T=pose(), origin=(1.0, -2.0, 0.5), what="a pose and an origin of its own")
    cloud.free()


def test_empty_cloud_inserts_the_origin_alone(gpu):
    cfg = np_bki.Config(resolution=0.5, num_classes=3)
    cloud = gpu.upload(CvoPointCloud.from_arrays(np.zeros((0, 3), F32)))
    sa = insert_both(gpu, cfg, cloud, origin=(1.0, 1.0, 1.0), what="n == 0")
    assert sa["training"] == 1 and sa["voxels"] == 1
    cloud.free()


# ---- 4. refusals leave the map ----
def _refusal(gpu, cfg, good, bad_cloud, T=None, origin=None, code=_capi.CVO_E_INVALID, own_gpu=None):
    """A map holding one good frame refuses the bad insert and stays what the statement holds; returns the text."""
    m, stat = open_map(gpu, cfg), np_bki.Map(cfg)
    xyz, feat, label = host_rows(good, cfg.num_classes)
    m.insert_cloud(good, pose=pose())
    stat.insert(move(pose(), xyz), feat, label, pose()[:, 3])
    before = m.debug_stats(readback=True)
    with pytest.raises(u.CvoError) as err:
        m.insert_cloud(bad_cloud, pose=T, origin=origin)
    text = str(err.value)
    assert str(code) in text and "cvo_map_insert_cloud:" in text, text
    after = m.debug_stats(readback=True)
    for k in ("keys", "ms", "fs"):
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    assert bc.first_difference(after, stat.table()) is None
    assert after["on_device"] == 1
    m.insert_cloud(good, pose=pose(0.1))  # (and goes on working)
    m.close()
    return text.split("cvo_map_insert_cloud: ", 1)[1]


def _host_text(gpu, cfg, cloud, T):
    """the text the host route refuses the same rows with, behind its prefix"""
    m = open_map(gpu, cfg)
    with pytest.raises(u.CvoError) as err:
        m.insert(host_rows(cloud, cfg.num_classes), pose=T)
    m.close()
    return str(err.value).split(": ", 2)[2]


def test_refusals_leave_the_map(gpu):
    cfg, xyz, feat, label = _frame300(35)
    good = gpu.upload(CvoPointCloud.from_arrays(xyz, feat, label))
    # a translation that takes every hit (|x| <= 6) beyond the map's 2^20 blocks per axis
    far = pose(0.0, (0.5 * 524287 + 16.0, 0.0, 0.0))
    text = _refusal(gpu, cfg, good, good, T=far)
    assert text.startswith("hit 0 ") and text == _host_text(gpu, cfg, good, far), text
    # a finite scale that takes a moved coordinate to infinity: 3e38 x is finite for |x| <= 1 and overflows at x = 2
    huge = np.array([[3e38, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F32)
    spiky = xyz.copy()
    spiky[:, 0] = np.clip(spiky[:, 0], -1.0, 1.0)
    spiky[[17, 200, 290], 0] = 2.0
    first = int(np.flatnonzero(~np.isfinite(move(huge, spiky)).all(axis=1))[0])
    assert np.isfinite(huge).all() and first == 17
    spiked = gpu.upload(CvoPointCloud.from_arrays(spiky, feat, label))
    text = _refusal(gpu, cfg, good, spiked, T=huge)
    assert text == "hit 17 has a coordinate that is not finite" == _host_text(gpu, cfg, spiked, huge), text
    # a NaN in the pose, an infinite origin
    nan = pose()
    nan[1, 2] = np.nan
    assert "pose is not finite" in _refusal(gpu, cfg, good, good, T=nan)
    assert "origin is not finite" in _refusal(gpu, cfg, good, good, origin=(0.0, np.inf, 0.0))
    # a labelled map and a cloud without labels
    bare = gpu.upload(CvoPointCloud.from_arrays(xyz, feat))
    assert "needs label rows" in _refusal(gpu, cfg, good, bare, T=pose())
    # a cloud of another context
    other = CvoGPU(params=cases.load_params("geometric_gpu"))
    foreign = other.upload(CvoPointCloud.from_arrays(xyz, feat, label))
    assert "another context" in _refusal(gpu, cfg, good, foreign, T=pose())
    foreign.free()
    other.close()
    # 65 536 beam samples or more
    long_cfg = np_bki.Config(resolution=0.5, num_classes=3, free_resolution=1.0)
    text = _refusal(gpu, long_cfg, good, good, T=pose(), origin=(70000.0, 0.0, 0.0), code=_capi.CVO_E_UNSUPPORTED)
    assert "65536 beam samples" in text, text
    for c in (good, bare, spiked):
        c.free()


def test_both_pointers_null_is_refused_by_the_library(gpu):
    cfg, xyz, feat, label = _frame300(36)
    cloud = gpu.upload(CvoPointCloud.from_arrays(xyz, feat, label))
    m = open_map(gpu, cfg)
    assert gpu.L.cvo_map_insert_cloud(m.handle, cloud.handle, None, None) == _capi.CVO_E_INVALID
    assert gpu.L.cvo_last_error(gpu.ctx).decode().startswith("cvo_map_insert_cloud:")
    assert gpu.L.cvo_map_insert_cloud(None, cloud.handle, None, None) == _capi.CVO_E_INVALID
    host = u.map_open_host(u.MapConfig(**cfg.kwargs()))
    o = bc.f32(0, 0, 0)
    assert gpu.L.cvo_map_insert_cloud(host.handle, cloud.handle, None, ing._fp(o)) == _capi.CVO_E_INVALID
    assert m.size() == (0, 0) and host.size() == (0, 0)
    host.close()
    m.close()
    cloud.free()


# ---- 5. the side rule ----
def _counted(n, seed=51):
    """a frame of exactly n + 1 training points: no beam samples, every hit kept"""
    cfg, frames = bc.scattered(seed, n, C=3, spread=20.0, free_resolution=1e4)
    xyz, feat, label, _ = frames[0]
    return cfg, CvoPointCloud.from_arrays(xyz, feat, wide(label))


def test_switch_on_takes_the_host_side():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    g.set_option("BKI_HOST", 1)
    cfg, pc = _counted(300)
    cloud = g.upload(pc)
    sa = insert_both(g, cfg, cloud, T=pose(), on_device=0, what="BKI_HOST=1")
    assert sa["training"] == 301
    cloud.free()
    g.close()


@pytest.mark.parametrize("n, on_device", [(HOST_BELOW - 2, 0), (HOST_BELOW - 1, 1)])
def test_first_insert_decides_the_side_by_its_training_points(n, on_device):
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    g.set_option("BKI_HOST", -1)  # (by the first insert's training points, whatever the environment says)
    cfg, pc = _counted(n)
    cloud = g.upload(pc)
    sa = insert_both(g, cfg, cloud, T=pose(), on_device=on_device, what=f"{n + 1} training points")
    assert sa["training"] == n + 1
    # a second insert, of the other size class, keeps the side
    m, stat = open_map(g, cfg), np_bki.Map(cfg)
    _, other_pc = _counted(HOST_BELOW + 500 if on_device == 0 else 40, seed=52)
    other = g.upload(other_pc)
    for c, T in ((cloud, pose()), (other, pose(0.2))):
        m.insert_cloud(c, pose=T)
        xyz, feat, label = host_rows(c, 3)
        stat.insert(move(T, xyz), feat, label, T[:, 3])
        s = m.debug_stats(readback=True)
        assert s["on_device"] == on_device
        assert bc.first_difference(s, stat.table()) is None
    m.close()
    for c in (cloud, other):
        c.free()
    g.close()


# ---- 6. the read-out ----
def _outcome(fn):
    try:
        r = fn()
    except u.CvoError as e:
        return ("refused", str(e))
    if hasattr(r, "transform"):
        return ("solved", r.ret, r.iterations, None if r.transform is None else r.transform.view(np.uint32).tolist())
    return ("value", r)


def same_resident_clouds(gpu, m, what, min_rows=0):
    """resident_cloud() against cloud(resident=True)[3]: rows, present bits, spatial order, a score and a solve."""
    xyz, feat, label, old = m.cloud(resident=True)
    new = m.resident_cloud()
    assert new.n == old.n == len(xyz) >= min_rows, what
    dn, do = new.download(), old.download()
    assert dn.present == do.present, what
    for name in ("positions_", "features_", "labels_"):
        a, b = getattr(dn, name), getattr(do, name)
        assert a.shape == b.shape and np.array_equal(bc.bits(a), bc.bits(b)), f"{what}: {name}"
    if new.n == 0:
        return new, old
    assert np.array_equal(bc.bits(dn.positions_), bc.bits(xyz)) and np.array_equal(bc.bits(dn.features_), bc.bits(feat))
    assert new.debug_order_route() == old.debug_order_route(), what
    assert np.array_equal(new.debug_order(), old.debug_order()), what
    # the fixed frame: every second voxel centre (all of them when there are fewer than two), shifted a little
    step = 2 if new.n > 1 else 1
    frame = gpu.upload(CvoPointCloud.from_arrays(xyz[::step] + F32(0.03), feat[::step], wide(label[::step]) if label.shape[1] else None))
    init = np.eye(4, dtype=F32)
    ip = [_outcome(lambda: gpu.inner_product_gpu(frame, c, init, 0.3)) for c in (new, old)]
    assert ip[0] == ip[1], (what, ip)
    runs = [_outcome(lambda: gpu.align(frame, c, init, max_iterations=20)) for c in (new, old)]
    assert runs[0] == runs[1], what
    frame.free()
    return new, old


def _filled(gpu, case):
    cfg, frames = case
    m = open_map(gpu, cfg)
    for xyz, feat, label, origin in frames:
        m.insert((xyz, feat, label), origin=origin)
    return m


@pytest.mark.parametrize("n", [1, 64, 65, 3000])
def test_read_out_equals_the_uploaded_cloud(gpu, n):
    m = _filled(gpu, bc.occupied_cloud(300 + n, n))
    assert m.debug_stats()["on_device"] == 1
    new, old = same_resident_clouds(gpu, m, f"read-out of {n}", min_rows=n - n // 10 - 1)
    assert new.download().present == 3
    for c in (new, old):
        c.free()
    m.close()


@pytest.mark.parametrize("C", [0, 3, 19])
def test_read_out_of_three_inserts(gpu, C):
    m = _filled(gpu, bc.three_inserts(C=C))
    new, old = same_resident_clouds(gpu, m, f"three_inserts C {C}", min_rows=50 if C else 5)  # (C = 0: the case has 9 occupied voxels)
    d = new.download()
    assert d.present == (3 if C else 1)
    if 0 < C < 19:
        assert not d.labels_[:, C:].any() and d.labels_[:, :C].any()  # (zeros behind the map's classes)
    for c in (new, old):
        c.free()
    m.close()


@pytest.mark.parametrize("order", [None, "wide"])
def test_read_out_above_16384_voxels(gpu, order):
    m = _filled(gpu, bc.occupied_cloud(77, 17000))
    gpu.set_option("ORDER", order)
    try:
        new, old = same_resident_clouds(gpu, m, f"17000 voxels, ORDER={order}", min_rows=16385)
        assert new.debug_order_route() == (2 if order else 0)
    finally:
        gpu.set_option("ORDER", None)
    for c in (new, old):
        c.free()
    m.close()


def test_read_out_of_an_empty_map(gpu):
    m = open_map(gpu, np_bki.Config(resolution=0.5, num_classes=3))
    c = m.resident_cloud()
    assert c.n == 0 and c.download().present == 0
    c.free()
    m.insert((np.zeros((0, 3), F32), None, None), origin=(0.0, 0.0, 0.0))  # (one FREE voxel: still no occupied one)
    assert m.debug_stats()["on_device"] == 1
    new, old = same_resident_clouds(gpu, m, "no occupied voxel")
    assert new.n == 0
    m.close()


def test_read_out_of_a_host_side_map():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    g.set_option("BKI_HOST", 1)
    m = _filled(g, bc.three_inserts(C=3))
    assert m.debug_stats()["on_device"] == 0
    new, old = same_resident_clouds(g, m, "BKI_HOST=1", min_rows=50)
    for c in (new, old):
        c.free()
    m.close()
    g.close()


# ---- 7. the loop: frame in, align against the map, insert under the solved pose, read the map out ----
def test_the_loop_without_a_host_copy(gpu):
    cfg, frames = bc.three_inserts()
    dev, host = open_map(gpu, cfg), open_map(gpu, cfg)
    init = np.eye(4, dtype=F32)
    for f, (xyz, feat, label, _) in enumerate(frames):
        poses = []
        for route in ("device", "host"):
            frame = gpu.upload(CvoPointCloud.from_arrays(xyz, feat, label))
            target = dev.resident_cloud() if route == "device" else host.cloud(resident=True)[3]
            if target.n == 0:  # (the first frame opens the map where it stands)
                T = np.array([[1, 0, 0, 0.1], [0, 1, 0, 0.2], [0, 0, 1, 0.3]], F32)
            else:
                run = gpu.align(frame, target, init, max_iterations=20)
                assert run.iterations > 0
                T = np.ascontiguousarray(run.transform[:3, :4])
            poses.append(T)
            if route == "device":
                dev.insert_cloud(frame, pose=T)
            else:
                host.insert((xyz, feat, label), pose=T)
            frame.free()
            target.free()
        assert np.array_equal(poses[0].view(np.uint32), poses[1].view(np.uint32)), f"frame {f}"
    sd, sh = dev.debug_stats(readback=True), host.debug_stats(readback=True)
    assert sd["on_device"] == 1 and sd["voxels"] > 300
    same_tables(sd, sh, "the loop")
    dev.close()
    host.close()
