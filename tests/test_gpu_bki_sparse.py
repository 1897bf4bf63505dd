"""The sparse kernel of the semantic voxel map on the device (BKI_HOST=0): the kernels of cvo_k_bki_sparse.h against the
statement (np_bki_sparse.py), bit for bit on the whole table - keys, ms, fs through cvo_debug_map_stats - and on the cloud read
out, on every case of bki_sparse_cases.py: one hit and its neighbours, hits on shared faces, the length scale on both sides of
the block size, segment lengths on both sides of the lane / wave split and of the wave's trips, real beams with a cluster at
the origin, the class counts with and without feature rows, repeated and mixed inserts, table growth by neighbour-only voxels,
the posed and resident routes, the refusals, and the same bits on every run.  The counting kernel's path is checked unchanged."""
import numpy as np
import pytest

import bki_cases as bc
import bki_sparse_cases as sc
import cases
import np_bki_sparse as sp
import test_bki_cpu as cpu
import test_bki_sparse_cpu as scpu
import test_gpu_map_resident as res
import unified_cvo_amd as u
from unified_cvo_amd import CvoGPU, CvoPointCloud

pytestmark = pytest.mark.gpu

F32 = np.float32


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))  # one context across the cases
    g.set_option("BKI_HOST", 0)
    yield g
    g.close()


def open_map(gpu, cfg, kernel=None, initial_voxels=0):
    m = gpu.map_open(u.MapConfig(**sc.map_kwargs(cfg)), initial_voxels=initial_voxels)
    if kernel is not None:
        m.set_kernel(kernel)
    return m


def run_device(gpu, case, initial_voxels=0):
    m = open_map(gpu, case[0], initial_voxels=initial_voxels)
    out = sc.run_map(m, case)
    m.close()
    assert all(stats["on_device"] == 1 for stats, _, _ in out)
    return out


# ---- 1. the counting kernel's path is unchanged ----
@pytest.mark.parametrize("name", ["hits257", "run65", "rays"])
@pytest.mark.parametrize("touch", [False, True])
def test_counting_kernel_is_unchanged(gpu, name, touch):
    cfg, frames = bc.all_cases()[name]
    m = open_map(gpu, cfg)
    if touch:
        m.set_kernel("csm")
        m.set_kernel("sparse")
        m.set_kernel("csm")
    got = []
    for xyz, feat, label, origin in frames:
        m.insert((xyz, feat, label), origin=origin)
        got.append((m.debug_stats(readback=True), m.cloud(), m.size()))
    m.close()
    assert got[0][0]["on_device"] == 1
    cpu.compare(got, bc.statement_of(name), name)


# ---- 2 - 9. every case against the statement ----
@pytest.mark.parametrize("name", sorted(sc.all_cases()))
def test_device_equals_the_statement(gpu, name):
    got = run_device(gpu, sc.all_cases()[name])
    cpu.compare(got, sc.statement_of(name), name)
    for stats, _, _ in got:
        assert stats["voxels"] * 2 <= stats["capacity"]  # never past half full


def test_one_hit_counts_its_fourteen_voxels(gpu):
    (stats, cloud, size), = run_device(gpu, sc.all_cases()["one_hit"])
    assert size == (14, 7) and stats["voxels"] == 14  # the hit's seven are OCCUPIED, the origin's seven FREE
    at = list(stats["keys"]).index(cpu.key_of(2, 2, 2))
    assert stats["ms"][at][1] == F32(0.7)


def test_zero_weight_neighbours_are_stored_and_free(gpu):
    (stats, cloud, size), = run_device(gpu, sc.all_cases()["ell_quarter"])
    assert size == (14, 1) and len(cloud[0]) == 1


def test_long_segments_take_the_wave_kernel(gpu):
    for name in ("run3000_alone", "run3000_beside"):
        got = run_device(gpu, sc.all_cases()[name])
        assert got[0][0]["longest_run"] == 3000 > bc.SHORT_RUN


def test_table_grows_by_neighbour_only_voxels(gpu):
    case = sc.all_cases()["growth"]
    got = run_device(gpu, case, initial_voxels=16)
    first, second = got[0][0], got[1][0]
    members = sc.statement_of("growth")[0][2]["members"]
    assert first["voxels"] > 3 * members  # (more voxels than the frame has memberships: most have only a neighbour with points)
    assert first["growths"] >= 2 and second["growths"] > first["growths"]
    assert second["capacity"] > first["capacity"] > 32
    cpu.compare(got, sc.statement_of("growth"), "growth from 16 voxels")


# ---- 10. the posed and the resident routes ----
def test_posed_and_resident_inserts_equal_the_insert_of_the_moved_rows(gpu):
    cfg, frames = sc.all_cases()["classes19_feat"]
    xyz, feat, label, _ = frames[0][1]
    T = res.pose()
    moved = res.move(T, xyz)
    stat = sp.Map(cfg, sp.SPARSE)
    stat.insert(moved, feat, label, T[:, 3])
    maps = [open_map(gpu, cfg, "sparse") for _ in range(3)]
    maps[0].insert((moved, feat, label), origin=T[:, 3])
    maps[1].insert((xyz, feat, label), pose=T)
    cloud = gpu.upload(CvoPointCloud.from_arrays(xyz, feat, res.wide(label)))
    maps[2].insert_cloud(cloud, pose=T)
    for m, what in zip(maps, ("insert", "insert_posed", "insert_cloud")):
        stats = m.debug_stats(readback=True)
        assert stats["on_device"] == 1
        diff = bc.first_difference(stats, stat.table())
        assert diff is None, f"{what}: {diff}"
    # the read-out: the resident cloud built on the device against the upload of the rows
    rows = maps[2].cloud(resident=True)
    want = stat.cloud()
    for a, b in zip(rows[:3], want):
        assert a.shape == b.shape and np.array_equal(bc.bits(a), bc.bits(b))
    built = maps[2].resident_cloud()
    assert built.n == rows[3].n == len(want[0]) > 50
    a, b = built.download(), rows[3].download()
    for x, y in ((a.positions_, b.positions_), (a.features_, b.features_), (a.labels_, b.labels_)):
        assert np.array_equal(bc.bits(x), bc.bits(y))
    cloud.free()
    for m in maps:
        m.close()


# ---- 11. refusals ----
def test_set_kernel_refuses_and_leaves_the_device_map(gpu):
    cfg, frames = sc.all_cases()["classes2_feat"]
    m, stat = open_map(gpu, cfg, "sparse"), sp.Map(cfg, sp.SPARSE)
    m.insert(frames[0][1][:3], origin=frames[0][1][3])
    stat.insert(*frames[0][1])
    text = scpu.check_set_kernel_refusals(m, stat)
    assert "cvo_map_set_kernel:" in text
    m.insert(frames[0][1][:3], origin=frames[0][1][3])  # still sparse
    stat.insert(*frames[0][1])
    stats = m.debug_stats(readback=True)
    assert stats["on_device"] == 1 and bc.first_difference(stats, stat.table()) is None
    m.close()
    for kw in scpu.BAD_SCALES:
        m = open_map(gpu, scpu.config_with(kw))
        with pytest.raises(u.CvoError) as err:
            m.set_kernel("sparse")
        assert "cvo_map_set_kernel:" in str(err.value)
        m.close()


def test_record_cap_refuses_and_leaves_the_device_map(gpu):
    cfg, xyz, origin = scpu.record_cap_frame()
    m = open_map(gpu, cfg, "sparse")
    m.insert((bc.f32([1, 1, 1]), None, None), origin=bc.f32(0, 0, 0))
    assert m.debug_stats()["on_device"] == 1
    scpu.check_record_cap(m)
    m.close()


def test_insert_refusals_leave_the_sparse_map(gpu):
    for name in ("nan_hit", "hit_out_of_range", "ray_too_long"):
        cfg, frames = cpu.bad_insert_map(name)
        cfg = sc.config(resolution=float(cfg.resolution), free_resolution=float(cfg.free_resolution), num_classes=cfg.num_classes)
        m, stat = open_map(gpu, cfg, "sparse"), sp.Map(cfg, sp.SPARSE)
        m.insert(frames[0][:3], origin=frames[0][3])
        stat.insert(*frames[0])
        cpu.check_refusal(m, stat, name)
        m.close()


# ---- 12. the same bits on every run ----
def test_the_same_insert_gives_the_same_bits(gpu):
    case = sc.all_cases()["rays"]
    a, b = run_device(gpu, case), run_device(gpu, case, initial_voxels=50000)  # (another table size: other slots, other arrival)
    for k in ("keys", "ms", "fs"):
        assert np.array_equal(a[0][0][k].view(np.uint8), b[0][0][k].view(np.uint8)), k
    for x, y in zip(a[0][1], b[0][1]):
        assert np.array_equal(bc.bits(x), bc.bits(y))


# ---- the side rule: unchanged for counting maps, its own measured crossover for maps that are sparse at their first insert ----
SPARSE_HOST_BELOW = 547  # BKI_SPARSE_HOST_BELOW (cvo_bki.hip)


def test_side_rule_of_a_map_that_starts_sparse():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))  # (BKI_HOST unset)
    for kernel, n, on_device in (("sparse", SPARSE_HOST_BELOW - 2, 0), ("sparse", SPARSE_HOST_BELOW - 1, 1), ("csm", SPARSE_HOST_BELOW - 1, 0),
                            ("csm", res.HOST_BELOW - 2, 0)):
        _, frames = bc.scattered(77, n, C=2)
        cfg = sc.config(sf2=1.0, ell=1.0, num_classes=2)  # (free_resolution 100, no beam samples: n + 1 training points)
        xyz, feat, label, origin = frames[0]
        cloud = g.upload(CvoPointCloud.from_arrays(xyz, feat, res.wide(label)))
        tables = {}
        for route in ("insert", "insert_cloud"):
            m = open_map(g, cfg, kernel)
            if route == "insert":
                m.insert((xyz, feat, label), origin=origin)
            else:
                m.insert_cloud(cloud, origin=origin)
            stats = m.debug_stats(readback=True)
            assert stats["training"] == n + 1 and stats["on_device"] == on_device, (kernel, n, route)
            tables[route] = stats
            m.insert((xyz, feat, label), origin=origin)  # the side is kept
            assert m.debug_stats()["on_device"] == on_device
            m.close()
        if not on_device:  # the twin stores voxels as they come: the resident rows, copied down, leave the host rows' table bit for bit
            for k in ("keys", "ms", "fs"):
                assert len(tables["insert"][k]) > 0
                assert np.array_equal(tables["insert"][k].view(np.uint8), tables["insert_cloud"][k].view(np.uint8)), (kernel, n, k)
        cloud.free()
    g.close()
