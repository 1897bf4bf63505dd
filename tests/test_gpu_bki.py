"""The semantic voxel map on the device (BKI_HOST=0): the kernels of cvo_k_bki.h against the statement (np_bki.py), bit for bit
on ms, fs, keys and the rows of the cloud, on every case of bki_cases.py: block and wave edges of the hit count, per-voxel
hit runs on both sides of the short / long split, the longest and shortest rays in one wave, repeated inserts, table growth,
the read-out's sort, and the resident cloud.  Every call is checked, through the debug stats, to have run on the device."""
import numpy as np
import pytest

import bki_cases as bc
import cases
import np_bki
import test_bki_cpu as cpu
import unified_cvo_amd as u
from unified_cvo_amd import CvoGPU, CvoPointCloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))  # one context across the cases
    g.set_option("BKI_HOST", 0)
    yield g
    g.close()


def run_device(gpu, case, initial_voxels=0):
    """[(stats with the read-back table, cloud, size)] after every frame"""
    cfg, frames = case
    m = gpu.map_open(u.MapConfig(**cfg.kwargs()), initial_voxels=initial_voxels)
    out = []
    for xyz, feat, label, origin in frames:
        m.insert((xyz, feat, label), origin=origin)
        stats = m.debug_stats(readback=True)  # (one read-back: a mismatch below names its first voxel from it)
        assert stats["on_device"] == 1
        out.append((stats, m.cloud(), m.size()))
    m.close()
    return out


@pytest.mark.parametrize("name", sorted(bc.all_cases()))
def test_device_equals_the_statement(gpu, name):
    got = run_device(gpu, bc.all_cases()[name])
    cpu.compare(got, bc.statement_of(name), name)
    for stats, _, _ in got:
        assert stats["voxels"] * 2 <= stats["capacity"]  # never past half full


def test_long_run_takes_the_wave_kernel(gpu):
    got = run_device(gpu, bc.all_cases()["run3000"])
    assert got[0][0]["longest_run"] == 3000 > bc.SHORT_RUN


def test_table_grows_within_an_insert_and_again(gpu):
    got = run_device(gpu, bc.all_cases()["growth"], initial_voxels=16)
    first, second = got[0][0], got[1][0]
    assert first["growths"] >= 2 and second["growths"] > first["growths"]
    assert second["capacity"] > first["capacity"] > 32
    cpu.compare(got, bc.statement_of("growth"), "growth from 16 voxels")


@pytest.mark.parametrize("n", [1, 64, 65, 3000])
def test_read_out_is_sorted_by_key(gpu, n):
    case = bc.occupied_cloud(300 + n, n)
    want = bc.statement(case)
    assert abs(len(want[0][1][0]) - n) <= n // 10 + 1  # about n occupied voxels (random cells may coincide)
    keys = want[0][0][0]
    if n > 1:
        assert len(set(int(k) >> 40 for k in keys)) > 1 and len(set(int(k) & 0xFFFFF for k in keys)) > 1
    cpu.compare(run_device(gpu, case), want, f"read-out of {n}")


def test_refusals_leave_the_device_map(gpu):
    for name in sorted(cpu.BAD_INSERTS):
        cfg, frames = cpu.bad_insert_map(name)
        m, stat = gpu.map_open(u.MapConfig(**cfg.kwargs())), np_bki.Map(cfg)
        m.insert(frames[0][:3], origin=frames[0][3])
        stat.insert(*frames[0])
        text = cpu.check_refusal(m, stat, name)
        assert "cvo_map_insert" in text, text
        assert m.debug_stats()["on_device"] == 1
        m.close()


def test_posed_insert_moves_the_rows(gpu):
    cfg, frames = bc.all_cases()["hits65"]
    xyz, feat, label, _ = frames[0]
    a = 0.3
    T = np.array([[np.cos(a), -np.sin(a), 0, 0.5], [np.sin(a), np.cos(a), 0, -0.25], [0, 0, 1, 0.125]], np.float32)
    moved = np.empty_like(xyz)
    for r in range(3):  # fma(T0, x, T1 * y) + fma(T2, z, T3), as the cloud transform
        t = T[r].astype(np.float64)
        lo = (t[0] * xyz[:, 0].astype(np.float64) + (T[r, 1] * xyz[:, 1]).astype(np.float64)).astype(np.float32)
        hi = (t[2] * xyz[:, 2].astype(np.float64) + t[3]).astype(np.float32)
        moved[:, r] = lo + hi
    stat = np_bki.Map(cfg)
    stat.insert(moved, feat, label, T[:, 3])
    m = gpu.map_open(u.MapConfig(**cfg.kwargs()))
    m.insert((xyz, feat, label), pose=T)
    stats = m.debug_stats(readback=True)
    assert stats["on_device"] == 1
    diff = bc.first_difference(stats, stat.table())
    assert diff is None, diff
    m.close()


def test_resident_cloud_is_the_upload_of_the_rows(gpu):
    case = bc.three_inserts()
    cfg, frames = case
    m = gpu.map_open(u.MapConfig(**cfg.kwargs()))
    for xyz, feat, label, origin in frames:
        m.insert((xyz, feat, label), origin=origin)
    xyz, feat, label, resident = m.cloud(resident=True)
    assert m.debug_stats()["on_device"] == 1 and resident.n == len(xyz) > 50
    want = bc.statement_of("three_inserts")[-1][1]
    assert np.array_equal(bc.bits(xyz), bc.bits(want[0])) and np.array_equal(bc.bits(feat), bc.bits(want[1])) and np.array_equal(bc.bits(label), bc.bits(want[2]))
    uploaded = gpu.upload(CvoPointCloud.from_arrays(xyz, feat, label))
    # the fixed frame: every second voxel centre of the map, shifted a little, with its own attributes
    frame = gpu.upload(CvoPointCloud.from_arrays(xyz[::2] + np.float32(0.03), feat[::2], label[::2]))
    init = np.eye(4, dtype=np.float32)
    ip = [gpu.inner_product_gpu(frame, c, init, 0.3) for c in (resident, uploaded)]
    assert ip[0] == ip[1] and ip[0] > 0
    runs = [gpu.align(frame, c, init, max_iterations=20) for c in (resident, uploaded)]
    assert runs[0].iterations == runs[1].iterations
    assert np.array_equal(runs[0].transform.view(np.uint32), runs[1].transform.view(np.uint32))
    m.close()
