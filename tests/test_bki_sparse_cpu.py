"""The sparse kernel of the semantic voxel map without a GPU: the statement's weight (np_bki_sparse.py) against the float64
evaluation of upstream's expression and against hand-worked micro cases, and the CPU twin (cvo_map_set_kernel on a map of
cvo_map_open_host) against the statement, bit for bit, on every case of bki_sparse_cases.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bki_cases as bc
import bki_sparse_cases as sc
import cases
import np_bki
import np_bki_sparse as sp
import test_bki_cpu as cpu
import unified_cvo_amd as u
from unified_cvo_amd import _capi

F32 = np.float32


# ---- the weight ----
def accuracy_sample():
    d = [np.linspace(0, 1.5, 3000001).astype(F32)]
    for c in (0.25, 0.5, 0.75, 1.0):
        lo = hi = F32(c)
        for _ in range(64):
            lo, hi = np.nextafter(lo, F32(-1)), np.nextafter(hi, F32(3))
            d.append(np.array([lo, hi], F32))
    return np.concatenate(d)


def test_weight_is_as_accurate_as_numpys_float32():
    d = accuracy_sample()
    D, PI = d.astype(np.float64), np.float64(sp.PI)
    ref = np.maximum((2 + np.cos(D * 2 * PI)) * (1 - D) / 3 + np.sin(D * 2 * PI) / (2 * PI), 0)  # upstream's expression, its clamp
    a = d * F32(2) * sp.PI
    plain = (F32(2) + np.cos(a)) * (F32(1) - d) / F32(3) + np.sin(a) / (F32(2) * sp.PI)
    assert plain.dtype == F32
    numpy_error = float(np.abs(np.maximum(plain, F32(0)).astype(np.float64) - ref).max())
    mine = sp.weight_of_distance(d)
    assert mine.dtype == F32
    own_error = float(np.abs(mine.astype(np.float64) - ref).max())
    print(f"largest |k - float64|: the statement's routine {own_error:.3e}, numpy's float32 {numpy_error:.3e}")
    assert own_error <= 2 * numpy_error


@pytest.mark.parametrize("sf2", [1.0, 0.7, 3.0, 1e-3])
def test_weight_at_zero_is_sf2(sf2):
    assert sp.weight_of_distance(F32(0), F32(sf2)) == F32(sf2)
    assert sp.sparse_k(bc.f32(1, 1, 1), bc.f32([1, 1, 1]), sf2, 0.3)[0] == F32(sf2)


def test_weight_is_zero_from_one_and_a_half_and_never_negative():
    d = accuracy_sample()
    k = sp.weight_of_distance(d)
    assert (k >= 0).all() and (k[d >= F32(1.5)] == 0).all()
    assert sp.weight_of_distance(F32(4)) == 0 and sp.weight_of_distance(F32(1e30)) == 0
    assert (k[d >= 1] <= 1e-7).all()  # what rounding leaves of the expression's zero at d = 1


def test_sincos_quadrants():
    a = np.linspace(0, 3 * np.pi, 20001).astype(F32)[:-1]
    s, c = sp.sincos(a)
    assert np.abs(s - np.sin(a.astype(np.float64))).max() < 1.5e-7 and np.abs(c - np.cos(a.astype(np.float64))).max() < 1.5e-7
    assert sp.sincos(F32(0)) == (F32(0), F32(1))


def test_slots_are_get_extended_blocks():
    key = cpu.key_of(2, -3, 4)
    want = [(2, -3, 4), (3, -3, 4), (1, -3, 4), (2, -2, 4), (2, -4, 4), (2, -3, 5), (2, -3, 3)]
    assert [sp.slot_key(key, j) for j in range(7)] == [cpu.key_of(*w) for w in want]
    assert sp.slot_key(0, 2) is None and sp.slot_key(0xFFFFF, 5) is None and sp.slot_key(0xFFFFF, 6) == 0xFFFFE


def test_constants_mirror_the_headers():
    math = open(os.path.join(cases.ROOT, "unified_cvo_amd", "csrc", "cvo_bki_math.h")).read()
    assert re.search(r"BKI_SPARSE_MAX_RECORDS = 1ll << (\d+);", math).group(1) == "24" and sp.MAX_RECORDS == 1 << 24
    assert int(re.search(r"BKI_SPARSE_SLOTS = (\d+);", math).group(1)) == sp.SLOTS
    assert F32(float(re.search(r"BKI_SPARSE_PI = ([0-9.]+)f;", math).group(1))) == sp.PI
    assert sp.MAX_RECORDS > 567876 * 8  # every point of the LiDAR-like frame on a corner


# ---- the statement on hand-worked cases ----
def voxel(table, kx, ky, kz):
    keys, ms, fs = table
    at = list(keys).index(cpu.key_of(kx, ky, kz))
    return ms[at], fs[at]


NEIGHBOURS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def test_one_hit_at_a_voxel_centre():
    (table, cloud, last), = sc.statement_of("one_hit")
    sf2 = F32(0.7)
    k_half = sp.weight_of_distance(F32(0.5), sf2)  # resolution / ell
    assert 0 < k_half < sf2
    ms, fs = voxel(table, 2, 2, 2)
    assert list(ms) == [0, sf2] and np.array_equal(fs, np.full(5, sf2, F32))
    for d in NEIGHBOURS:
        ms, fs = voxel(table, 2 + d[0], 2 + d[1], 2 + d[2])
        assert list(ms) == [0, k_half] and np.array_equal(fs, np.full(5, k_half, F32))
        assert list(voxel(table, *d)[0]) == [k_half, 0]  # the origin votes class 0
    assert list(voxel(table, 0, 0, 0)[0]) == [sf2, 0]
    assert len(table[0]) == 14 and last == dict(training=2, members=2, longest_run=1)


@pytest.mark.parametrize("name,blocks", [("face", 2), ("edge", 4), ("corner", 8)])
def test_a_hit_on_a_shared_face_votes_through_every_membership(name, blocks):
    (table, _, last), = sc.statement_of(name)
    assert last["members"] == blocks + 1
    # the hit at (1.25, ...) is 0.25 from the centres of its blocks on every shared axis: each of its blocks hears it through
    # its self slot and through the slots of its other blocks, all at the same distance
    axes = {"face": 1, "edge": 2, "corner": 3}[name]
    d = F32(np.sqrt(F32(axes) * F32(0.25) * F32(0.25)))
    k = sp.weight_of_distance(d)
    ms, _ = voxel(table, 2, 2, 2)
    want = F32(0)
    for _ in range(1 + axes):  # self, then one neighbour slot per shared axis
        want = F32(want + k)
    assert ms[1] == want and ms[1] > k


def test_ell_variations():
    (table, cloud, _), = sc.statement_of("ell_is_resolution")
    assert voxel(table, 3, 2, 2)[0][1] == sp.weight_of_distance(F32(1)) <= 1e-7
    (table, cloud, _), = sc.statement_of("ell_quarter")
    assert len(table[0]) == 14
    for d in NEIGHBOURS:  # exactly zero, stored all the same; with prior 0 FREE and absent from the cloud
        ms, fs = voxel(table, 2 + d[0], 2 + d[1], 2 + d[2])
        assert not ms.any() and not fs.any()
    assert len(cloud[0]) == 1 and list(cloud[0][0]) == [1, 1, 1]
    (table, cloud, _), = sc.statement_of("ell_twenty")
    assert voxel(table, 3, 2, 2)[0][1] == sp.weight_of_distance(F32(0.05)) > 0.98


def test_distances_on_both_sides_of_one_and_one_and_a_half():
    cfg, frames = sc.all_cases()["d_edges"]
    xyz = frames[0][1][0]
    d = sp.distance(sp.centre_of(cpu.key_of(0, 0, 0), cfg.resolution), xyz, F32(cfg.ell))
    assert list(d) == sc.D_EDGES
    assert [len(np_bki.blocks_of(p[0], p[1], p[2], cfg.resolution)) for p in xyz] == [1, 2, 1, 1, 1, 1]
    (table, _, _), = sc.statement_of("d_edges")
    k = sp.weight_of_distance(np.array(sc.D_EDGES, F32), F32(cfg.sf2))
    assert (k[3:] == 0).all()
    # the voxel at 0: the first two hits through its self slot, the hits of its +x neighbour (the second again) through that
    want = F32(F32(k[0] + k[1]) + F32(F32(F32(F32(k[1] + k[2]) + k[3]) + k[4]) + k[5]))
    assert voxel(table, 0, 0, 0)[0][1] == want


def test_the_long_segment_is_order_sensitive():
    cfg, frames = sc.all_cases()["run3000_alone"]
    (table, _, last), = sc.statement_of("run3000_alone")
    assert last["longest_run"] == 3000
    xyz, feat, label, origin = frames[0][1]
    centre = bc.f32(2.0, 1.0, -1.0)
    inside = np.flatnonzero(np.all(np.abs(xyz - centre) < 0.25, axis=1))
    k = sp.sparse_k(centre, xyz[inside], cfg.sf2, cfg.ell)
    fwd = [sp.float_sum(k * feat[inside, f]) for f in range(5)]
    rev = [sp.float_sum((k * feat[inside, f])[::-1]) for f in range(5)]
    assert fwd != rev and list(voxel(table, 4, 2, -2)[1]) == fwd


def test_neighbour_only_voxels_are_stored_unlike_the_counting_insert():
    cfg, frames = sc.all_cases()["one_hit"]
    a, b = sp.Map(cfg, sp.SPARSE), np_bki.Map(cfg)
    a.insert(*frames[0][1])
    b.insert(*frames[0][1])
    assert len(a.voxels) == 14 and len(b.voxels) == 2 and set(b.voxels) <= set(a.voxels)


# ---- the CPU twin against the statement ----
def run_twin(case):
    m = u.map_open_host(u.MapConfig(**sc.map_kwargs(case[0])))
    out = sc.run_map(m, case)
    m.close()
    return out


@pytest.mark.parametrize("name", sorted(sc.all_cases()))
def test_twin_equals_the_statement(name):
    got = run_twin(sc.all_cases()[name])
    assert all(s["on_device"] == 0 for s, _, _ in got)
    cpu.compare(got, sc.statement_of(name), name)


def test_default_kernel_is_the_counting_one():
    cfg, frames = bc.all_cases()["hits65"]
    for touch in (False, True):
        m = u.map_open_host(u.MapConfig(**sc.map_kwargs(cfg)))
        if touch:
            m.set_kernel("sparse")
            m.set_kernel("csm")
        m.insert(frames[0][:3], origin=frames[0][3])
        assert bc.first_difference(m.debug_stats(readback=True), bc.statement_of("hits65")[0][0]) is None
        m.close()


def check_set_kernel_refusals(m, stat):
    """unknown kernels, and - on maps opened for it - SPARSE with a bad sf2 or ell: the table and the kernel stay"""
    before = m.debug_stats(readback=True)
    for bad in (2, -1, 7):
        with pytest.raises(u.CvoError) as err:
            m.set_kernel(bad)
        assert str(_capi.CVO_E_INVALID) in str(err.value)
        with pytest.raises(np_bki.Refused):
            stat.set_kernel(bad)
    after = m.debug_stats(readback=True)
    for k in ("keys", "ms", "fs"):
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    return str(err.value)


BAD_SCALES = [dict(sf2=0.0), dict(sf2=-1.0), dict(sf2=float("nan")), dict(ell=0.0), dict(ell=float("inf")), dict(ell=float("nan"))]


def test_set_kernel_refuses_and_leaves_the_map():
    cfg, frames = sc.all_cases()["classes2_feat"]
    m, stat = u.map_open_host(u.MapConfig(**sc.map_kwargs(cfg))), sp.Map(cfg, sp.SPARSE)
    m.set_kernel("sparse")
    m.insert(frames[0][1][:3], origin=frames[0][1][3])
    stat.insert(*frames[0][1])
    check_set_kernel_refusals(m, stat)
    m.insert(frames[0][1][:3], origin=frames[0][1][3])  # still sparse
    stat.insert(*frames[0][1])
    assert bc.first_difference(m.debug_stats(readback=True), stat.table()) is None
    m.close()
    assert _capi.lib().cvo_map_set_kernel(None, 1) == _capi.CVO_E_INVALID
    for kw in BAD_SCALES:
        bad = config_with(kw)
        m = u.map_open_host(u.MapConfig(**sc.map_kwargs(bad)))
        with pytest.raises(u.CvoError):
            m.set_kernel("sparse")
        with pytest.raises(np_bki.Refused):
            sp.Map(bad, sp.SPARSE)
        m.set_kernel("csm")  # the counting kernel never looks at them
        m.insert(frames[0][1][:3], origin=frames[0][1][3])  # ... and is the one that runs
        plain = np_bki.Map(bad)
        plain.insert(*frames[0][1])
        assert bc.first_difference(m.debug_stats(readback=True), plain.table()) is None
        m.close()


def config_with(kw):
    return sc.config(**dict(dict(sf2=1.0, ell=1.0, num_classes=2), **kw))


def record_cap_frame():
    """72 rays of about 60 000 samples along lines that lie ON an edge of the grid (y and z on faces): 4.3 million training
    points, below 2^24, with four memberships each, above 2^24"""
    x = np.linspace(59.0, 60.0, 72).astype(F32)
    xyz = np.stack([x, np.full(72, 0.25, F32), np.full(72, 0.25, F32)], 1)
    return sc.config(free_resolution=0.001), xyz, bc.f32(0.1, 0.25, 0.25)


def check_record_cap(m):
    """m holds one good sparse frame: the insert beyond the record cap is refused as unsupported and leaves the table"""
    cfg, xyz, origin = record_cap_frame()
    before = m.debug_stats(readback=True)
    with pytest.raises(u.CvoError) as err:
        m.insert((xyz, None, None), origin=origin)
    assert str(_capi.CVO_E_UNSUPPORTED) in str(err.value)
    assert m.gpu is None or "memberships" in str(err.value)  # (a host map has no context to hold a text)
    after = m.debug_stats(readback=True)
    for k in ("keys", "ms", "fs"):
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    m.set_kernel("csm")  # the counting insert has no such cap
    m.insert((xyz, None, None), origin=origin)
    assert m.debug_stats()["members"] > sp.MAX_RECORDS > m.debug_stats()["training"]


def test_record_cap_refuses_and_leaves_the_map():
    cfg, xyz, origin = record_cap_frame()
    m = u.map_open_host(u.MapConfig(**sc.map_kwargs(cfg)))
    m.set_kernel("sparse")
    m.insert((bc.f32([1, 1, 1]), None, None), origin=bc.f32(0, 0, 0))
    check_record_cap(m)
    m.close()
