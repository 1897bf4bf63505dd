"""The read side of the semantic voxel map without a GPU: the CPU twin (cvo_map_query_host / _raycast_host / _render_host on a
map of cvo_map_open_host) against the statement (np_bki_query.py), bit for bit, on every case of bki_query_cases.py; the
statement's own walk against a property test in exact rationals that shares no code with it; hand-checked answers; the two
consistency rules (the read-out's rows, render against raycast); the refusals."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import bki_cases as bc
import bki_query_cases as qc
import cases
import np_bki
import np_bki_query as nq
import unified_cvo_amd as u
from unified_cvo_amd import _capi

F32 = np.float32


def host_map(name):
    c = qc.case(name)
    return qc.fill(u.map_open_host(u.MapConfig(**qc.config_kwargs(c.cfg))), c)


# ---- 1. the twin equals the statement ----
@pytest.mark.parametrize("name", qc.names())
def test_twin_equals_the_statement(name):
    m = host_map(name)
    diff = qc.differences(m, name)
    m.close()
    assert not diff, "\n".join(diff)


def test_constants_mirror_the_headers():
    math = open(os.path.join(cases.ROOT, "unified_cvo_amd", "csrc", "cvo_bki_math.h")).read()
    assert re.search(r"BKI_RAY_MAX_STEPS = 1 << (\d+);", math).group(1) == "20" and nq.MAX_STEPS == 1 << 20
    assert re.search(r"BKI_RENDER_MAX_PIXELS = 1ll << (\d+);", math).group(1) == "24" and nq.MAX_PIXELS == 1 << 24
    assert "BKI_BIT_FREE = 1, BKI_BIT_OCCUPIED = 2, BKI_BIT_UNKNOWN = 4, BKI_BIT_ABSENT = 8" in math
    assert (_capi.CVO_MAP_STOP_FREE, _capi.CVO_MAP_STOP_OCCUPIED, _capi.CVO_MAP_STOP_UNKNOWN, _capi.CVO_MAP_STOP_ABSENT) == (1, 2, 4, 8)
    assert "0x7fc00000u" in math and nq.NAN.view(np.uint32) == 0x7FC00000


# ---- 2. hand-checked answers of the statement ----
def test_fma32_rounds_once():
    rng = np.random.default_rng(1)
    a, x, c = (rng.uniform(-4, 4, 20000) * np.exp(rng.uniform(-20, 20, 20000))).astype(F32), rng.uniform(-4, 4, 20000).astype(F32), rng.uniform(-4, 4, 20000).astype(F32)
    want = np.array([F32(Fraction(float(p)) * Fraction(float(q)) + Fraction(float(r))) for p, q, r in zip(a, x, c)], F32)
    # (F32(Fraction) goes through a correctly rounded double: compare only where that double is no float32 tie)
    exact = [Fraction(float(p)) * Fraction(float(q)) + Fraction(float(r)) for p, q, r in zip(a, x, c)]
    tie = np.array([Fraction(float(e)) != e and (np.float64(float(e)).view(np.int64) & ((1 << 29) - 1)) == (1 << 28) for e in exact])
    got = nq.fma32(a, x, c)
    assert np.array_equal(got[~tie], want[~tie]) and tie.sum() < 5


def test_a_face_point_is_stored_in_two_voxels_and_found_in_one():
    c, want = qc.case("faces"), qc.expected("faces")
    size = c.cfg.resolution
    for i in range(6):
        p = c.points[i]
        stored = np_bki.blocks_of(p[0], p[1], p[2], size)
        assert len(stored) == 2 and all(k in want["map"].voxels for k in stored)
        assert want["query"]["found"][i] == nq.FOUND
        hit = [k for k in stored if np.array_equal(nq.centre_of(k, size), want["query"]["centre"][i])]
        assert len(hit) == 1 and hit[0] == nq.key_of(p, size)  # the +0.5 truncation picks one of the insert's two
        # k0 rounds half away from zero towards +infinity: the upper voxel on both signs of the coordinate
        a = int(np.flatnonzero(np.abs(p) % F32(0.5) == F32(0.25))[0])
        assert want["query"]["centre"][i][a] == p[a] + F32(0.25)


def test_key_range_and_the_outside_answer():
    c, q = qc.case("key_range"), qc.expected("key_range")["query"]
    assert list(q["found"]) == [1, 1, 0] + [2] * 11 + [0]
    outside = q["found"] == nq.OUTSIDE
    assert (q["state"][outside] == np_bki.UNKNOWN).all() and (q["semantics"][outside] == -1).all()
    assert (q["centre"][outside].view(np.uint32) == 0x7FC00000).all()
    nclass, prior = 2, F32(0.25)
    assert np.array_equal(q["probs"][outside], np.full((11, nclass), prior / (prior + prior), F32))
    assert np.array_equal(q["centre"][0], c.points[0]) and np.array_equal(q["centre"][1], c.points[1])
    rays = qc.expected("key_range")["rays"][0]
    assert list(rays["status"]) == [0, 0, 3, 3, 3, 3, 3] and (rays["key"][2:] == nq.NO_KEY).all() and (rays["steps"][2:] == 0).all()


def test_the_default_node():
    m = nq.node(qc.expected("empty")["map"], nq.key_of(bc.f32(0, 0, 0), F32(0.5)))
    assert m[0] is False and m[1] == np_bki.UNKNOWN and m[2] == -1
    assert np.isnan(m[3]).all() and np.isnan(m[4]).all() and np.isnan(m[5]).all()  # prior 0: 0 / 0, as upstream's node would give
    m = nq.node(qc.expected("empty_prior")["map"], nq.key_of(bc.f32(0, 0, 0), F32(0.5)))
    assert np.array_equal(m[3], bc.f32(0.5, 0.5)) and np.array_equal(m[4], bc.f32(0.125, 0.125)) and np.array_equal(m[5], np.zeros(5, F32))


def test_getters_against_float64():
    want = qc.expected("classes_19")
    q, m = want["query"], want["map"]
    found = np.flatnonzero(q["found"] == nq.FOUND)
    assert len(found) > 100
    for i in found[:60]:
        ms, fs = m.voxels[nq.key_of(qc.case("classes_19").points[i], m.cfg.resolution)]
        ms64, s = ms.astype(np.float64), ms.astype(np.float64).sum()
        p = ms64 / s
        assert np.allclose(q["probs"][i], p, rtol=1e-5, atol=0) and np.allclose(q["vars"][i], (p - p * p) / (s + 1), rtol=1e-4, atol=1e-9)
        assert q["semantics"][i] == int(np.argmax(q["probs"][i])) and np.allclose(q["feat"][i], fs / ms64[1:].sum(), rtol=1e-5)
        assert q["state"][i] == np_bki.state_of(m.cfg, ms)


def test_every_state_is_met():
    states = set()
    for name in ("one_hit_occupied", "one_hit_unknown", "wall"):
        q = qc.expected(name)["query"]
        states |= set(q["state"][q["found"] == nq.FOUND].tolist())
        assert (q["found"] == nq.ABSENT).any()
    assert states == {np_bki.FREE, np_bki.OCCUPIED, np_bki.UNKNOWN}
    sparse = qc.expected("sparse")
    q = sparse["query"]
    assert (q["state"][q["found"] == nq.FOUND] == np_bki.FREE).sum() > 50  # (neighbour-only voxels are stored and FREE)


def test_rays_stop_where_the_cases_say():
    w = qc.expected("wall")["rays"]
    occ, occ_unknown, none = w[0], w[1], w[3]
    assert list(occ["status"][:3]) == [0, 0, 0] and list(occ["steps"][:3]) == [1, 1, 1] and (occ["t"][:3] == 0).all()  # zero length, one voxel
    assert list(none["steps"][3:9]) == [7] * 6 and (none["status"] == nq.RAY_END).all()  # axis-parallel: 1 + 6 voxels
    assert list(none["steps"][9:12]) == [19] * 3 and list(none["steps"][12:15]) == [13] * 3  # corners: 1 + 3 * 6; edges: 1 + 2 * 6
    assert list(occ["status"][18:21]) == [0, 1, 1] and occ["steps"][19] == occ["steps"][20] == 9  # before, in, behind an OCCUPIED voxel
    assert occ["state"][19] == np_bki.OCCUPIED and occ["key"][19] == occ["key"][20] == qc.key_of(4, 2, 2)
    assert occ["status"][3] == 0 and occ_unknown["status"][3] == 1 and occ_unknown["state"][3] == np_bki.UNKNOWN  # bit 4
    assert occ_unknown["key"][3] == qc.key_of(4, 0, 0) and occ_unknown["t"][3] == F32(1.75 / 3.0)
    exact, short, long_, stop, stop_short, one = w[7:13]
    assert (exact["status"][0], exact["steps"][0]) == (0, 10) and (short["status"][0], short["steps"][0]) == (2, 0)
    assert long_["steps"][0] == 10 and stop_short["status"][0] == 2 and (one["status"][0], one["steps"][0]) == (0, 1)


# ---- 3. the walk against exact rationals ----
def segments():
    out = []
    for seed, size, spread in ((1, 0.5, 6.0), (2, 0.3, 4.0), (3, 0.05, 1.0), (4, 0.25, 30.0)):
        rng = np.random.default_rng(seed)
        o, e = rng.uniform(-spread, spread, (150, 3)).astype(F32), rng.uniform(-spread, spread, (150, 3)).astype(F32)
        e[:40] = o[:40] + rng.uniform(-4, 4, (40, 3)).astype(F32) * F32(size)
        o[100:], e[100:] = np.round(o[100:] / F32(size / 2)) * F32(size / 2), np.round(e[100:] / F32(size / 2)) * F32(size / 2)  # faces, edges, corners
        e[140:, 2] = o[140:, 2]
        out += [(F32(size), o[i], e[i]) for i in range(150)]
    return out


def box_meets_segment(lo, hi, o, e):
    """exact: the closed box [lo, hi] meets the segment o -> e (slabs over Fractions)"""
    t0, t1 = Fraction(0), Fraction(1)
    for a in range(3):
        d = e[a] - o[a]
        if d == 0:
            if not lo[a] <= o[a] <= hi[a]:
                return False
            continue
        ta, tb = (lo[a] - o[a]) / d, (hi[a] - o[a]) / d
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    return t0 <= t1


def test_walk_properties_in_exact_rationals():
    """The tolerance: a voxel's box is inflated by resolution * 2^-30 on every side.  What it has to cover: the k0 rule itself
    rounds p / resolution + 524288.5 in double, which moves a voxel's faces by up to resolution * 524288.5 * 2^-52 < resolution
    * 2^-33 against the exact grid; a crossing's b is one rounded product (|b| 2^-53) and its t three more roundings, so two
    crossings are taken in the wrong order only when they lie within about 4 * 2^-53 (|b| + |e - o|) of each other in position,
    below 2^-38 resolution for every segment here (|coordinate| <= 140 resolutions).  No segment is left out: the share the
    check cannot decide is 0, within the 1 % the cap allows."""
    left_out, segs = 0, segments()
    for size, o, e in segs:
        keys = nq.visited(size, o, e)
        k0 = [np_bki.k0_of(o[a], size) for a in range(3)]
        k1 = [np_bki.k0_of(e[a], size) for a in range(3)]
        idx = [((k >> 40) & 0xFFFFF, (k >> 20) & 0xFFFFF, k & 0xFFFFF) for k in keys]
        assert list(idx[0]) == k0 and list(idx[-1]) == k1
        assert len(keys) == 1 + sum(abs(k1[a] - k0[a]) for a in range(3))
        for p, q in zip(idx, idx[1:]):
            assert sorted(abs(p[a] - q[a]) for a in range(3)) == [0, 0, 1]
        res = Fraction(float(size))
        tol = res / (1 << 30)
        fo, fe = [Fraction(float(v)) for v in o], [Fraction(float(v)) for v in e]
        for k in idx:
            lo = [(k[a] - np_bki.KOFF - Fraction(1, 2)) * res - tol for a in range(3)]
            hi = [(k[a] - np_bki.KOFF + Fraction(1, 2)) * res + tol for a in range(3)]
            assert box_meets_segment(lo, hi, fo, fe), (float(size), o, e, k)
    assert left_out / len(segs) <= 0.01


def test_ties_go_to_the_lowest_axis():
    keys = nq.visited(F32(0.5), bc.f32(0, 0, 0), bc.f32(1, 1, 1))
    idx = [((k >> 40) - np_bki.KOFF, ((k >> 20) & 0xFFFFF) - np_bki.KOFF, (k & 0xFFFFF) - np_bki.KOFF) for k in keys]
    assert idx == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2)]


# ---- 4. consistency ----
@pytest.mark.parametrize("name", ["classes_19", "sparse", "room"])
def test_occupied_rows_of_the_read_out_are_found(name):
    m = host_map(name)
    xyz, feat, label = m.cloud()
    assert len(xyz) > 20
    q = m.query(xyz)
    C_ = qc.case(name).cfg.num_classes
    assert (q.found == nq.FOUND).all() and (q.state == np_bki.OCCUPIED).all()
    assert np.array_equal(qc.raw(q.centre), qc.raw(xyz)) and np.array_equal(qc.raw(q.feat), qc.raw(feat))
    assert np.array_equal(qc.raw(q.probs[:, 1:C_ + 1]), qc.raw(label))  # get_occupied_probs
    sx, sf, sl = qc.expected(name)["map"].cloud()
    assert np.array_equal(qc.raw(sx), qc.raw(xyz)) and np.array_equal(qc.raw(sl), qc.raw(label))
    m.close()


def test_render_depth_equals_raycast_of_the_same_rays():
    m, c = host_map("room"), qc.case("room")
    for v in c.views:
        kw = dict(v)
        mask = kw.pop("stop_mask")
        view = m.render(stop=mask, **kw)
        origin, end = nq.pixel_rays(**{k: kw[k] for k in ("pose", "fx", "fy", "cx", "cy", "rows", "cols", "z_far")})
        rays = m.raycast(origin.reshape(-1, 3), end.reshape(-1, 3), stop=mask)
        stop = rays.status == nq.RAY_STOPPED
        # (float)(t * (double)z_far) needs the double t: the statement keeps it next to the float cast the library returns
        want = nq.raycast(qc.expected("room")["map"], origin.reshape(-1, 3), end.reshape(-1, 3), mask, nq.MAX_STEPS)
        assert np.array_equal(qc.raw(rays.t), qc.raw(want["t"])) and np.array_equal(rays.status, want["status"])
        depth = np.where(stop, (want["td"] * float(F32(kw["z_far"]))).astype(F32), F32(0)).reshape(view.depth.shape)
        assert np.array_equal(qc.raw(view.depth), qc.raw(depth))
        assert np.array_equal(view.semantics.reshape(-1), np.where(stop, rays.semantics, -1))
        assert ((view.depth > 0) == stop.reshape(view.depth.shape)).all()
    m.close()


def test_every_plane_null_in_turn():
    m, v = host_map("room"), dict(qc.case("room").views[2])
    mask, want = v.pop("stop_mask"), qc.expected("room")["views"][2]
    for leave in nq_fields():
        planes = tuple(p for p in nq_fields() if p != leave)
        view = m.render(stop=mask, planes=planes, **v)
        assert getattr(view, leave) is None and qc.first_difference(view, want, qc.VIEW_FIELDS) is None
    m.close()


def nq_fields():
    return qc.VIEW_FIELDS


def test_queries_leave_the_table_alone_and_inserts_go_on():
    name = "classes_1"
    m, c = host_map(name), qc.case(name)
    before = m.debug_stats(readback=True)
    for _ in range(3):
        assert not qc.differences(m, name)
    after = m.debug_stats(readback=True)
    for k in ("keys", "ms", "fs"):
        assert np.array_equal(qc.raw(before[k]), qc.raw(after[k])), k
    xyz, feat, label, origin = c.frames[0]
    m.insert((xyz, feat, label), origin=origin)
    stat = c.statement_map()
    stat.insert(xyz, feat, label, origin)
    assert bc.first_difference(m.debug_stats(readback=True), stat.table()) is None
    m.close()


# ---- 5. refusals ----
def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_refusals_of_the_host_entry_points():
    L = _capi.lib()
    m = host_map("one_hit_occupied")
    xyz, out = bc.f32(0, 0, 0, 1, 1, 1).reshape(2, 3), _capi.cvo_map_query_out_t()
    inv = _capi.CVO_E_INVALID
    assert L.cvo_map_query_host(None, 2, _fp(xyz), C.byref(out)) == inv
    assert L.cvo_map_query_host(m.handle, -1, _fp(xyz), C.byref(out)) == inv
    assert L.cvo_map_query_host(m.handle, 2, None, C.byref(out)) == inv
    assert L.cvo_map_query_host(m.handle, 0, None, C.byref(out)) == 0 and L.cvo_map_query_host(m.handle, 0, None, None) == 0
    assert L.cvo_map_query_host(m.handle, 2, _fp(xyz), None) == 0  # (no output wanted)
    assert L.cvo_map_query(m.handle, 2, _fp(xyz), C.byref(out)) == inv  # a host map through the context's entry point
    rays = _capi.cvo_map_ray_out_t()
    assert L.cvo_map_raycast_host(None, 2, _fp(xyz), _fp(xyz), 2, 100, C.byref(rays)) == inv
    assert L.cvo_map_raycast_host(m.handle, -1, _fp(xyz), _fp(xyz), 2, 100, C.byref(rays)) == inv
    assert L.cvo_map_raycast_host(m.handle, 2, None, _fp(xyz), 2, 100, C.byref(rays)) == inv
    assert L.cvo_map_raycast_host(m.handle, 2, _fp(xyz), None, 2, 100, C.byref(rays)) == inv
    for steps in (0, -1, (1 << 20) + 1):
        assert L.cvo_map_raycast_host(m.handle, 2, _fp(xyz), _fp(xyz), 2, steps, C.byref(rays)) == inv
    assert L.cvo_map_raycast_host(m.handle, 2, _fp(xyz), _fp(xyz), 16, 100, C.byref(rays)) == inv
    for steps in (1, 1 << 20):
        assert L.cvo_map_raycast_host(m.handle, 2, _fp(xyz), _fp(xyz), 0, steps, C.byref(rays)) == 0
    assert L.cvo_map_raycast_host(m.handle, 0, None, None, 0, 1, None) == 0
    assert L.cvo_map_raycast(m.handle, 2, _fp(xyz), _fp(xyz), 2, 100, C.byref(rays)) == inv
    view, T = _capi.cvo_map_render_out_t(), qc.look_along_x()

    def render(pose=T, fx=8.0, fy=8.0, cx=3.5, cy=3.5, rows=8, cols=8, z_far=3.0, mask=2, handle=m.handle, call=L.cvo_map_render_host):
        return call(handle, None if pose is None else _fp(np.ascontiguousarray(pose, F32)), fx, fy, cx, cy, rows, cols, z_far, mask, C.byref(view))

    assert render() == 0
    assert render(handle=None) == inv and render(pose=None) == inv and render(call=L.cvo_map_render) == inv
    assert render(rows=0) == inv and render(cols=-3) == inv and render(mask=16) == inv
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert render(fx=bad) == inv and render(fy=bad) == inv and render(z_far=bad) == inv
    assert render(cx=np.nan) == inv and render(cy=np.inf) == inv
    for q in (0, 7, 11):
        P = T.copy()
        P.reshape(-1)[q] = np.nan
        assert render(pose=P) == inv
    assert render(rows=4097, cols=4096) == _capi.CVO_E_UNSUPPORTED and render(rows=1 << 20, cols=1 << 20) == _capi.CVO_E_UNSUPPORTED
    m.close()
