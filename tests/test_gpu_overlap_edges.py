"""k_overlap and k_tile_spheres (cvo_k_overlap.h) on their structural edges: the cases of overlap_cases.py, whose conditions
test_overlap_cases_cpu.py asserts without a GPU.

Every case is checked four ways (`_check`):
  a. route       debug_last_score_batch() == (1, 0, 1): the overlap kernel answered alone (the void case: the chain ran);
  b. statement   the value is the float64 statement within TOL_F64 (geometry), TOL_F64_FEATURED (colour, one-hot) or TOL_FAR;
  c. chain       it is the forced list chain's (IP_CHAIN=1) to rel = 2e-7; bit for bit in the void case;
  d. order       the same clouds under the default order give the same float32 bits as under NO_SORT=1.
Edges: the first cull at its tight side (touching tiles, f = 0.98 / 1.02 of the cut-off, under rotations, a reflection, two
matrices that are no rotation and far from the origin; thin tiles for the box), partial tiles of either cloud, the
parked-pair list at 1024 / 1025 / 4096 pairs with unequal and alternating quarters and rows that differ in class from their
neighbours - on one wave (one tile pair) and on all eight at once (8 / 9 tiles of 4096 candidates) -, the tile list at 512 / 513 / 1024 / 1025 / 1026 tiles (second pass, second round), three jobs on one grid, the
table kernel's search, and the tile records themselves (DeviceCloud.debug_tiles).

TOL_FAR: the oracle, which computes in the device's floats, is 9.953e-5 from float64 on the far-from-origin cases
(test_overlap_cases_cpu.ORACLE_F64_DIST_FAR, measured there on the CPU); the device gets twice that, by the
argument TOL_F64_FEATURED records.  Against the chain those cases stay at 2e-7.

Wall time on an MI355X host, first run (pytest --durations=0; 69 tests in 4.8 s, the numpy statements included):
  test_batch_of_five_unequal_jobs                     0.45 s (five cases through _check, one of 65 563 rows, then the batch)
  test_tile_list                                      [1024 .. 1026] 0.21 - 0.25 s each, [512, 513] 0.11 - 0.13 s each
  test_exact_function_angle_three_jobs_on_one_grid    0.09 s
  test_touching_balls                                 0.05 s per pose (20 cases each; 24 for the two non-rotations)
  test_parked_pair_list_on_every_wave                 0.02 s, 0.01 s
  test_touching_thin_tiles                            0.02 s per pose (12 cases each)
  every other test                                    under 5 ms; 0.35 s once for the module's two contexts
"""
import ctypes

import numpy as np
import pytest

import overlap_cases as oc
from test_gpu_feature_gates import TOL_F64_FEATURED
from test_gpu_row_classes import TOL_F64
from test_overlap_cases_cpu import ORACLE_F64_DIST_FAR, TOL as CPU_TOL
from unified_cvo_amd import CvoGPU, CvoPointCloud, _capi

pytestmark = pytest.mark.gpu

TOL_FAR = 2 * ORACLE_F64_DIST_FAR
TOL = {"geo": TOL_F64, "featured": TOL_F64_FEATURED, "far": TOL_FAR}
assert TOL == CPU_TOL  # (test_overlap_cases_cpu.test_tolerances_are_the_projects says so without a device)
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def ctxs():
    """(a context under NO_SORT=1, one under the default order); a case sets its own parameters on both."""
    ns, df = CvoGPU(params=oc.params()), CvoGPU(params=oc.params())
    ns.set_option("NO_SORT", "1")
    yield ns, df
    ns.close()
    df.close()


def _bits(v):
    return np.float32(v).view(np.uint32)


def _check(ctxs, case, kept=None):
    """The four checks on one case.  kept: a dict the caller wants (name -> float32 value under NO_SORT) filled."""
    ns, df = ctxs
    ns.params = df.params = case.P
    src, tgt = case.clouds()
    a, b = ns.upload(src), ns.upload(tgt)
    a2, b2 = df.upload(src), df.upload(tgt)
    try:
        assert np.array_equal(a.debug_order(), np.arange(case.N)) and np.array_equal(b.debug_order(), np.arange(case.M))
        got = np.float32(ns.inner_product_gpu(a, b, case.T, case.ell))
        route = ns.debug_last_score_batch()
        ns.set_option("IP_CHAIN", "1")
        try:
            chain = np.float32(ns.inner_product_gpu(a, b, case.T, case.ell))
        finally:
            ns.set_option("IP_CHAIN", None)
        dflt = np.float32(df.inner_product_gpu(a2, b2, case.T, case.ell))
    finally:
        for c in (a, b, a2, b2):
            c.free()
    want = case.statement()["total"]
    msg = f"{case.name}: got {float(got)!r} statement {want!r} chain {float(chain)!r} default order {float(dflt)!r} route {route}"
    if case.void:
        assert route[0] == 1 and route[1] == 1, msg
        assert _bits(got) == _bits(chain), msg
    else:
        assert route == (1, 0, 1), msg
        assert float(got) == pytest.approx(float(chain), rel=2e-7, abs=0), msg
    assert float(got) == pytest.approx(want, rel=TOL[case.tol], abs=0), msg
    assert _bits(got) == _bits(dflt), msg
    if kept is not None:
        kept[case.name] = got
    return got


# ---- the tile records -----------------------------------------------------------------------------------------------------------
def _record_clouds():
    rs = np.random.default_rng(21)
    out = {f"n{n}": rs.normal(0, 2.0, (n, 3)) for n in (1, 63, 64, 65, 129)}
    out["copies"] = np.tile(rs.normal(0, 2.0, (1, 3)), (64, 1))
    for a in range(3):
        line = np.tile(rs.normal(0, 2.0, (1, 3)), (64, 1))
        line[:, a] += rs.uniform(-5, 5, 64)
        out[f"line{'xyz'[a]}"] = line
    outlier = rs.normal(0, 0.5, (64, 3))
    outlier[17] += (1e4, 0, 0)
    out["outlier"] = outlier
    out["offset"] = rs.normal(0, 2.0, (200, 3)) + oc.OFFSET
    zeros = rs.normal(0, 1.0, (130, 3))
    zeros[::3, 0] = 0.0
    zeros[5] = 0.0
    zeros[64:128] = 0.0          # a tile of nothing but zeros: centre, radius and extents are the additive slack alone
    zeros[128:, 1] = 0.0
    out["zeros"] = zeros
    lone = rs.normal(0, 1.0, (65, 3))
    lone[64] = (900.0, -40.0, 7.0)  # a last tile of one point, far from tile 0: padding with anything else would show
    out["lone_last"] = lone
    return {k: v.astype(np.float32) for k, v in out.items()}


RECORD_CLOUDS = _record_clouds()


@pytest.mark.parametrize("name", list(RECORD_CLOUDS))
def test_tile_records_bound_their_points_tightly(ctxs, name):
    """Every tile's sphere and box hold its points (float64 on the stored floats), and both are tight: the radius is at most
    the largest distance to the stored centre times (1 + 1e-4) plus the kernel's additive slack, the half extents likewise.
    The slack is the kernel's own expression 1e-6f (|cx| + |cy| + |cz|) + 1e-30f in ITS floats, one ulp up (evaluated in
    float64 it would sit half an ulp above or below the float the kernel adds, and a tile of one point has nothing else in
    its radius; the ulp covers a compiler that fuses the multiply and the add); every comparison is made in float64."""
    ns, _ = ctxs
    pts = RECORD_CLOUDS[name]
    d = ns.upload(CvoPointCloud.from_xyz(pts))
    try:
        rec = d.debug_tiles()
        assert np.array_equal(d.debug_order(), np.arange(len(pts)))
    finally:
        d.free()
    nt = (len(pts) + 63) // 64
    assert rec.shape == (nt, 8) and rec.dtype == np.float32
    f = np.float32
    for t in range(nt):
        p = pts[64 * t:64 * t + 64].astype(np.float64)
        c32 = rec[t, :3]
        slack = float(np.nextafter(f(f(f(1e-6) * f(f(abs(c32[0]) + abs(c32[1])) + abs(c32[2]))) + f(1e-30)), f(np.inf)))
        c, r, h = rec[t, :3].astype(np.float64), float(rec[t, 3]), rec[t, 4:7].astype(np.float64)
        dist = np.linalg.norm(p - c, axis=1)
        ext = np.abs(p - c).max(0)
        assert (dist <= r).all(), (name, t, dist.max(), r)
        assert (np.abs(p - c) <= h).all(), (name, t, ext, h)
        assert r <= dist.max() * (1 + 1e-4) + slack, (name, t, r, dist.max(), slack)
        assert (h <= ext * (1 + 1e-4) + slack).all(), (name, t, h, ext, slack)
        assert rec[t, 7] == 0.0


def test_reading_the_records_changes_no_score(ctxs):
    """A score before debug_tiles() equals the score after it, a cloud whose records were READ first scores the same, and
    both routes hold the same records."""
    ns, _ = ctxs
    case = oc.queue_case("quarters")
    ns.params = case.P
    src, tgt = case.clouds()
    a, b = ns.upload(src), ns.upload(tgt)
    first = ns.inner_product_gpu(a, b, case.T, case.ell)
    ra, rb = a.debug_tiles(), b.debug_tiles()
    assert ns.inner_product_gpu(a, b, case.T, case.ell) == first
    a2, b2 = ns.upload(src), ns.upload(tgt)
    ra2, rb2 = a2.debug_tiles(), b2.debug_tiles()
    assert np.array_equal(ra, ra2) and np.array_equal(rb, rb2)
    assert ns.inner_product_gpu(a2, b2, case.T, case.ell) == first
    assert ns.debug_last_score_batch() == (1, 0, 1)
    for c in (a, b, a2, b2):
        c.free()


def test_debug_tiles_refusals(ctxs):
    """Null pointers, an empty cloud and a cloud of another context are CVO_E_INVALID, as the neighbouring entries refuse."""
    ns, df = ctxs
    L = ns.L
    buf = np.zeros(8, np.float32)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    n = ctypes.c_int(-7)
    d = ns.upload(CvoPointCloud.from_xyz(np.ones((3, 3), np.float32)))
    empty = ns.upload(CvoPointCloud.from_xyz(np.zeros((0, 3), np.float32)))
    for args in ((None, d.handle, fp, ctypes.byref(n)), (ns.ctx, None, fp, ctypes.byref(n)), (ns.ctx, d.handle, None, ctypes.byref(n)),
                 (ns.ctx, d.handle, fp, None), (ns.ctx, empty.handle, fp, ctypes.byref(n)), (df.ctx, d.handle, fp, ctypes.byref(n))):
        assert L.cvo_debug_cloud_tiles(*args) == _capi.CVO_E_INVALID, args
    assert n.value == -7 and not buf.any()
    assert L.cvo_debug_cloud_tiles(ns.ctx, d.handle, fp, ctypes.byref(n)) == 0 and n.value == 1
    d.free()
    empty.free()


# ---- the first cull at its tight edge -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", oc.BALL_POSES)
def test_touching_balls(ctxs, pose):
    """Ball against ball, touching at f = 0.98 (one pair: one kernel value) and 1.02 (exactly 0.0) in ten directions; the
    touching tile sits between two culled ones.  Under the two matrices that are no rotation also along the axis they stretch
    most, the target a ball in its OWN frame: its record says 5 r, the moved tile reaches 10 r (6.5 r) from its centre, and
    only `stretch` in the first cull's reach keeps the tile."""
    for case in oc.touching_cases(pose):
        got = _check(ctxs, case)
        assert (got > 0) == (case.limit["f"] < 1), case.name


@pytest.mark.parametrize("pose", oc.THIN_POSES)
def test_touching_thin_tiles(ctxs, pose):
    """A segment 20 r long against a ball, in both roles: the sphere test passes by far, the box decides.  `cyclic` is a
    rotation whose |R| is not symmetric (the 90 degree rotations' is): a box moved with the transposed matrix lies along
    another axis."""
    for case in oc.thin_cases(pose):
        got = _check(ctxs, case)
        assert (got > 0) == (case.limit["f"] < 1), case.name


# ---- partial tiles ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", oc.PARTIAL)
def test_partial_tiles_every_pair_a_hit(ctxs, n, m):
    _check(ctxs, oc.partial_case(n, m))


@pytest.mark.parametrize("lone", ["target", "row"])
def test_partial_tiles_lone_point(ctxs, lone):
    """M = 65 with target 64 - alone in tile 1 - the only one in reach (the positions beyond the cloud must not count), and
    N = 65 with row 64 the only row with pairs."""
    _check(ctxs, oc.partial_case(64, 65, "target") if lone == "target" else oc.partial_case(65, 64, "row"))


# ---- the parked-pair list ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feature", oc.QUEUE_FEATURES, ids=lambda f: f or "geometry")
@pytest.mark.parametrize("layout", oc.QUEUE_LAYOUTS)
def test_parked_pair_list(ctxs, layout, feature):
    """1024 candidates (the list full, one group), 1025 (four quarters), 4096, quarters of 1024 / 1 / 0 / 37, lanes
    alternating between 0 and 64; with colour features that all pass and with one-hot classes that alternate between
    neighbouring rows (an evaluating lane that took its OWN row's class or denominators would change the sum)."""
    _check(ctxs, oc.queue_case(layout, feature))


@pytest.mark.parametrize("n_tiles", oc.BUSY_TILES)
def test_parked_pair_list_on_every_wave(ctxs, n_tiles):
    """8 / 9 target tiles of 4096 candidates each against one row tile: all eight waves are on a four-quarter tile at once
    (no idle list next to a full one), with 9 wave 0 takes a second; the classes keep one pair per row and tile."""
    _check(ctxs, oc.busy_queue_case(n_tiles))


def test_void_at_K63_not_at_K64(ctxs):
    """The 1025 layout has rows of 64 pairs: K = 63 voids k_overlap and the chain answers, bit for bit; K = 64 does not."""
    _check(ctxs, oc.queue_case("1025", None, K=63))
    _check(ctxs, oc.queue_case("1025", None, K=64))


# ---- the tile list -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filling", oc.FILLINGS)
@pytest.mark.parametrize("n_tiles", oc.TILE_COUNTS)
def test_tile_list(ctxs, n_tiles, filling):
    """64 rows against 512 .. 1026 target tiles, the last one partial, pairs in the tiles at both ends of a 512-tile pass, of
    a 1024-tile round and of the cloud; nearly all tiles culled (far) or all listed and rejected by the second cull
    (shell).  N stays 64: the all-listed 1026-tile case is one block of 1026 tiles."""
    _check(ctxs, oc.list_case(n_tiles, filling))


def test_nothing_in_reach(ctxs):
    """Exactly 0.0, not void, no chain launch."""
    case = oc.nothing_case()
    assert _check(ctxs, case) == 0.0
    ns, _ = ctxs
    src, tgt = case.clouds()
    assert ns.function_angle(src, tgt, case.T, case.ell, is_approximate=True) == 0.0
    assert ns.debug_last_score_batch() == (1, 0, 1)


# ---- several jobs in one launch ----------------------------------------------------------------------------------------------------
def _angle_case():
    """The 1025-tile far cloud against ONE point, the first row of its row grid (its pair: the first target of tile 0).  The
    far targets are nodes of one lattice of spacing 4 r and the near ones 1.2 r and more from each other, so <Y, Y> is its
    diagonal: M sigma^2."""
    full = oc.list_case(1025, "far")
    P, r = full.P, oc.radius(full.P)
    near = np.array([j for _, j in full.limit["pairs"]])
    far = np.setdiff1d(np.arange(full.M), near)
    node = (full.tgt[far].astype(np.float64) - 60.0 * r) / (4.0 * r)
    assert np.abs(node - np.rint(node)).max() < 1e-3 and len(np.unique(np.rint(node).astype(np.int64), axis=0)) == len(far)
    y = full.tgt.astype(np.float64)
    d = np.linalg.norm(y[near][:, None, :] - y[None, :, :], axis=2)
    d[np.arange(len(near)), near] = np.inf
    r_max = r * (np.linalg.norm(y, axis=1).max() / 500.0 + 1.0)          # the largest cut-off radius of any target as a row
    r_near = r * (np.linalg.norm(y[near], axis=1).max() / 500.0 + 1.0)  # ... of a near one
    assert d[:, near].min() > 1.15 * r_near and d[:, far].min() > 2.0 * r_max and 4.0 * r > 2.0 * r_max
    s2 = float(np.float32(P.sigma)) ** 2
    xy, yx = (c.statement()["total"] for c in oc.angle_cases())
    assert xy > 0 and yx > 0
    return full, xy / np.sqrt(s2 * full.M * s2), yx / np.sqrt(full.M * s2 * s2)


def test_exact_function_angle_three_jobs_on_one_grid(ctxs):
    """Exact function_angle of N = 1 against 1025 target tiles and the reverse: jobs of 1, 1 and 1025 row tiles share the grid
    of k_overlap_entry.  Route (3, 0, 1); the value is <X, Y> / sqrt(<X, X> <Y, Y>) of the float64 statements, each sum
    within TOL_F64 and the two under the root at half weight: 2 TOL_F64, plus four float roundings of the host arithmetic.
    (No chain here: the chain's workspace for 65 563 x 65 563 is not what this test is about.)"""
    full, want_xy, want_yx = _angle_case()
    ns, df = ctxs
    ns.params = df.params = full.P
    x, y = CvoPointCloud.from_xyz(full.src[:1]), CvoPointCloud.from_xyz(full.tgt)
    bound = 2 * TOL_F64 + 4 * 2.0 ** -24
    for g in (ns, df):
        dx, dy = g.upload(x), g.upload(y)
        fa = g.function_angle(dx, dy, EYE, full.ell, is_approximate=False)
        assert g.debug_last_score_batch() == (3, 0, 1)
        fb = g.function_angle(dy, dx, EYE, full.ell, is_approximate=False)
        assert g.debug_last_score_batch() == (3, 0, 1)
        assert fa == pytest.approx(want_xy, rel=bound, abs=0), (fa, want_xy)
        assert fb == pytest.approx(want_yx, rel=bound, abs=0), (fb, want_yx)
        both = g.function_angle_batch([dx, dy], [dy, dx], [EYE, EYE], full.ell, is_approximate=False)
        assert _bits(both[0]) == _bits(fa) and _bits(both[1]) == _bits(fb)
        dx.free()
        dy.free()


def test_batch_of_five_unequal_jobs(ctxs):
    """Five geometry cases in one inner_product_batch - 2, 3, 1, 1 and 1025 row tiles: the table kernel's binary search over
    unequal tile counts - equal their single calls bit for bit, which _check holds to the statement and the chain."""
    ns, _ = ctxs
    jobs = [oc.partial_case(65, 64), oc.nothing_case(), oc.queue_case("1025"), oc.list_case(513, "shell"), oc.reversed_list_case()]
    single = {}
    for case in jobs:
        _check(ctxs, case, kept=single)
    assert [(c.N + 63) // 64 for c in jobs] == [2, 3, 1, 1, 1025]
    ns.params = jobs[0].P
    clouds = [c.clouds() for c in jobs]
    up = [(ns.upload(s), ns.upload(t)) for s, t in clouds]
    got = ns.inner_product_batch([u[0] for u in up], [u[1] for u in up], [c.T for c in jobs], oc.ELL)
    assert ns.debug_last_score_batch() == (5, 0, 1)
    for case, v in zip(jobs, got):
        assert _bits(v) == _bits(single[case.name]), (case.name, float(v), float(single[case.name]))
    for u in up:
        u[0].free()
        u[1].free()
