"""The score cases of overlap_cases.py (no GPU): the conditions that keep tests/test_gpu_overlap_edges.py from hiding a
failure, asserted on EVERY case.

  margin         no pair or non-pair is closer to a gate (geometric cut-off, colour / semantic cut-off, a > sp_thres) than
                 float32 rounding can move it: 1e-3 relative near the origin (row_classes.py's margin); far from the origin
                 the larger of that and the bound computed from the terms of R^T y - R^T T (FAR_ULPS below);
  visibility     one dropped or doubled pair moves the sum by at least 100 tolerances: min pair value / statement > 100 tol;
  no truncation  the largest row count stays below K (but the void case, a row of K + 1, and the K = 64 case, a row of K);
  limit          the case lies on the structural limit it was built for.
"""
import numpy as np
import pytest

import overlap_cases as oc

MARGIN = 1e-3
# Far from the origin a coordinate of y' - x is the rounded sum of three products and a translation, minus a coordinate of x:
# three products and Tinv's own three (half an ulp each), two + two + one additions and the subtraction - 12 roundings of at
# most half an ulp of the LARGEST term, 6 ulps; FAR_ULPS = 8 leaves room for the inputs' own rounding in the statement's
# favour.  Each coordinate of the difference moves by at most delta = FAR_ULPS 2^-23 max_term, the distance d by sqrt(3) delta,
# d^2 relatively by 2 sqrt(3) delta / d - set against the pair's distance to its gate.
FAR_ULPS = 8
# The bounds against float64 the GPU test uses (test_gpu_row_classes.TOL_F64, test_gpu_feature_gates.TOL_F64_FEATURED =
# 2 x test_row_class_clouds.ORACLE_F64_DIST; test_gpu_overlap_edges.py asserts these are the same numbers)
TOL = {"geo": 2e-6, "featured": 2 * 6.1e-7}
# ... and, far from the origin, the oracle's own distance from float64, measured here (test_oracle_distance_far_from_origin):
# 9.953e-5, on touch-far-xy-0.98.  Coordinates of 800 carry an ulp of 6.1e-5, the pair's distance is 1.9: d^2 is off by
# some 1e-4 relative before the exponential (exponent -2.7) sees it.
ORACLE_F64_DIST_FAR = 9.953e-5
TOL["far"] = 2 * ORACLE_F64_DIST_FAR

CASES = oc.all_cases()
IDS = [c.name for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_margin_visibility_truncation(case):
    st = case.statement()
    need = MARGIN
    if case.tol == "far":
        d = st["nearest"][0] * oc.radius(case.P) * (np.linalg.norm(oc.OFFSET) / 500.0 + 1.0)
        delta = FAR_ULPS * 2.0 ** -23 * st["max_term"]
        need = max(MARGIN, 2.0 * np.sqrt(3.0) * delta / d)
        assert st["max_term"] > 500.0 and need > MARGIN, (st["max_term"], need)  # (the case IS far from the origin)
    assert st["margin"] >= need, (case.name, st["margin"], need)
    if len(st["pairs"][0]):
        assert st["min_value"] / st["total"] > 100.0 * TOL[case.tol], (case.name, st["min_value"], st["total"], len(st["pairs"][0]))
    else:
        assert st["total"] == 0.0
    K = int(case.P.nearest_neighbors_max)
    if case.void:
        assert st["widest"] == K and int(st["counts"].max()) == K and case.limit  # (cut to K by the statement's first-K)
    elif case.name.endswith("-K64"):
        assert st["widest"] == K  # (the issue's own K = 64 case: a row of exactly K pairs, which nothing truncates)
    else:
        assert st["widest"] < K, (case.name, st["widest"])


def _by(tag):
    return [c for c in CASES if tag in c.tags]


@pytest.mark.parametrize("case", _by("queue"), ids=lambda c: c.name)
def test_queue_cases_sit_on_the_list_capacity(case):
    """One row tile, one target tile; the geometric candidates per quarter of the wave (16 lanes = 16 rows) are the
    layout's, so their total is 1024 (one group, the list full), 1025 (four quarters) ..., and in reach means in reach of
    whole clusters: a row's candidates are 0, 1, 37 or 64."""
    st = case.statement()
    assert case.N == 64 and case.M == 64
    ci, cj = st["cand"]
    per_row = np.bincount(ci, minlength=64)
    assert [int(per_row[16 * q:16 * q + 16].sum()) for q in range(4)] == case.limit["quarters"]
    assert set(per_row.tolist()) <= {0, 1, 37, 64}
    total = int(per_row.sum())
    if case.name.startswith("queue-1024"):
        assert total == oc.OV_QCAP and all(per_row[list(oc.SPREAD_ROWS)] == 64)
    if case.name.startswith("queue-1025"):
        assert total == oc.OV_QCAP + 1 and per_row[20] == 1
    if case.name.startswith("queue-alternate"):
        assert all(per_row[0::2] == 64) and not per_row[1::2].any()
    n_pairs = len(st["pairs"][0])
    if case.P.is_using_semantics:  # classes alternate between neighbouring rows and targets: the other class is rejected
        pi, pj = st["pairs"]
        assert 0 < n_pairs < total and np.all(pi % 2 == pj % 2)
        assert n_pairs == int(((ci % 2) == (cj % 2)).sum())
    elif not case.void:
        assert n_pairs == total
    if case.void:
        assert per_row.max() == 64 > case.P.nearest_neighbors_max
    # the rows in reach hold different values
    if n_pairs:
        assert st["min_value"] < 0.8 * st["total"] / n_pairs or case.name.startswith("queue-4096")


@pytest.mark.parametrize("case", _by("partial"), ids=lambda c: c.name)
def test_partial_cases(case):
    st = case.statement()
    pi, pj = st["pairs"]
    assert len(pi) == case.limit["pairs"]
    if "only_target" in case.limit:
        assert case.M == 65 and np.all(pj == 64) and len(np.unique(pi)) == case.N
    elif "only_row" in case.limit:
        assert case.N == 65 and np.all(pi == 64) and len(np.unique(pj)) == case.M
    else:
        assert len(pi) == case.N * case.M and 64 in (case.N, case.M)


@pytest.mark.parametrize("case", _by("touch"), ids=lambda c: c.name)
def test_touching_cases(case):
    """|x* - y*| = f r_x* after the pose, to 1e-3 (float32 inputs far from the origin: 1e-4 of r), every other cross pair
    beyond 2 r; the touching tile is target tile 1 of 3, point 0 of both tiles."""
    st = case.statement()
    f = case.limit["f"]
    pi, pj = st["pairs"]
    assert len(pi) == case.limit["pairs"]
    if f < 1:
        assert (int(pi[0]), int(pj[0])) == (0, 64)
    assert abs(st["nearest"][0] - f) < 1e-3, st["nearest"]
    assert st["nearest"][1] > 2.0, st["nearest"]
    assert case.N == 64 and case.M == 192
    if "stretch" in case.limit:
        # the first cull's sphere test as cvo_k_overlap.h states it, in float64 on the float64 records: with the pose's
        # stretch the touching tile is within reach, without it the tile is culled - whatever the slack factors add
        x, y = case.src.astype(np.float64), case.tgt[64:128].astype(np.float64)
        R, t = case.T[:3, :3].astype(np.float64), case.T[:3, 3].astype(np.float64)
        xc, yc = 0.5 * (x.min(0) + x.max(0)), 0.5 * (y.min(0) + y.max(0))
        xr, yr = np.linalg.norm(x - xc, axis=1).max(), np.linalg.norm(y - yc, axis=1).max()
        r = oc.radius(case.P) * (np.linalg.norm(x, axis=1).max() / 500.0 + 1.0)
        dist = np.linalg.norm((yc - t) @ R - xc)
        fro = np.sqrt((R * R).sum())
        assert case.limit["stretch"] > 1.2 and fro >= case.limit["stretch"]
        assert dist > (xr + r + yr) * 1.05, (dist, xr, r, yr)     # culled without `* stretch` (slack: 1e-4 and 4e-6 terms)
        assert f > 1 or dist < xr + yr * case.limit["stretch"] + r  # ... and at f = 0.98 in reach with the true stretch


@pytest.mark.parametrize("case", _by("busy"), ids=lambda c: c.name)
def test_busy_queue_cases(case):
    """Every one of the 8 / 9 target tiles holds 4096 candidates for the one row tile, and 64 pairs: one per row."""
    st = case.statement()
    n = case.limit["tiles"]
    assert case.N == 64 and case.M == 64 * n
    assert (oc.tile_pair_counts(st["cand"], 1, n)[0] == 4096).all() and 4096 > oc.OV_QCAP
    per = oc.tile_pair_counts(st["pairs"], 1, n)[0]
    assert (per == 64).all() and (st["counts"] == n).all() and len(st["pairs"][0]) == case.limit["pairs"]
    pi, pj = st["pairs"]
    assert (pi != pj % 64).any()  # (pairs evaluated by a lane other than the row's own)


@pytest.mark.parametrize("case", _by("reversed") + _by("angle"), ids=lambda c: c.name)
def test_reversed_and_angle_cases(case):
    st = case.statement()
    assert sorted(zip(st["pairs"][0].tolist(), st["pairs"][1].tolist())) == case.limit["pairs"] and len(case.limit["pairs"]) >= 1
    assert (max(case.N, case.M) + 63) // 64 == 1025 and min(case.N, case.M) in (1, 64)


def test_tolerances_are_the_projects():
    """TOL above are the numbers the GPU tests of the row classes and the feature gates hold (no device needed to say so)."""
    from test_gpu_feature_gates import TOL_F64_FEATURED
    from test_gpu_row_classes import TOL_F64
    assert TOL == {"geo": TOL_F64, "featured": TOL_F64_FEATURED, "far": 2 * ORACLE_F64_DIST_FAR}


@pytest.mark.parametrize("case", _by("list"), ids=lambda c: c.name)
def test_list_cases(case):
    """The pairs are the built ones: 3 .. 5 in each of the tiles that end or start a 512-tile pass, a 1024-tile round or the
    cloud; the last tile is partial; no other target is in reach of any row."""
    st = case.statement()
    pi, pj = st["pairs"]
    n_tiles = (case.M + 63) // 64
    assert case.M == 64 * n_tiles - 37 and n_tiles in oc.TILE_COUNTS
    assert sorted(zip(pi.tolist(), pj.tolist())) == case.limit["pairs"]
    per_tile = oc.tile_pair_counts((pi, pj), 1, n_tiles)[0]
    assert np.flatnonzero(per_tile).tolist() == case.limit["tiles"] == oc.special_tiles(n_tiles)
    assert all(3 <= per_tile[t] <= 5 for t in case.limit["tiles"])
    assert n_tiles - 1 in case.limit["tiles"] and 0 in case.limit["tiles"] and oc.OV_PASS - 1 in case.limit["tiles"]
    if n_tiles > oc.OV_PASS:
        assert oc.OV_PASS in case.limit["tiles"]          # the second pass of the test loop
    if n_tiles > oc.OV_LIST_CAP:
        assert oc.OV_LIST_CAP in case.limit["tiles"] and oc.OV_LIST_CAP - 1 in case.limit["tiles"]  # the second round
    # the filling: what the first cull sees, stated on the float64 geometry (sphere about the box centre)
    x = case.src.astype(np.float64)
    xc = 0.5 * (x.min(0) + x.max(0))
    xr = np.linalg.norm(x - xc, axis=1).max()
    r = oc.radius(case.P) * (np.linalg.norm(x, axis=1).max() / 500.0 + 1.0)
    y = case.tgt.astype(np.float64)
    plain = [t for t in range(n_tiles) if t not in case.limit["tiles"]]
    gap = []
    for t in plain[:: max(1, len(plain) // 40)]:
        p = y[64 * t:64 * t + 64]
        c = 0.5 * (p.min(0) + p.max(0))
        gap.append(np.linalg.norm(c - xc) - np.linalg.norm(p - c, axis=1).max() - xr)
    if "far" in case.name:
        assert min(gap) > 10 * r      # spheres apart: culled
    else:
        assert max(gap) < 0.0         # inside the row tile's sphere: listed, whatever the slack factors


def test_nothing_case():
    c = _by("nothing")[0]
    assert c.statement()["total"] == 0.0 and c.statement()["nearest"][0] > 10.0 and c.N > 128 and c.M > 128


def test_oracle_distance_far_from_origin(oracle):
    """|oracle - float64| / float64 on the far-from-origin cases with a pair: the oracle computes in the device's floats, and
    its distance from the statement is what the GPU test allows the device twice (the argument TOL_F64_FEATURED records).
    Measured: see ORACLE_F64_DIST_FAR."""
    worst, where = 0.0, None
    for case in CASES:
        if case.tol != "far" or not len(case.statement()["pairs"][0]):
            continue
        src, tgt = case.clouds()
        got = oracle.inner_product(oracle.params_from(case.P), oracle.Cloud.from_pointcloud(src), oracle.Cloud.from_pointcloud(tgt),
                                   case.T, case.ell)
        want = case.statement()["total"]
        if abs(got - want) / want > worst:
            worst, where = abs(got - want) / want, case.name
    print(f"oracle vs float64, far from the origin: {worst:.5e} on {where}")
    assert 0.0 < worst <= ORACLE_F64_DIST_FAR, worst


def test_debug_cloud_tiles_is_exported_and_refuses_nulls():
    """cvo_debug_cloud_tiles is bound, and without a context it is CVO_E_INVALID before any device work."""
    from unified_cvo_amd import _capi
    assert "cvo_debug_cloud_tiles" in _capi.EXPORTED
    assert _capi.lib().cvo_debug_cloud_tiles(None, None, None, None) == _capi.CVO_E_INVALID
