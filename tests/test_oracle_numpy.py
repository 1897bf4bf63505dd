"""The oracle's kernel matrix / flow / step coefficients against the independent float64 numpy
re-derivation in np_reference.py (SURVEY.md 8(c) "independent cross-check")."""
import numpy as np
import pytest

import cases
import feature_mixes as fm
import np_reference as npr
from unified_cvo_amd import CvoParams, CvoPointCloud, synth


def _oracle_iter(oracle, P, src, tgt, R, T, ell, K):
    op = oracle.params_from(P)
    ox, oy = oracle.Cloud.from_pointcloud(src), oracle.Cloud.from_pointcloud(tgt)
    return oracle.iteration(op, ox, oy, R, T, ell, K, want_ell=True), ox, oy


def _dense_from_ell(o, n, m):
    A = np.zeros((n, m))
    for i in range(n):
        for s in range(int(o["nonzeros"][i])):
            A[i, o["ind"][i, s]] = o["mat"][i, s]
    return A


def _check(oracle, P, src, tgt, R, T, ell, K, **feat):
    o, ox, oy = _oracle_iter(oracle, P, src, tgt, R, T, ell, K)
    r = npr.iteration(P, src.positions(), tgt.positions(), R, T, ell, K, **feat)
    tr = o["trace"]
    n, m = src.num_points(), tgt.num_points()
    A = _dense_from_ell(o, n, m)
    # same sparsity pattern except for pairs within float rounding of a cut-off
    mism = (A > 0) != r["keep"]
    assert mism.sum() <= max(2, int(1e-3 * r["keep"].sum())), mism.sum()
    both = (A > 0) & r["keep"]
    assert np.allclose(A[both], r["A"][both], rtol=2e-5)
    if mism.sum() == 0:
        assert tr.nnz == r["nnz"] and tr.max_nnz == r["max_nnz"]
        assert np.allclose(list(tr.omega), r["omega"], atol=2e-5)
        assert np.allclose(list(tr.v), r["v"], atol=2e-5)
        for name in "BCDE":
            assert getattr(tr, name) == pytest.approx(r[name], rel=5e-3, abs=1e-3 * abs(r["E"]) * 1e-6), name
        want_step = npr.step_from_coeffs(tr.B, tr.C, tr.D, tr.E, P.min_step, P.max_step)
        assert tr.step == pytest.approx(want_step, rel=1e-5)
    return o, r


def test_geometric_iteration(oracle):
    P, src, tgt, init = cases.config2(n=300)
    _check(oracle, P, src, tgt, init[:3, :3], init[:3, 3], P.ell_init, P.nearest_neighbors_max)


def test_geometric_iteration_nonidentity_pose(oracle):
    P, src, tgt, _ = cases.config2(n=250)
    Tm = synth.gt_motion()
    _check(oracle, P, src, tgt, Tm[:3, :3].astype(np.float32), Tm[:3, 3].astype(np.float32), 0.4, 64)


def test_ordered_truncation(oracle):
    """Rows keep the FIRST K qualifying targets in ascending j (CvoGPU.cu:526,576-589)."""
    P, src, tgt, init = cases.config2(n=200)
    P.ell_init = 2.0  # wide kernel: every row has far more than K neighbours
    o, r = _check(oracle, P, src, tgt, init[:3, :3], init[:3, 3], 2.0, 7)
    assert (o["nonzeros"] == 7).all()
    assert np.all(np.diff(o["ind"][:, :7], axis=1) > 0)


def test_colour_iteration(oracle):
    P, src, tgt, init = cases.config3(n=300)
    _check(oracle, P, src, tgt, init[:3, :3], init[:3, 3], P.ell_init, P.nearest_neighbors_max,
           fx=src.features(), fy=tgt.features())


def test_semantic_iteration(oracle):
    P, src, tgt, init = cases.config4(n=300)
    P.ell_init = 0.5  # the shipped 0.1 gives a handful of pairs at n=300; widen for a meaningful check
    _check(oracle, P, src, tgt, init[:3, :3], init[:3, 3], 0.5, P.nearest_neighbors_max,
           fx=src.features(), fy=tgt.features(), lx=src.labels(), ly=tgt.labels())


def test_geometric_type_gate(oracle):
    P, src, tgt, init = cases.config2(n=200)
    P.is_using_geometric_type = 1
    rs = np.random.default_rng(0)
    gx = np.where(rs.random((200, 1)) < 0.5, [[1.0, 0.0]], [[0.0, 1.0]]).astype(np.float32)
    gy = np.where(rs.random((200, 1)) < 0.5, [[1.0, 0.0]], [[0.0, 1.0]]).astype(np.float32)
    src = CvoPointCloud.from_arrays(src.positions(), None, None, gx)
    tgt = CvoPointCloud.from_arrays(tgt.positions(), None, None, gy)
    o, r = _check(oracle, P, src, tgt, init[:3, :3], init[:3, 3], 0.5, 512, gx=gx, gy=gy)
    # pairs of different type never associate
    A = _dense_from_ell(o, 200, 200)
    different = (gx[:, None, 0] != gy[None, :, 0])
    assert not (A[different] > 0).any()


def _mix_case(oracle, mix, labels, moved, ell, K):
    """One setting of the four switches through _check as it stands, and _check's allowance for pairs within float
    rounding of a cut-off must come out unused: oracle and numpy keep exactly the same pairs."""
    d, init = fm.arrays(300, labels)
    P = fm.params(mix, moved=moved)
    src, tgt = fm.clouds(d)
    o, r = _check(oracle, P, src, tgt, init[:3, :3], init[:3, 3], ell, K, fx=d["fx"], fy=d["fy"], lx=d["lx"], ly=d["ly"],
                  gx=d["gx"], gy=d["gy"])
    A = _dense_from_ell(o, 300, 300)
    assert ((A > 0) != r["keep"]).sum() == 0
    assert o["trace"].nnz == r["nnz"] and o["trace"].max_nnz == r["max_nnz"]
    return d, init, P, r


@pytest.mark.parametrize("ell,K", fm.SHIPPED_STATES)
@pytest.mark.parametrize("mix", fm.MIXES, ids=fm.MIX_IDS)
def test_switch_matrix_shipped_cutoffs(oracle, mix, ell, K):
    """All 16 settings of (geometry, intensity, semantics, geometric_type) with the shipped cut-offs, soft class rows and
    mixed geometric types ([0.3, 0.9] and [0.8, -0.5] among them)."""
    _mix_case(oracle, mix, "soft", False, ell, K)


@pytest.mark.parametrize("ell,K", fm.MOVED_STATES)
@pytest.mark.parametrize("labels", ["soft", "hot", "hot_soft"])
@pytest.mark.parametrize("mix", fm.MIXES, ids=fm.MIX_IDS)
def test_switch_matrix_moved_cutoffs_every_gate_rejects(oracle, mix, labels, ell, K):
    """The same 16 settings with sigma, sp_thres, c_ell and s_ell moved (feature_mixes.MOVED): every switched-on gate
    rejects between a tenth and nine tenths of the pairs that reach it - the product gate too wherever geometry meets
    another factor; with a single factor the factor's own cut-off is a > sp_thres and the product gate rejects nothing."""
    d, init, P, r = _mix_case(oracle, mix, labels, True, ell, K)
    R, T = init[:3, :3].astype(np.float64), init[:3, 3].astype(np.float64)
    y = (d["y"].astype(np.float64) - T) @ R
    shares = npr.gate_shares(P, d["x"], y, d["fx"], d["fy"], d["lx"], d["ly"], d["gx"], d["gy"], ell)
    assert set(shares) == {n for n, on in zip(("geometry", "colour", "semantics", "geotype"), mix) if on} | {"product"}
    for name, (reached, rejected) in shares.items():
        if name != "product" or (mix[0] and sum(mix) > 1):
            assert 0.1 * reached <= rejected <= 0.9 * reached, (name, reached, rejected)
        elif sum(mix) <= 1:
            assert rejected == 0, (name, reached, rejected)
    if K >= 300:  # no first-K truncation: the pairs that survive all five gates are the reference's nonzeros
        assert shares["product"][0] - shares["product"][1] == r["nnz"]


def test_range_ell_only_in_step_size(oracle):
    """K2 always applies the range factor; K5 only when is_using_range_ell (CvoGPU.cu:506-507 vs 1035-1037)."""
    P, src, tgt, init = cases.config2(n=200)
    o0, _, _ = _oracle_iter(oracle, P, src, tgt, init[:3, :3], init[:3, 3], 0.3, 512)
    P.is_using_range_ell = 1
    o1, _, _ = _oracle_iter(oracle, P, src, tgt, init[:3, :3], init[:3, 3], 0.3, 512)
    assert np.array_equal(o0["mat"], o1["mat"]) and np.array_equal(o0["ind"], o1["ind"])
    assert o0["trace"].B != o1["trace"].B
    r = npr.iteration(P, src.positions(), tgt.positions(), init[:3, :3], init[:3, 3], 0.3, 512)
    assert o1["trace"].B == pytest.approx(r["B"], rel=5e-3)


def test_literal_and_blocked_rows_agree(oracle):
    """The vectorisable blocked scan is only a re-ordering of `continue`s: identical ELL output."""
    P, src, tgt, init = cases.config2(n=700, m=530)
    op = oracle.params_from(P)
    ox = oracle.Cloud.from_pointcloud(src)
    _, _, yt = oracle.transform_cloud(init[:3, :3], init[:3, 3], tgt.positions())
    oy = oracle.Cloud(yt)
    for K in (3, 512):
        a = oracle.se_kernel(op, ox, oy, K, 0.35, literal=False)
        b = oracle.se_kernel(op, ox, oy, K, 0.35, literal=True)
        for u, v in zip(a, b):
            assert np.array_equal(u, v)


def test_empty_cloud_returns_zero_and_leaves_transform(oracle):
    P = CvoParams()
    op = oracle.params_from(P)
    x = oracle.Cloud(np.zeros((0, 3), np.float32))
    y = oracle.Cloud(np.ones((5, 3), np.float32))
    r = oracle.align(op, x, y, np.eye(4))
    assert r["ret"] == 0 and r["iterations"] == 0 and not r["transform"].any()


def test_all_zero_geometric_type_gives_minus_one(oracle):
    """0/0 = NaN geo_sim => every comparison false => empty A => ret -1 (CvoGPU.cu:203-215,545,576,1454-1458)."""
    P, src, tgt, init = cases.config2(n=100)
    P.is_using_geometric_type = 1
    src = CvoPointCloud.from_arrays(src.positions())
    tgt = CvoPointCloud.from_arrays(tgt.positions())
    op = oracle.params_from(P)
    r = oracle.align(op, oracle.Cloud.from_pointcloud(src), oracle.Cloud.from_pointcloud(tgt), init)
    assert r["ret"] == -1 and r["iterations"] == 0
    assert np.allclose(r["transform"], np.eye(4))


def test_alignment_recovers_ground_truth(oracle):
    P, src, tgt, init = cases.config2(n=800)
    op = oracle.params_from(P)
    r = oracle.align(op, oracle.Cloud.from_pointcloud(src), oracle.Cloud.from_pointcloud(tgt), init)
    assert r["iterations"] == P.MAX_ITER  # clamped at min_step, never reaches eps_2
    assert np.max(np.abs(r["transform"] - np.linalg.inv(synth.gt_motion()))) < 3e-3


def test_transform_pose_vec_matches_float64(oracle):
    """transform_point_pose_vec (multi-frame frames): float32 result within a few ulp of the float64 product."""
    rs = np.random.default_rng(5)
    xyz = rs.uniform(-30, 30, (2000, 3)).astype(np.float32)
    ang = 0.3
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    pose = np.hstack([R, np.array([[0.5], [-1.25], [2.0]])])
    got = oracle.transform_pose_vec(pose, xyz)
    pose32 = pose.astype(np.float32).astype(np.float64)
    want = xyz.astype(np.float64) @ pose32[:, :3].T + pose32[:, 3]
    assert np.max(np.abs(got - want)) < 2e-5          # |coords| <= ~45: a handful of float32 ulps
    # identity pose reproduces the input exactly (the edge kernel relies on it)
    I = np.hstack([np.eye(3), np.zeros((3, 1))])
    assert np.array_equal(oracle.transform_pose_vec(I, xyz), xyz)


def test_grid_variant_is_identical_to_the_dense_scan(oracle):
    """The "best-effort CPU" timing variant (uniform grid over the targets) must reproduce the dense scan bit for bit:
    same ELL pattern and values in one iteration, same pose after a short trajectory."""
    import cases
    for builder, kw in ((cases.config2, dict(n=1500)), (cases.config3, dict(n=900)), (cases.config4, dict(n=800))):
        P, src, tgt, init = builder(**kw)
        op = oracle.params_from(P)
        X, Y = oracle.Cloud.from_pointcloud(src), oracle.Cloud.from_pointcloud(tgt)
        try:
            oracle.set_grid(False)
            a = oracle.iteration(op, X, Y, init[:3, :3], init[:3, 3], P.ell_init, P.nearest_neighbors_max, want_ell=True)
            ta = oracle.align(op, X, Y, init, max_iterations=40)
            oracle.set_grid(True)
            b = oracle.iteration(op, X, Y, init[:3, :3], init[:3, 3], P.ell_init, P.nearest_neighbors_max, want_ell=True)
            tb = oracle.align(op, X, Y, init, max_iterations=40)
        finally:
            oracle.set_grid(False)
        assert np.array_equal(a["nonzeros"], b["nonzeros"]) and int(a["nonzeros"].sum()) > 0
        assert np.array_equal(a["ind"], b["ind"]) and np.array_equal(a["mat"], b["mat"])
        assert np.array_equal(ta["transform"], tb["transform"])
