"""Multi-frame align on the CPU side: the restatement's Jacobian, Plus and convergence (tests/np_multiframe.py), and the
library's exports of cvo_multiframe_align / cvo_debug_irls_normal (no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np

import cases
import irls_cases as ic
import np_multiframe as nm
from unified_cvo_amd import _capi, synth


def _pose(deg, axis, t):
    return np.hstack([synth.rot_axis_angle(axis, deg), np.asarray(t, np.float64)[:, None]]).reshape(12)


def _reference_jacobians(p1, p2, T1, T2):
    """PairwiseAnalyticalDiffFunctor::Evaluate (IRLS_Cost_CPU.hpp:79-166) as written: DT1 / DT2 built block by block,
    jacob1 = e^T DT1, jacob2 = -e^T DT2, then each times ComputeJacobian of its pose."""
    T1m, T2m = T1.reshape(3, 4), T2.reshape(3, 4)
    h1, h2 = np.append(p1, 1.0), np.append(p2, 1.0)
    DT1, DT2 = np.zeros((3, 12)), np.zeros((3, 12))
    for r in range(3):
        DT1[r, 4 * r:4 * r + 4] = h1
        DT2[r, 4 * r:4 * r + 4] = h2
    e = T1m @ h1 - T2m @ h2
    return (e @ DT1) @ nm.plus_jacobian(T1), (-e @ DT2) @ nm.plus_jacobian(T2)


def test_tangent_jacobian_is_the_references_product_and_lacks_2w():
    rs = np.random.default_rng(3)
    T1 = _pose(4.0, (0.3, 1.0, 0.2), (0.1, -0.2, 0.3))
    T2 = _pose(-7.0, (1.0, 0.1, -0.4), (-0.4, 0.05, 0.2))
    P1, P2 = rs.normal(0, 2, (20, 3)), rs.normal(0, 2, (20, 3))
    w = rs.uniform(0.1, 0.9, 20)
    res, J = nm.edge_terms(P1, P2, w, T1, T2)
    for i in range(20):
        j1, j2 = _reference_jacobians(P1[i], P2[i], T1, T2)
        assert np.allclose(J[i, :6], j1, rtol=1e-12, atol=1e-12)
        assert np.allclose(J[i, 6:], j2, rtol=1e-12, atol=1e-12)
    # central differences of res through Plus: exactly 2 w times the Jacobian upstream hands to Ceres
    h = 1e-6
    for i in range(5):
        fd = np.zeros(12)
        for q in range(12):
            d = np.zeros(6)
            d[q % 6] = h
            A1, A2 = (nm.plus(T1, d), T2) if q < 6 else (T1, nm.plus(T2, d))
            B1, B2 = (nm.plus(T1, -d), T2) if q < 6 else (T1, nm.plus(T2, -d))
            fd[q] = (nm.edge_terms(P1[i:i + 1], P2[i:i + 1], w[i:i + 1], A1, A2)[0][0] -
                     nm.edge_terms(P1[i:i + 1], P2[i:i + 1], w[i:i + 1], B1, B2)[0][0]) / (2 * h)
        assert np.allclose(fd, 2.0 * w[i] * J[i], rtol=1e-6, atol=1e-8)
        assert not np.allclose(fd, J[i], rtol=1e-3)


def _exp_se3_reference(delta):
    """Exp_SE3 (LieGroup.cpp:169-192) spelled out: w = tail, u = head; Exp_SO3 and LeftJacobian_SO3 by their formulas."""
    u, w = np.asarray(delta[:3]), np.asarray(delta[3:])
    th = np.linalg.norm(w)
    A = nm.skew(w)
    if th < 1e-6:
        return np.hstack([np.eye(3), u[:, None]])
    R = np.eye(3) + (np.sin(th) / th) * A + ((1 - np.cos(th)) / th ** 2) * A @ A
    Jl = np.eye(3) + ((1 - np.cos(th)) / th ** 2) * A + ((th - np.sin(th)) / th ** 3) * A @ A
    return np.hstack([R, (Jl @ u)[:, None]])


def _expm_series(M, terms=40):
    """exp of a 4x4 matrix by its power series (independent of the closed forms of LieGroup.cpp)."""
    out, term = np.eye(4), np.eye(4)
    for k in range(1, terms):
        term = term @ M / k
        out = out + term
    return out


def test_plus_is_T_times_the_matrix_exponential_of_the_twist():
    """Plus(T, (u, w)) == T * expm([[w]x, u], [0, 0]]), the exponential taken by its power series."""
    rs = np.random.default_rng(5)
    T = _pose(12.0, (0.2, 0.5, 1.0), (1.0, -2.0, 0.5))
    T4 = np.vstack([T.reshape(3, 4), [0, 0, 0, 1]])
    for delta in [rs.normal(0, 0.2, 6) for _ in range(5)] + [np.array([0.1, 0.2, 0.3, 0, 0, 0]),
                                                              np.array([0.1, 0, 0, 1e-9, 0, 0]),
                                                              np.array([0.0, 0.3, -0.1, 0.8, -0.5, 0.4])]:
        M = np.zeros((4, 4))
        M[:3, :3], M[:3, 3] = nm.skew(delta[3:]), delta[:3]
        # below |w| = 1e-6 (TOLERANCE, LieGroup.cpp:9) Exp_SO3 returns the identity: a rotation of |w| is dropped
        tol = 1e-12 if np.linalg.norm(delta[3:]) >= 1e-6 else 1e-8
        assert np.allclose(nm.plus(T, delta), (T4 @ _expm_series(M))[:3].reshape(12), rtol=0, atol=tol)


def _oracle_A_fn(oracle, P, xyz):
    """A_fn of np_multiframe over the oracle's edge kernel (transform_pose_vec + se_kernel)."""
    po = oracle.params_from(P)

    def make(edges):
        def fn(k, pose1, pose2, ell, K):
            a, b = edges[k]
            c1 = oracle.Cloud(oracle.transform_pose_vec(pose1, xyz[a]))
            c2 = oracle.Cloud(oracle.transform_pose_vec(pose2, xyz[b]))
            mat, ind, nz = oracle.se_kernel(po, c1, c2, K, ell)
            return mat, ind, nz, int(nz.sum())
        return fn
    return make


def test_restatement_solves_descend_on_the_oracles_matrix(oracle):
    """3 frames of the street scene (1500 points), frame 0 held, the others perturbed by ~2 deg / 5 cm, the restatement
    fed by the oracle's edge kernel: every trust-region solve ends on one of its stopping rules and lowers the cost it
    minimises, and the pivot never moves.  (Pose recovery is not asserted here: on this scene at ell 0.3 upstream's
    objective, with its Jacobian, moved the worst translation error from 7.1 cm to 9.6 cm over 12 outer iterations;
    at ell 0.08 to 6.2 cm.  DESIGN.md section 4.)"""
    oracle.set_num_threads(8)
    P = cases.load_params("geometric_gpu")
    P.multiframe_ell_init, P.multiframe_ell_min, P.multiframe_ell_decay_rate = 0.3, 0.1, 0.7
    P.multiframe_num_neighbors, P.multiframe_max_iters = 64, 6
    P.multiframe_iterations_per_ell, P.multiframe_iterations_per_solve, P.multiframe_min_nonzeros = 3, 8, 300
    xyz, gt = synth.scene_sequence(3, 1500, seed=2)
    X0 = np.stack([g.reshape(12) for g in gt])
    X0[1] = _compose(X0[1], _pose(2.0, (0, 1, 0.3), (0.05, 0, -0.03)))
    X0[2] = _compose(X0[2], _pose(-1.5, (1, 0.2, 0), (-0.04, 0.03, 0.05)))
    edges = [(0, 1), (1, 2), (0, 2)]
    X, rows = nm.multiframe_align(P, xyz, X0, [True, False, False], edges, _oracle_A_fn(oracle, P, xyz)(edges))
    assert np.array_equal(X[0], X0[0])
    solved = [r for r in rows if r["solved"]]
    assert len(solved) >= 3 and all(r["accepted"] > 0 for r in solved)
    for r in solved:
        assert r["termination"] in (nm.TERM_FUNCTION, nm.TERM_GRADIENT, nm.TERM_PARAMETER, nm.TERM_ITERATIONS)
        assert r["cost_final"] < r["cost_initial"]
    assert not np.array_equal(X[1], X0[1]) and not np.array_equal(X[2], X0[2])


def _compose(A, B):
    A4, B4 = np.eye(4), np.eye(4)
    A4[:3], B4[:3] = np.asarray(A).reshape(3, 4), np.asarray(B).reshape(3, 4)
    return (A4 @ B4)[:3].reshape(12)


def test_library_exports_multiframe_entry_points_with_declared_struct_sizes():
    assert os.path.exists(_capi.LIB_PATH), "build the HIP extension first (python -m unified_cvo_amd.build)"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert "cvo_multiframe_align" in exported and "cvo_debug_irls_normal" in exported
    assert ctypes.sizeof(_capi.cvo_multiframe_info_t) == 32
    assert ctypes.sizeof(_capi.cvo_multiframe_trace_t) == 48
    header = open(os.path.join(cases.ROOT, "include", "cvo_hip.h")).read()
    assert "CVO_MULTIFRAME_MAX_FRAMES 64" in header and "CVO_MULTIFRAME_MAX_EDGES 2048" in header


def test_exact_irls_inputs_and_their_integer_reference():
    """tests/irls_cases.py, the reference of the bit-equality tests of k_irls_eval: its integers are the float64
    restatement's (cost, g, H) up to that one's rounding, the bound that makes every summation order exact (sum |term|
    below 2^53 quanta) holds with room on tables of the largest sizes the GPU tests use, and the half matrices tell R
    from R^T."""
    rs = np.random.default_rng(20)
    sizes = (300, 40, 173, 97)
    xyz = [ic.exact_cloud(rs, n) for n in sizes]
    poses = ic.exact_poses(rs, 4)
    for f, T in enumerate(poses):
        R = T.reshape(3, 4)[:, :3]
        assert set(np.abs(R).ravel()) <= {0.0, 0.5, 1.0} and np.all(np.abs(xyz[f]) <= 2)
        if f % 2 == 0:
            assert not np.array_equal(R, R.T) and not np.allclose(R @ R.T, np.eye(3))
        else:
            assert np.allclose(R @ R.T, np.eye(3)) and np.count_nonzero(R) == 3 and not np.any(np.diag(R))
    t = ic.Table()
    for k, (f1, f2, n) in enumerate([(0, 1, 12289), (3, 0, 4097), (2, 3, 0), (1, 2, 300), (3, 1, 65)]):
        t.add(f1, f2, *ic.entries(rs, sizes[f1], sizes[f2], n, empty="interleaved" if k % 2 else "none"))
    want, worst = ic.exact_table(xyz, poses, t)
    assert worst < ic.EXACT_LIMIT // 64, worst
    assert not want[2].any()
    for k in range(t.n_edges):
        f1, f2, r, c, w = t.edge(k)
        keep = c >= 0
        cost, g, H = nm.edge_normal(xyz[f1][r[keep]].astype(np.float64), xyz[f2][c[keep]].astype(np.float64),
                                    w[keep].astype(np.float64), poses[f1], poses[f2])
        got = np.concatenate([[cost], g, H[ic.TRIU]])
        _, mag = ic.exact_edge(xyz[f1], xyz[f2], r, c, w, poses[f1], poses[f2])
        S = ic.to_doubles(mag)
        assert np.all(np.abs(got - want[k]) <= 1e-13 * S), k
        if keep.any():
            # R for R^T in J changes the result on these poses (a signed permutation alone could hide it)
            Tt = poses[f1].reshape(3, 4).copy()
            Tt[:, :3] = Tt[:, :3].T
            wrong, _ = ic.exact_edge(xyz[f1], xyz[f2], r, c, w, Tt.reshape(12), poses[f2])
            assert not np.array_equal(ic.to_doubles(wrong), want[k])
    for T in poses:   # row 0 of every rotation block differs from its column 0
        R = T.reshape(3, 4)[:, :3]
        assert not np.array_equal(R[0], R[:, 0])


def test_restatement_refuses_non_finite_poses():
    xyz = [np.zeros((4, 3), np.float32)] * 2
    X0 = np.stack([np.eye(4)[:3].reshape(12)] * 2)
    for bad in (np.nan, np.inf, -np.inf):
        X = X0.copy()
        X[1, 7] = bad
        try:
            nm.multiframe_align(cases.load_params("geometric_gpu"), xyz, X, None, [(0, 1)], None)
        except ValueError:
            continue
        raise AssertionError("a non-finite pose was accepted")
