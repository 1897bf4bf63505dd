"""float64 numpy restatement of multi-frame align (cvo_multiframe_align): CvoBatchIRLS::solve (IRLS.cpp:77-215) with the
Levenberg-Marquardt trust-region loop that replaces ceres::Solve.  It follows DESIGN.md section 4 line for line; every
constant carries its Ceres option name.

The kernel matrix of an edge comes from a callable, A_fn(edge, pose1_f32, pose2_f32, ell, K) -> (mat [n1 x K],
ind [n1 x K], nonzeros [n1], nonzero_sum): BinaryStateGPU::update_inner_product on the two frames transformed by their
float poses (the oracle's edge kernel on the CPU side, the library's edge_kernel_matrix in the GPU tests).
"""
import numpy as np

# Ceres Solver::Options defaults upstream does not override (IRLS.cpp:164-176 sets only the tolerances and the cap)
INITIAL_TRUST_REGION_RADIUS = 1e4   # initial_trust_region_radius
MAX_TRUST_REGION_RADIUS = 1e16      # max_trust_region_radius
MIN_TRUST_REGION_RADIUS = 1e-32     # min_trust_region_radius
MIN_RELATIVE_DECREASE = 1e-3        # min_relative_decrease
MIN_LM_DIAGONAL = 1e-6              # min_lm_diagonal
MAX_LM_DIAGONAL = 1e32              # max_lm_diagonal
MAX_CONSECUTIVE_INVALID_STEPS = 5   # max_num_consecutive_invalid_steps (the 5th invalid step in a row ends the solve)
# set by upstream (IRLS.cpp:164-166)
FUNCTION_TOLERANCE = 1e-5           # function_tolerance
GRADIENT_TOLERANCE = 1e-5           # gradient_tolerance
PARAMETER_TOLERANCE = 1e-5          # parameter_tolerance
SO3_TOLERANCE = float(np.float32(1e-6))  # LieGroup.cpp:9, a float compared with a double

TERM_NONE, TERM_FUNCTION, TERM_GRADIENT, TERM_PARAMETER, TERM_RADIUS, TERM_ITERATIONS, TERM_INVALID = range(7)


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def exp_se3(delta):
    """Exp_SE3(delta, is_wu=false) (LieGroup.cpp:169-192): u = delta[:3], w = delta[3:] -> 3x4."""
    u, w = np.asarray(delta[:3], np.float64), np.asarray(delta[3:6], np.float64)
    A = skew(w)
    th = np.sqrt(w @ w)
    R, V = np.eye(3), np.eye(3)
    if not th < SO3_TOLERANCE:
        R = np.eye(3) + np.sin(th) / th * A + (1 - np.cos(th)) / (th * th) * (A @ A)
        V = np.eye(3) + (1 - np.cos(th)) / (th * th) * A + (th - np.sin(th)) / (th ** 3) * (A @ A)
    return np.hstack([R, (V @ u)[:, None]])


def plus(T, delta):
    """LocalParameterizationSE3::Plus: T * Exp_SE3(delta) on 3x4 row-major (12-vector) poses."""
    T4 = np.eye(4)
    T4[:3] = np.asarray(T, np.float64).reshape(3, 4)
    X4 = np.eye(4)
    X4[:3] = exp_se3(delta)
    return (T4 @ X4)[:3].reshape(12)


def plus_jacobian(T):
    """LocalParameterizationSE3::ComputeJacobian (local_parameterization_se3.hpp:49-88), entry by entry: 12 x 6."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    d1, d2, d3 = T[:, 0], T[:, 1], T[:, 2]
    J = np.zeros((12, 6))
    J[0, 4], J[0, 5], J[4, 4], J[4, 5], J[8, 4], J[8, 5] = -d3[0], d2[0], -d3[1], d2[1], -d3[2], d2[2]
    J[1, 3], J[1, 5], J[5, 3], J[5, 5], J[9, 3], J[9, 5] = d3[0], -d1[0], d3[1], -d1[1], d3[2], -d1[2]
    J[2, 3], J[2, 4], J[6, 3], J[6, 4], J[10, 3], J[10, 4] = -d2[0], d1[0], -d2[1], d1[1], -d2[2], d1[2]
    J[3, 0:3], J[7, 0:3], J[11, 0:3] = T[0, :3], T[1, :3], T[2, :3]
    return J


def edge_terms(P1, P2, w, T1, T2):
    """Per entry (rows of P1 / P2 / w): residual res = w |T1 p1 - T2 p2|^2 and the tangent Jacobian [J1 | J2] (n x 12)
    as upstream writes it: J1 = e^T [R1, -R1 [p1]x] = [a, p1 x a], a = R1^T e; J2 = -[b, p2 x b], b = R2^T e."""
    T1 = np.asarray(T1, np.float64).reshape(3, 4)
    T2 = np.asarray(T2, np.float64).reshape(3, 4)
    e = (P1 @ T1[:, :3].T + T1[:, 3]) - (P2 @ T2[:, :3].T + T2[:, 3])
    res = w * np.einsum("ij,ij->i", e, e)
    a = e @ T1[:, :3]
    b = e @ T2[:, :3]
    J = np.hstack([a, np.cross(P1, a), -b, -np.cross(P2, b)])
    return res, J


def edge_normal(P1, P2, w, T1, T2):
    """(cost, g[12], H 12x12) of one edge: what k_irls_normal reduces."""
    res, J = edge_terms(P1, P2, w, T1, T2)
    return 0.5 * float(res @ res), J.T @ res, J.T @ J


def edge_entries(mat, ind, x1, x2):
    """Stored entries (r, c, w) of an edge's kernel matrix in the reference's host layout -> (P1, P2, w) in double."""
    r, s = np.nonzero(ind >= 0)
    c = ind[r, s]
    return x1[r].astype(np.float64), x2[c].astype(np.float64), mat[r, s].astype(np.float64)


def solve(X, free, edges_terms, max_iterations, eval_cost, normal=None):
    """One trust-region solve.  X: F x 12 poses (modified copy returned); free: F bools; edges_terms: list of
    (f1, f2, P1, P2, w).  Returns (X, dict(steps, accepted, termination, cost_initial, cost_final, events)).
    normal (optional): stands in for edge_normal, (P1, P2, w, T1, T2) -> (cost, g[12], H 12x12) of one edge - the
    synthetic records of tests/test_irls_solve_cpu.py."""
    X = X.copy()
    F = X.shape[0]
    fi = -np.ones(F, int)
    fi[free] = np.arange(int(np.sum(free)))
    m = 6 * int(np.sum(free))

    one_edge = normal or edge_normal

    def normal(Y):
        H, g, cost = np.zeros((m, m)), np.zeros(m), 0.0
        for f1, f2, P1, P2, w in edges_terms:
            c, ge, He = one_edge(P1, P2, w, Y[f1], Y[f2])
            cost += c
            idx = [6 * fi[f1] + q if fi[f1] >= 0 else -1 for q in range(6)] + \
                  [6 * fi[f2] + q if fi[f2] >= 0 else -1 for q in range(6)]
            for i in range(12):
                if idx[i] < 0:
                    continue
                g[idx[i]] += ge[i]
                for j in range(12):
                    if idx[j] >= 0:
                        H[idx[i], idx[j]] += He[i, j]
        return cost, g, H

    def plus_all(Y, d, sign):
        Z = Y.copy()
        for f in range(F):
            if fi[f] >= 0:
                Z[f] = plus(Y[f], sign * d[6 * fi[f]:6 * fi[f] + 6])
        return Z

    def gradient_small(Y, g):  # gradient_tolerance: |x - Plus(x, -g)|_inf
        Z = plus_all(Y, g, -1.0)
        return float(np.max(np.abs(Y[free] - Z[free]), initial=0.0)) <= GRADIENT_TOLERANCE

    cost, g, H = normal(X)
    out = dict(steps=0, accepted=0, termination=TERM_NONE, cost_initial=cost, cost_final=cost, events=[])
    sc = 1.0 / (1.0 + np.sqrt(np.diag(H)))  # Jacobi scaling from the first Jacobian
    mu, decrease, invalid = INITIAL_TRUST_REGION_RADIUS, 2.0, 0
    term = TERM_GRADIENT if gradient_small(X, g) else TERM_NONE
    while term == TERM_NONE:
        if out["steps"] >= max_iterations:
            term = TERM_ITERATIONS
            break
        out["steps"] += 1
        s2 = sc * sc
        D = np.clip(s2 * np.diag(H), MIN_LM_DIAGONAL, MAX_LM_DIAGONAL) / s2
        try:
            L = np.linalg.cholesky(H + np.diag(D / mu))
            d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
            model = -(g @ d + 0.5 * d @ H @ d)
            valid = bool(np.isfinite(model) and model > 0)
        except np.linalg.LinAlgError:
            valid = False
        if valid:
            xn = np.sqrt(np.sum(X[free] ** 2))
            if np.sqrt(d @ d) <= PARAMETER_TOLERANCE * (xn + PARAMETER_TOLERANCE):
                term = TERM_PARAMETER
                break
            Xc = plus_all(X, d, 1.0)
            cost_new = eval_cost(Xc)
            valid = bool(np.isfinite(cost_new))
        if not valid:
            out["events"].append("invalid")
            invalid += 1
            if invalid >= MAX_CONSECUTIVE_INVALID_STEPS:  # HandleInvalidStep: ++count >= max fails
                term = TERM_INVALID
                break
        else:
            invalid = 0
            rho = (cost - cost_new) / model
            if rho > MIN_RELATIVE_DECREASE:
                out["events"].append("accept")
                X = Xc
                mu = min(MAX_TRUST_REGION_RADIUS, mu / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
                decrease = 2.0
                out["accepted"] += 1
                cost_old = cost
                cost, g, H = normal(X)
                out["cost_final"] = cost
                if abs(cost_old - cost_new) / cost_old <= FUNCTION_TOLERANCE:
                    term = TERM_FUNCTION
                    break
                if gradient_small(X, g):
                    term = TERM_GRADIENT
                    break
                continue
            out["events"].append("reject")
        mu /= decrease
        decrease *= 2.0
        if mu < MIN_TRUST_REGION_RADIUS:
            term = TERM_RADIUS
            break
    out["termination"] = term
    return X, out


def multiframe_align(params, xyz, poses, hold_const, edges, A_fn):
    """CvoBatchIRLS::solve.  params: a CvoParams-like object; xyz: F clouds (n x 3 float32, untransformed); poses:
    F x 12 doubles; edges: list of (frame1, frame2).  Returns (poses, trace rows as dicts)."""
    X = np.array(poses, np.float64).reshape(-1, 12).copy()
    if not np.all(np.isfinite(X)):  # cvo_multiframe_align: CVO_E_INVALID before anything is written
        raise ValueError("non-finite pose")
    F = X.shape[0]
    free = np.array([not (hold_const is not None and hold_const[f]) for f in range(F)])
    K0 = int(params.multiframe_num_neighbors)
    E = len(edges)
    Kn, lastmax = [K0] * E, [0] * E
    ell_e = [np.float32(params.multiframe_ell_init)] * E
    ell = float(np.float32(params.multiframe_ell_init))
    ell_min, rate = float(np.float32(params.multiframe_ell_min)), float(np.float32(params.multiframe_ell_decay_rate))
    it, last_nonzeros, converged, rows = 0, 0, False, []
    while not converged:
        Xf = X.astype(np.float32)  # CvoFrameGPU::transform_pointcloud casts the pose to float
        counter, total, terms = 0, 0, []
        for k, (a, b) in enumerate(edges):
            if lastmax[k] > 0:
                Kn[k] = min(K0, int(lastmax[k] * 1.1))
            mat, ind, nz, s = A_fn(k, Xf[a], Xf[b], float(ell_e[k]), Kn[k])
            lastmax[k] = int(np.max(nz)) if len(nz) else 0
            total += int(s)
            if int(s) > params.multiframe_min_nonzeros:
                counter += 1
                P1, P2, w = edge_entries(mat, ind, xyz[a], xyz[b])
                terms.append((a, b, P1, P2, w))
        row = dict(iter=it, n_active_edges=counter, solved=0, steps=0, accepted=0, termination=0,
                   ell=float(np.float32(ell)), total_nonzeros=total, cost_initial=0.0, cost_final=0.0, events=[])
        if counter == 0 or it == params.multiframe_max_iters:
            rows.append(row)
            break
        if total > last_nonzeros or it < params.multiframe_iterations_per_ell:
            last_nonzeros = total

            def eval_cost(Y):
                return sum(0.5 * float(np.sum(edge_terms(P1, P2, w, Y[f1], Y[f2])[0] ** 2))
                           for f1, f2, P1, P2, w in terms)

            X, o = solve(X, free, terms, params.multiframe_iterations_per_solve, eval_cost)
            row.update(solved=1, steps=o["steps"], accepted=o["accepted"], termination=o["termination"],
                       cost_initial=o["cost_initial"], cost_final=o["cost_final"], events=o["events"])
        else:
            if ell >= ell_min:
                last_nonzeros = 0
                ell = ell * rate
                for k in range(E):
                    if ell_e[k] > np.float32(params.multiframe_ell_min):
                        ell_e[k] = np.float32(ell_e[k] * np.float32(params.multiframe_ell_decay_rate))
            else:
                converged = True
            if it > params.multiframe_max_iters:
                converged = True
        rows.append(row)
        it += 1
    return X, rows
