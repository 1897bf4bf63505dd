"""The multi-frame least-squares kernels on their own: k_irls_eval<true / false> + k_irls_finish through
cvo_debug_irls_eval on caller-made launch tables (bit equality against integer arithmetic on exactly representable
inputs, tests/irls_cases.py), k_irls_gather through cvo_debug_irls_gather against cvo_edge_kernel_matrix, and one
realistic table against a wider-than-double reference, per component."""
import math

import numpy as np
import pytest

import cases
import irls_cases as ic
import np_multiframe as nm
import row_classes as rcl
from unified_cvo_amd import CvoError, CvoGPU, CvoPointCloud, synth

pytestmark = pytest.mark.gpu

SIZES = (300, 40, 173, 97)   # points per frame: all different, none a multiple of a wave
BLOCK = 4096                 # IRLS_BLOCK_ENTRIES: entry slots one block of k_irls_eval walks
COUNTS = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 12289)


@pytest.fixture(scope="module")
def rig():
    """One context, four resident clouds on the exact grid and their poses (two half matrices, two signed permutations)."""
    rs = np.random.default_rng(20)
    xyz = [ic.exact_cloud(rs, n) for n in SIZES]
    poses = ic.exact_poses(rs, len(SIZES))
    gpu = CvoGPU(params=cases.load_params("geometric_gpu"))
    devs = [gpu.upload(CvoPointCloud.from_xyz(x)) for x in xyz]
    return gpu, devs, xyz, poses


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _run(rig, table, expect_zero=False):
    """Both instantiations on `table`, twice: the precondition of exactness, then bit equality with the integers."""
    gpu, devs, xyz, poses = rig
    want, worst = ic.exact_table(xyz, poses, table)
    assert worst < ic.EXACT_LIMIT, worst   # sum |term| / quantum < 2^53: every summation order gives the same double
    ef, off, r, c, w = table.arrays()
    full = gpu.debug_irls_eval(devs, poses, ef, off, r, c, w, normal=True)
    cost = gpu.debug_irls_eval(devs, poses, ef, off, r, c, w, normal=False)
    assert full.shape == (table.n_edges, ic.W) and cost.shape == (table.n_edges,)
    bad = np.argwhere(_bits(full) != _bits(want))
    assert bad.size == 0, (bad[:8], full[tuple(bad[0])], want[tuple(bad[0])])
    assert np.array_equal(_bits(cost), _bits(full[:, 0]))
    assert np.array_equal(_bits(gpu.debug_irls_eval(devs, poses, ef, off, r, c, w, normal=True)), _bits(full))
    assert np.array_equal(_bits(gpu.debug_irls_eval(devs, poses, ef, off, r, c, w, normal=False)), _bits(cost))
    if expect_zero:
        assert not full.any()
    return full


def _pair(k):
    """Frame pairs in turn, both orders (f1 > f2 included), n1 != n2."""
    return [(0, 1), (1, 0), (2, 3), (3, 1), (0, 2), (3, 0)][k % 6]


@pytest.mark.parametrize("slots", COUNTS)
def test_single_edge_slot_counts(rig, slots):
    """One edge whose slot count sits on a wave (64), a 256-thread pass or a block (4096) edge, one short and one
    beyond: cost, g and H bit for bit, the cost-only launch equal to element 0, two calls equal."""
    f1, f2 = _pair(COUNTS.index(slots))
    rs = np.random.default_rng(1000 + slots)
    full = _run(rig, ic.Table().add(f1, f2, *ic.entries(rs, SIZES[f1], SIZES[f2], slots)))
    assert full[0, 0] > 0 and full[0, 1:13].any()


@pytest.mark.parametrize("slots", [1, 257, 4096, 4097])
def test_single_edge_all_slots_empty(rig, slots):
    rs = np.random.default_rng(2000 + slots)
    _run(rig, ic.Table().add(1, 2, *ic.entries(rs, SIZES[1], SIZES[2], slots, empty="all")), expect_zero=True)


@pytest.mark.parametrize("slots", [65, 4096, 12289])
def test_single_edge_empty_slots_between_stored_ones(rig, slots):
    rs = np.random.default_rng(3000 + slots)
    r, c, w = ic.entries(rs, SIZES[3], SIZES[0], slots, empty="interleaved")
    assert (c < 0).any() and (c >= 0).any() and (c[:-1] < 0).any() and (r[c < 0] >= 0).any()
    _run(rig, ic.Table().add(3, 0, r, c, w))


def test_multi_edge_table(rig):
    """Every row of a table that mixes the counts above with zero-slot edges first, in the middle (two adjacent) and
    last, an edge with f1 > f2, the same frame pair twice with different entries, four frames of different sizes: the
    binary search over blk0 and k_irls_finish's block ranges on every edge."""
    rs = np.random.default_rng(40)
    plan = [(0, 1, 0), (0, 1, 4097), (2, 0, 64), (1, 3, 0), (3, 1, 0), (0, 1, 255), (3, 2, 4096), (1, 2, 1),
            (2, 3, 8192), (0, 3, 65), (3, 0, 12289), (1, 0, 63), (2, 1, 0)]
    t = ic.Table()
    for k, (f1, f2, n) in enumerate(plan):
        t.add(f1, f2, *ic.entries(rs, SIZES[f1], SIZES[f2], n, empty="interleaved" if k % 3 == 2 else "none"))
    assert t.frames.count((0, 1)) >= 2 and any(a > b for a, b in t.frames)
    full = _run(rig, t)
    empty = np.array([n == 0 for _, _, n in plan])
    assert not full[empty].any() and (full[~empty, 0] > 0).all()
    assert sum(-(-n // BLOCK) for _, _, n in plan) > len(plan)   # more blocks than edges: blk0 is not the edge index


def test_table_of_2048_edges(rig):
    """CVO_MULTIFRAME_MAX_EDGES edges of 0 .. 300 slots (runs of zero-slot edges among them), about 300k slots: one
    block per non-empty edge, so the search for the last edge with blk0 <= b has to step over every run."""
    rs = np.random.default_rng(41)
    counts = rs.integers(0, 301, 2048)
    for a in (0, 500, 501, 1200, 2040):   # runs of zero-slot edges: first, adjacent runs, last
        counts[a:a + 8] = 0
    counts[1000:1064] = 0
    t = ic.Table()
    for k, n in enumerate(counts):
        f1, f2 = _pair(int(rs.integers(0, 6)))
        t.add(f1, f2, *ic.entries(rs, SIZES[f1], SIZES[f2], int(n), empty="interleaved" if k % 5 == 0 else "none"))
    assert t.n_edges == 2048 and 250_000 < t.off[-1] < 350_000
    _run(rig, t)


def test_irls_eval_refuses_decreasing_offsets_and_wrong_sizes(rig):
    """Checked on the host before any launch (no out-of-range index is passed anywhere in this file)."""
    gpu, devs, xyz, poses = rig
    rs = np.random.default_rng(5)
    r, c, w = ic.entries(rs, SIZES[0], SIZES[1], 10)
    with pytest.raises(CvoError):
        gpu.debug_irls_eval(devs, poses, [[0, 1], [1, 0]], [0, 10, 4], r, c, w)
    with pytest.raises(CvoError):
        gpu.debug_irls_eval(devs, poses, [[0, 1]], [-1, 9], r, c, w)
    with pytest.raises(CvoError):
        gpu.debug_irls_gather(SIZES[0], 3)   # not the budget of an evaluation on this context (there was none)


# ---- k_irls_gather ----------------------------------------------------------------------------------------------

def _check_gather(gpu, f1, f2, ell, K):
    """After edge_kernel_matrix(f1, f2, ell, K) the gathered entries of each position are one row of (mat, ind), exactly
    and in order, under that row's original index; the slots past the row's count are (-1, -1, 0)."""
    mat, ind, nz, total = gpu.edge_kernel_matrix(f1, f2, ell, K)
    r, c, w = gpu.debug_irls_gather(f1.n, K)
    cnt = np.minimum(nz.astype(np.int64), K)
    stored = c >= 0
    n_pos = stored.sum(1)
    assert np.array_equal(stored, np.arange(K)[None, :] < n_pos[:, None])   # a row's entries come first
    assert (r[~stored] == -1).all() and (c[~stored] == -1).all() and not w[~stored].view(np.uint32).any()
    rows = np.flatnonzero(n_pos > 0)
    rid = r[rows, 0]
    assert np.array_equal(np.sort(rid), np.flatnonzero(cnt > 0))            # every non-empty row once
    assert np.array_equal(np.where(stored[rows], r[rows], -1), np.where(stored[rows], rid[:, None], -1))
    assert np.array_equal(n_pos[rows], cnt[rid])
    assert int(n_pos.sum()) == int(cnt.sum()) and (total == int(nz.sum()))
    assert np.array_equal(c[rows], np.where(stored[rows], ind[rid], -1))
    assert np.array_equal(w[rows].view(np.uint32), np.where(stored[rows], mat[rid], 0).astype(np.float32).view(np.uint32))
    return cnt


def _frames(gpu, rc):
    src, tgt = rc.clouds()
    pose = np.hstack([np.eye(3), np.zeros((3, 1))])
    return gpu.transformed(gpu.upload(src), pose), gpu.transformed(gpu.upload(tgt), pose)


def test_gather_small_rows_around_K():
    """K = 1 and K below, at and above the largest row count (7), with empty rows."""
    P = cases.load_params("geometric_gpu")
    rc = rcl.build(P, [0, 1, 2, 5, 7, 7, 3, 0, 6, 4] * 7, seed=11)
    gpu = CvoGPU(params=P)
    f1, f2 = _frames(gpu, rc)
    for K in (1, 6, 7, 8, 20):
        cnt = _check_gather(gpu, f1, f2, rc.ell, K)
        assert cnt.max() == min(K, 7) and np.array_equal(cnt, np.minimum(rc.counts, K))


@pytest.mark.parametrize("family", ["overflow", "dense_1216"])
def test_gather_row_classes(family):
    """Rows the wave-per-row kernels stored (row-major runs, dense_off) next to thread-per-row rows, cut at K: the
    overflow family (rows of 127 .. 2000 hits) and the dense-regime family (M = 1216).  The second evaluation with a
    smaller K on the same context is the driver's shrink."""
    P = cases.load_params("geometric_gpu")
    P.nearest_neighbors_max = 1025
    rc = rcl.overflow_family(P) if family == "overflow" else rcl.dense_family(P, 1216)
    gpu = CvoGPU(params=P)
    f1, f2 = _frames(gpu, rc)
    for K in (1025, 305, 64):
        cnt = _check_gather(gpu, f1, f2, rc.ell, K)
        assert np.array_equal(cnt, np.minimum(rc.counts, K)) and cnt.max() == min(K, rc.counts.max())


# ---- a realistic table ------------------------------------------------------------------------------------------

WIDE = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else None
DEVICE_MULTIPLE = 4.0


def _wide_edge(P1, P2, w, T1, T2):
    """(value[91], sum |term| [91]) of one edge in a wider arithmetic: np.longdouble where it is wider than double,
    else the float64 terms summed by math.fsum (exactly rounded sums)."""
    dt = WIDE or np.float64
    P1, P2, w, T1, T2 = (np.asarray(a, np.float64).astype(dt) for a in (P1, P2, w, T1, T2))
    T1, T2 = T1.reshape(3, 4), T2.reshape(3, 4)
    e = (P1 @ T1[:, :3].T + T1[:, 3]) - (P2 @ T2[:, :3].T + T2[:, 3])
    res = w * (e * e).sum(1)
    a, b = e @ T1[:, :3], e @ T2[:, :3]
    J = np.hstack([a, np.cross(P1, a), -b, -np.cross(P2, b)])
    cols = [0.5 * res * res] + [J[:, q] * res for q in range(12)] + [J[:, q] * J[:, s] for q in range(12) for s in range(q, 12)]
    if WIDE is not None:
        return np.array([c.sum() for c in cols]), np.array([np.abs(c).sum() for c in cols])
    return np.array([math.fsum(c) for c in cols]), np.array([math.fsum(np.abs(c)) for c in cols])


def test_realistic_table_per_component():
    """Three edges between random float32 clouds (500 / 400 / 300 points) under general rigid poses, the entries those
    of edge_kernel_matrix (K = 48, empty slots included), against np.longdouble (64-bit significand) or, where that is
    no wider than double, math.fsum over the float64 terms.

    Per component q the error is measured in units of S_q = sum over entries of |term_q|, never of the largest
    component: rho = max_q |value_q - wide_q| / S_q.  The float64 numpy evaluation (np_multiframe.edge_normal: every
    term rounded a handful of times, BLAS sums) is measured first, rho_np; the device, which forms the same terms and
    sums them in another order (16 per thread in turn, a butterfly over 64 lanes, 4 waves, the blocks in order), may be
    at most DEVICE_MULTIPLE = 4 times as far.  Why 4: the two evaluations round each term about as often and sum to a
    similar depth, so both distances are draws of one size of error, a few ulps of S_q at most; each is a maximum over
    273 components, which moves by less than a factor of 2 from draw to draw, and a second factor of 2 allows for the
    device forming a = R^T e and p x a in a different association than numpy's matrix products.  A wrong term, slot or
    block is of order S_q / entries, more than 1e10 times the bound.
    Measured on the MI355X: rho_np = 4.1e-16, the device 2.4e-16 (bound 1.65e-15)."""
    P = cases.load_params("geometric_gpu")
    rs = np.random.default_rng(77)
    xyz = [rs.uniform(-1.5, 1.5, (n, 3)).astype(np.float32) for n in (500, 400, 300)]
    poses = np.stack([np.hstack([synth.rot_axis_angle(rs.normal(size=3), rs.uniform(-25, 25)),
                                 rs.uniform(-0.2, 0.2, (3, 1))]).reshape(12) for _ in range(3)])
    gpu = CvoGPU(params=P)
    devs = [gpu.upload(CvoPointCloud.from_xyz(x)) for x in xyz]
    K, t = 48, ic.Table()
    for a, b in [(0, 1), (2, 1), (2, 0)]:
        t1, t2 = gpu.transformed(devs[a], poses[a]), gpu.transformed(devs[b], poses[b])
        mat, ind, nz, total = gpu.edge_kernel_matrix(t1, t2, 0.3, K)
        assert total > 1000 and (ind < 0).any()
        t.add(a, b, np.repeat(np.arange(len(xyz[a]), dtype=np.int32), K), ind.reshape(-1), mat.reshape(-1))
    # evaluated a little away from the poses the matrix was made at, as the solver does
    Q = np.stack([nm.plus(p, rs.normal(0, 0.01, 6)) for p in poses])
    ef, off, r, c, w = t.arrays()
    full = gpu.debug_irls_eval(devs, Q, ef, off, r, c, w, normal=True)
    cost = gpu.debug_irls_eval(devs, Q, ef, off, r, c, w, normal=False)
    rho_np = rho_dev = 0.0
    parts = []
    for k in range(3):
        f1, f2, rk, ck, wk = t.edge(k)
        keep = ck >= 0
        P1, P2, ww = xyz[f1][rk[keep]].astype(np.float64), xyz[f2][ck[keep]].astype(np.float64), wk[keep].astype(np.float64)
        wide, S = _wide_edge(P1, P2, ww, Q[f1], Q[f2])
        c64, g64, H64 = nm.edge_normal(P1, P2, ww, Q[f1], Q[f2])
        v64 = np.concatenate([[c64], g64, H64[ic.TRIU]])
        assert (S > 0).all()
        parts.append((np.abs(v64 - wide) / S, np.abs(full[k] - wide) / S, abs(cost[k] - wide[0]) / S[0]))
        rho_np = max(rho_np, float(parts[-1][0].max()))
        rho_dev = max(rho_dev, float(parts[-1][1].max()), float(parts[-1][2]))
    print(f"realistic table: rho_np = {rho_np:.3e}, device = {rho_dev:.3e}, bound = {DEVICE_MULTIPLE * rho_np:.3e}")
    assert 0 < rho_np < 1e-14
    for k, (d64, ddev, dcost) in enumerate(parts):
        assert (ddev <= DEVICE_MULTIPLE * rho_np).all(), (k, np.argmax(ddev), ddev.max(), rho_np)
        assert dcost <= DEVICE_MULTIPLE * rho_np, (k, dcost, rho_np)
