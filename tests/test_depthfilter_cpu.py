"""The keyframe depth filter without a GPU: the CPU twin (cvo_depth_filter_accumulate_host / _finish_host) against the
statement (np_depthfilter.py) bit for bit on the oracle's non-isotropic associations, a float64 second opinion of the whole
formula with a derived bound, and the edge rows of the count threshold, z0 == 0, the empty CSR and finish-then-add."""
import numpy as np
import pytest

import cases
import depthfilter_cases as dc
import np_depthfilter as npd
from unified_cvo_amd import depth_filter_accumulate_host, depth_filter_finish_host

U = 2.0 ** -24  # unit roundoff of float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _oracle_assoc(oracle, P, kf, kernel):
    ok = oracle.Cloud.from_pointcloud(kf)

    def assoc(k, pc, T):
        rp, col, val, _ = oracle.association_non_isotropic(oracle.params_from(P), ok, oracle.Cloud.from_pointcloud(pc), T, kernel)
        return rp, col, val
    return assoc


def _twin(kf_xyz, frames, assoc, min_count=3):
    state = None
    for k, (pc, T, Td) in enumerate(frames):
        rp, col, val = assoc(k, pc, T)
        if state is None:
            state = (np.zeros(len(kf_xyz), np.float32), np.zeros(len(kf_xyz), np.float32), np.zeros(len(kf_xyz), np.int32))
        depth_filter_accumulate_host(rp, col, val, pc.device_arrays()[0], Td, state)
    return state, depth_filter_finish_host(kf_xyz, state, min_count)


def _same(twin, stmt):
    (ds, ws, cnt), (xyz, kept, depth, nf) = twin
    s, (sxyz, skept, sdepth, snf) = stmt
    assert np.array_equal(cnt, s.count)
    assert np.array_equal(_bits(ds), _bits(s.depth_sum)) and np.array_equal(_bits(ws), _bits(s.weight_sum))
    assert np.array_equal(kept, skept) and nf == snf
    assert np.array_equal(_bits(depth), _bits(sdepth)) and np.array_equal(_bits(xyz), _bits(sxyz))


# (builder, its size, the kernel's scale: chosen so that rows below, on and above the count threshold all occur - asserted below)
BUILDERS = [(cases.config2, dict(n=300), 1.0), (cases.config3, dict(n=310), 4.0), (cases.config4, dict(n=290), 8.0)]


@pytest.fixture(scope="module")
def runs(oracle):
    """Per builder: the keyframe's rows, the frames with their cached oracle associations, the statement's result."""
    out = []
    for builder, kw, scale in BUILDERS:
        P, kf, tgt, _ = builder(**kw)
        n = tgt.num_points()
        frames = dc.frames_of(tgt, (n, n - 37, n // 2 + 3), seed=len(out))
        kernel = dc.rotated_kernel(scale)
        live = _oracle_assoc(oracle, P, kf, kernel)
        cache = [live(k, pc, T) for k, (pc, T, _) in enumerate(frames)]
        assoc = lambda k, pc, T, cache=cache: cache[k]  # noqa: E731
        kf_xyz = kf.device_arrays()[0]
        out.append((kf_xyz, frames, assoc, dc.statement(kf_xyz, frames, assoc)))
    return out


@pytest.mark.parametrize("which", range(len(BUILDERS)))
def test_twin_equals_statement_on_oracle_associations(runs, which):
    kf_xyz, frames, assoc, stmt = runs[which]
    s, (_, kept, _, _) = stmt
    assert sum(len(assoc(k, None, None)[1]) for k in range(len(frames))) > 100
    assert len(kept) > 0 and (s.count == 3).any() and (s.count == 4).any() and ((s.count > 0) & (s.count < 3)).any()  # (no entry at all: the hand-made rows below)
    _same(_twin(kf_xyz, frames, assoc), stmt)
    _same(_twin(kf_xyz, frames, assoc, min_count=1), dc.statement(kf_xyz, frames, assoc, min_count=1))


def _float64_opinion(kf_xyz, frames, assoc, min_count=3):
    """The whole formula in float64, row by row, written apart from the statement: per row (count, d, xyz', S) with S the
    row's magnitude scale max(|z0|, max_j |T20 x_j| + |T21 y_j| + |T22 z_j| + |T23|)."""
    n = len(kf_xyz)
    num, den, cnt, S = np.zeros(n), np.zeros(n), np.zeros(n, np.int64), np.abs(kf_xyz[:, 2].astype(np.float64))
    for k, (pc, T, Td) in enumerate(frames):
        rp, col, val = assoc(k, pc, T)
        y = pc.device_arrays()[0].astype(np.float64)
        r = np.asarray(Td, np.float32).astype(np.float64)[2]
        for i in range(n):
            for e in range(rp[i], rp[i + 1]):
                p = y[col[e]]
                num[i] += float(val[e]) * (r[0] * p[0] + r[1] * p[1] + r[2] * p[2] + r[3])
                den[i] += float(val[e])
                cnt[i] += 1
                S[i] = max(S[i], abs(r[0] * p[0]) + abs(r[1] * p[1]) + abs(r[2] * p[2]) + abs(r[3]))
    rows = np.flatnonzero(cnt > min_count)
    x = kf_xyz[rows].astype(np.float64)
    wbar = den[rows] / cnt[rows]
    d = (num[rows] + x[:, 2] * wbar) / (den[rows] + wbar)
    return rows, cnt[rows], d, x / x[:, 2:3] * d[:, None], S[rows]


@pytest.mark.parametrize("which", range(len(BUILDERS)))
def test_statement_against_a_float64_opinion(runs, which):
    """The bound, derived (u = 2^-24, gamma_k = k u / (1 - k u), every weight a > 0, W = sum a, c = count, S as above):
      * zj in float32 is 3 products and 3 sums of terms whose magnitudes sum to <= S:      |zj32 - zj| <= gamma_4 S;
      * depth_sum is c rounded products summed sequentially (c - 1 rounded sums):         |D32 - D| <= gamma_(c+4) S W;
      * weight_sum:  |W32 - W| <= gamma_(c-1) W;  wbar = W32 / c: relative gamma_c;  z0 wbar: gamma_(c+1) S W / c;
      * numerator D32 + z0 wbar, one more rounding:  |num32 - num| <= gamma_(c+6) S W (1 + 1/c);
      * denominator W32 + wbar: relative gamma_(c+2), and it is exactly W (1 + 1/c) > 0: no cancellation;
      * d = num / den, |d| <= S:   |d32 - d| <= (gamma_(c+6) + gamma_(c+3)) S <= gamma_(2c+10) S =: B_d;
      * xyz' = (p / z0) d: two more roundings on a product with d32:  |xyz'32 - xyz'| <= |p / z0| (B_d (1 + 2u) + gamma_2 S).
    The float64 opinion's own rounding is 2^-29 of that and is covered by the step from (2c + 9) to (2c + 10)."""
    kf_xyz, frames, assoc, stmt = runs[which]
    _, (sxyz, skept, sdepth, _) = stmt
    rows, c, d, xyz, S = _float64_opinion(kf_xyz, frames, assoc)
    assert np.array_equal(rows, skept)
    k = 2.0 * c + 10.0
    B_d = k * U / (1.0 - k * U) * S
    err_d = np.abs(sdepth.astype(np.float64) - d)
    print("depth: max error / bound =", float((err_d / B_d).max()))
    assert np.all(err_d <= B_d)
    ratio = np.abs(kf_xyz[rows].astype(np.float64) / kf_xyz[rows, 2:3].astype(np.float64))
    B_x = ratio * (B_d * (1.0 + 2.0 * U) + 2.0 * U / (1.0 - 2.0 * U) * S)[:, None]
    err_x = np.abs(sxyz.astype(np.float64) - xyz)
    print("xyz: max error / bound =", float((err_x / B_x).max()))
    assert np.all(err_x <= B_x)


# ---- edge rows, by hand ----

def _hand():
    """Six keyframe rows against two frames of five points.  Observations per row over (frame 0, frame 1):
    row 0: 3 + 0 (exactly min_count: dropped)   row 1: 4 + 0 (kept)   row 2: 1 + 2 (dropped)   row 3: 2 + 2 (kept)
    row 4: 4 + 0 with z0 == 0 (not finite: dropped and counted)   row 5: none."""
    kf = np.array([[0.1, 0.2, 1.5], [-0.3, 0.1, 2.0], [0.2, -0.2, 1.0], [0.4, 0.4, 3.0], [0.5, 0.1, 0.0], [1.0, 1.0, 1.0]], np.float32)
    rs = np.random.default_rng(5)
    y0, y1 = rs.uniform(-1, 3, (5, 3)).astype(np.float32), rs.uniform(-1, 3, (5, 3)).astype(np.float32)
    f0 = (np.array([0, 3, 7, 8, 10, 14, 14]), np.array([0, 2, 4, 0, 1, 2, 3, 1, 0, 4, 0, 1, 3, 4]))
    f1 = (np.array([0, 0, 0, 2, 4, 4, 4]), np.array([1, 3, 0, 2]))
    v0, v1 = rs.uniform(0.01, 0.9, 14).astype(np.float32), rs.uniform(0.01, 0.9, 4).astype(np.float32)
    Td0, Td1 = dc.rigid(3.0, (0.1, 1.0, 0.0), (0.0, 0.1, 0.2)), dc.rigid(-2.0, (1.0, 0.0, 0.3), (0.1, 0.0, -0.1))
    return kf, [(f0[0], f0[1], v0, y0, Td0), (f1[0], f1[1], v1, y1, Td1)]


def _twin_raw(kf, frames, min_count=3):
    state = None
    for rp, col, val, y, Td in frames:
        state = depth_filter_accumulate_host(rp, col, val, y, Td, state)
    return state, depth_filter_finish_host(kf, state, min_count)


def test_threshold_edges_and_zero_depth():
    kf, frames = _hand()
    s, (xyz, kept, depth, nf) = npd.run(kf, frames)
    assert s.count.tolist() == [3, 4, 3, 4, 4, 0]
    assert kept.tolist() == [1, 3] and nf == 1
    _same(_twin_raw(kf, frames), (s, (xyz, kept, depth, nf)))
    # the rows of count 3 are kept as soon as the bound is 2
    s2, fin2 = npd.run(kf, frames, min_count=2)
    assert fin2[1].tolist() == [0, 1, 2, 3] and fin2[3] == 1
    _same(_twin_raw(kf, frames, min_count=2), (s2, fin2))


def test_empty_csr_and_empty_keyframe():
    kf, frames = _hand()
    empty = (np.zeros(len(kf) + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros((0, 3), np.float32), np.eye(4))
    s, fin = npd.run(kf, [empty])
    assert not s.count.any() and len(fin[1]) == 0 and fin[3] == 0
    _same(_twin_raw(kf, [empty]), (s, fin))
    _same(_twin_raw(kf, [frames[0], empty, frames[1]]), npd.run(kf, frames))   # an empty frame in the middle changes nothing
    none = np.zeros((0, 3), np.float32)
    st, (xyz, kept, depth, nf) = _twin_raw(none, [(np.zeros(1, np.int32), [], [], frames[0][3], np.eye(4))])
    assert len(st[0]) == 0 and xyz.shape == (0, 3) and len(kept) == 0 and nf == 0


def test_finish_leaves_the_state():
    kf, frames = _hand()
    state = depth_filter_accumulate_host(*frames[0][:5])
    before = [a.copy() for a in state]
    first = depth_filter_finish_host(kf, state)
    assert all(np.array_equal(a, b) for a, b in zip(state, before))
    assert first[1].tolist() == [1] and first[3] == 1
    depth_filter_accumulate_host(*frames[1][:5], state)
    _same((state, depth_filter_finish_host(kf, state)), npd.run(kf, frames))


def test_twin_refuses_a_bad_association_before_writing():
    from unified_cvo_amd import CvoError
    kf, frames = _hand()
    rp, col, val, y, Td = frames[0]
    state = (np.full(6, 7, np.float32), np.full(6, 7, np.float32), np.full(6, 7, np.int32))
    bad_col = col.copy()
    bad_col[-1] = 5   # (the last entry of the last non-empty row: every earlier row would have been folded already)
    bad_rp = rp.copy()
    bad_rp[3] = 2
    for a, b in ((rp, bad_col), (bad_rp, col)):
        with pytest.raises(CvoError):
            depth_filter_accumulate_host(a, b, val, y, Td, state)
        assert all((x == 7).all() for x in state)
