"""The keyframe depth filter on the device (cvo_depth_filter_*) against the statement, np_depthfilter.py.

The truth is the statement fed with what code older than the filter returns: compute_association_gpu_non_isotropic for each
frame (the host CSR of the same evaluation) and download() of the frames.  "Equal" means: state() is bit for bit the
statement's accumulators; kept and depth are bit for bit; the result's download() is bitwise the statement's rows; the ordering
route, the order and the bits of an inner product against a fixed probe cloud are those of cvo_cloud_upload of those rows.  No
row is left out of any comparison.

Shapes: keyframes of 1, 64, 65, 257, 1024 and 1025 rows (the solo-pair wide phase of k_assoc_dense ends at N <= 1024); frames
of 1, 63, about 2000 and 17000 points (the last is ordered by the host: the gather by original index); the row classes of
row_classes.py - thread-per-row lists, wave-per-row rows stored slot-major and as row-major runs, wide rows around WIDE_MIN (a block per row), rows
with no entry, rows cut at nearest_neighbors_max 4 / 64 - with the populations asserted from the device's own record
(debug_rows); three frames of different sizes and an empty one in the middle."""
import numpy as np
import pytest

import cases
import depthfilter_cases as dc
import np_depthfilter as npd
import row_classes as rcl
from unified_cvo_amd import CvoGPU, CvoPointCloud

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)
U = 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _probe_cloud(pc):
    """A fixed cloud near the keyframe with its kinds of attributes: every third row, nudged."""
    return dc.subset(pc, np.arange(0, pc.num_points(), 3), shift=(0.01, -0.01, 0.02))


def _truth(gpu, kf_pc, kf_dev, frames, dev_frames, kernel, min_count):
    """The statement on the library's own exported associations and the frames as the device holds them."""
    kf_xyz = kf_pc.device_arrays()[0]
    s = npd.State(len(kf_xyz))
    for (pc, T, Td), fd in zip(frames, dev_frames):
        rp, col, val = gpu.compute_association_gpu_non_isotropic(kf_dev, fd, T, kernel)
        y = fd.download().positions()
        assert np.array_equal(_bits(y), _bits(pc.device_arrays()[0]))
        npd.add(s, rp, col, val, y, Td)
    return s, npd.finish(s, kf_xyz, min_count)


def _statement_rows(kf_pc, fin):
    """The cloud of the statement's rows: the kept keyframe rows with their moved coordinates."""
    xyz, kept = fin[0], fin[1]
    pc = kf_pc.select(kept)
    pc.positions_ = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    return pc


def _check_result(gpu, kf_pc, fin, got, probe):
    out, kept, depth, nf = got
    xyz_s, kept_s, depth_s, nf_s = fin
    assert np.array_equal(kept, kept_s) and nf == nf_s and out.n == len(kept_s)
    assert np.array_equal(_bits(depth), _bits(depth_s))
    want = _statement_rows(kf_pc, fin)
    d = out.download()
    wx, wf, wl, wg = want.device_arrays()
    gx, gf, gl, gg = d.device_arrays()
    assert np.array_equal(_bits(gx), _bits(wx))
    if len(kept_s):
        assert (gf is None) == (wf is None) and (gl is None) == (wl is None)
        assert wf is None or np.array_equal(_bits(gf), _bits(wf))
        assert wl is None or np.array_equal(_bits(gl), _bits(wl))
        assert np.array_equal(_bits(gg), _bits(wg))
    up = gpu.upload(want)
    assert out.debug_order_route() == up.debug_order_route()
    assert np.array_equal(out.debug_order(), up.debug_order())
    if len(kept_s) and probe is not None:
        a = gpu.inner_product_gpu(out, probe, EYE, 0.35)
        b = gpu.inner_product_gpu(up, probe, EYE, 0.35)
        assert np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32), (a, b)
    return out


def _run(P, kf_pc, frames, kernel, min_count=3, probe=True, one_call=True, free_keyframe=False):
    """open / add / finish against the truth, all comparisons; returns (gpu, filter (open), state, statement state, rows of
    every add)."""
    gpu = CvoGPU(params=P)
    kf_dev = gpu.upload(kf_pc)
    dev_frames = [gpu.upload(pc) for pc, _, _ in frames]
    s, fin = _truth(gpu, kf_pc, kf_dev, frames, dev_frames, kernel, min_count)
    probe_dev = gpu.upload(_probe_cloud(kf_pc)) if probe and kf_pc.num_points() >= 3 else None
    df = gpu.depth_filter_open(kf_dev)
    if free_keyframe:   # the filter holds what it needs: the caller's handle may go
        kf_dev.free()
    rows = []
    for (pc, T, Td), fd in zip(frames, dev_frames):
        df.add(fd, T, kernel, Td)
        if pc.num_points() and kf_pc.num_points():
            rows.append(df.debug_rows())
    ds, ws, cnt = df.state()
    assert np.array_equal(cnt, s.count), np.flatnonzero(cnt != s.count)[:8]
    assert np.array_equal(_bits(ds), _bits(s.depth_sum)), np.flatnonzero(_bits(ds) != _bits(s.depth_sum))[:8]
    assert np.array_equal(_bits(ws), _bits(s.weight_sum))
    _check_result(gpu, kf_pc, fin, df.finish(min_count, return_kept=True), probe_dev)
    ds2, ws2, cnt2 = df.state()   # finish leaves the state
    assert np.array_equal(cnt2, cnt) and np.array_equal(_bits(ds2), _bits(ds)) and np.array_equal(_bits(ws2), _bits(ws))
    if one_call and not free_keyframe:
        got = gpu.depth_filter(kf_dev, dev_frames, [T for _, T, _ in frames], [Td for _, _, Td in frames], kernel, min_count,
                               return_kept=True)
        _check_result(gpu, kf_pc, fin, got, probe_dev)
    return gpu, df, s, fin, rows


def _keyframe_and_frames(builder, big, N, sizes, seed):
    P, src, tgt, _ = builder(n=big)
    return P, src.select(np.arange(N)), dc.frames_of(tgt, sizes, seed=seed)


# ---- random clouds: sizes, features, kernels ----

@pytest.mark.parametrize("N,sizes", [(1, (1, 63, 2000)), (64, (63, 2000, 1)), (65, (2000, 0, 63, 1)), (257, (2000, 63, 1500)),
                                     (1024, (2000, 1700, 63)), (1025, (1999, 63, 1700))])
def test_geometry_keyframe_sizes(N, sizes):
    """Geometry only; three frames of different sizes (frame-major order), for N = 65 an empty frame in the middle."""
    P, kf, frames = _keyframe_and_frames(cases.config2, 2000, N, sizes, seed=N)
    _, _, s, fin, _ = _run(P, kf, frames, dc.rotated_kernel(1.5))
    if N >= 257:   # the threshold edge, across frames
        assert (s.count == 3).any() and (s.count == 4).any() and 0 < len(fin[1]) < N


def test_colour_keyframe_and_the_driver_kernel():
    """Colour features; diag(n, n, d) with d >> n, the driver's kernel."""
    P, kf, frames = _keyframe_and_frames(cases.config3, 2000, 1025, (2000, 1200, 63), seed=7)
    _, _, s, fin, _ = _run(P, kf, frames, dc.driver_kernel(0.02, 1.5))
    assert (s.count == 3).any() and (s.count == 4).any() and 0 < len(fin[1]) < 1025


@pytest.mark.parametrize("soft", [False, True], ids=["one_hot", "one_soft_row"])
def test_semantic_keyframe(soft):
    """Colour + class rows: every label row an exact one-hot (the result is a one-hot cloud, as the upload of its rows), and
    the same with ONE soft row among the kept rows (neither is)."""
    P, src, tgt, _ = cases.config4(n=1500)

    def harden(pc, soft_row=None):
        lab = pc.labels()
        cls = lab.argmax(1)
        hot = np.zeros_like(lab)
        hot[np.arange(len(lab)), cls] = 1.0
        if soft_row is not None:   # three quarters on its own class: it keeps its associations
            hot[soft_row] = 0.0
            hot[soft_row, cls[soft_row]], hot[soft_row, (cls[soft_row] + 1) % lab.shape[1]] = 0.75, 0.25
        pc.labels_ = hot
        return pc
    SOFT_ROW = 319   # the keyframe row with the most observations (7) here; it keeps them when softened
    kf = harden(src.select(np.arange(700)), soft_row=SOFT_ROW if soft else None)
    frames = dc.frames_of(harden(tgt), (1500, 900, 400), seed=11)
    _, _, s, fin, _ = _run(P, kf, frames, dc.rotated_kernel(8.0))
    assert 0 < len(fin[1]) < 700 and (s.count == 3).any() and (s.count == 4).any()
    assert SOFT_ROW in fin[1]   # (with soft: the result holds the soft row, so neither it nor the upload of its rows is one-hot)


def test_indefinite_kernel_has_no_cull_bound():
    P, kf, frames = _keyframe_and_frames(cases.config2, 400, 257, (400, 63), seed=3)
    frames = [(pc, EYE, Td) for pc, _, Td in frames]
    _, _, s, fin, _ = _run(P, kf, frames, np.diag([0.05, -0.08, 0.03]).astype(np.float32))
    assert s.count.max() > 3


def test_target_ordered_by_the_host():
    """A frame above 16 384 points is ordered by the host: the gather by ORIGINAL index must not see the spatial order."""
    P, src, tgt, _ = cases.config2(n=17000)
    kf = src.select(np.arange(0, 17000, 66)[:257])
    frames = dc.frames_of(tgt, (17000, 63), seed=5)
    gpu, _, s, fin, _ = _run(P, kf, frames, dc.rotated_kernel(0.6), one_call=False)
    assert gpu.upload(frames[0][0]).debug_order_route() == 0
    assert (s.count > 3).any() and (s.count <= 3).any()


def test_keyframe_freed_after_open_and_more_frames_after_finish():
    P, kf, frames = _keyframe_and_frames(cases.config2, 2000, 257, (2000, 700, 63), seed=9)
    gpu, df, s, fin, _ = _run(P, kf, frames, dc.rotated_kernel(1.5), free_keyframe=True)
    # finish, then one more frame, then finish: all adds followed by one finish
    extra = dc.frames_of(dc.subset(frames[0][0], np.arange(0, 2000, 2)), (900,), seed=10)[0]
    fd = gpu.upload(extra[0])
    df.add(fd, extra[1], dc.rotated_kernel(1.5), extra[2])
    kf_dev = gpu.upload(kf)
    rp, col, val = gpu.compute_association_gpu_non_isotropic(kf_dev, fd, extra[1], dc.rotated_kernel(1.5))
    npd.add(s, rp, col, val, extra[0].device_arrays()[0], extra[2])
    fin2 = npd.finish(s, kf.device_arrays()[0], 3)
    ds, ws, cnt = df.state()
    assert np.array_equal(cnt, s.count) and np.array_equal(_bits(ds), _bits(s.depth_sum)) and np.array_equal(_bits(ws), _bits(s.weight_sum))
    _check_result(gpu, kf, fin2, df.finish(3, return_kept=True), None)
    assert len(fin2[1]) >= len(fin[1])
    df.close()


def test_empty_keyframe_and_empty_frames():
    P, kf, frames = _keyframe_and_frames(cases.config2, 300, 64, (0, 0), seed=1)
    _, _, s, fin, _ = _run(P, kf, frames, dc.rotated_kernel())
    assert not s.count.any() and len(fin[1]) == 0
    gpu = CvoGPU(params=P)
    none = gpu.upload(CvoPointCloud.from_xyz(np.zeros((0, 3), np.float32)))
    fd = gpu.upload(frames[0][0]), gpu.upload(kf)
    with gpu.depth_filter_open(none) as df:
        df.add(fd[1], EYE, dc.rotated_kernel(), EYE)
        assert all(len(a) == 0 for a in df.state())
        out, kept, depth, nf = df.finish(return_kept=True)
        assert out.n == 0 and len(kept) == 0 and nf == 0


# ---- the row classes ----

def _row_class_frames(rc, T_depths):
    """The row-class pair as keyframe + frames: the whole target, every other target, none, the first 63 targets."""
    src, tgt = rc.clouds()
    M = rc.M
    cuts = (np.arange(M), np.arange(0, M, 2), np.zeros(0, np.int64), np.arange(min(63, M)))
    return src, [(dc.subset(tgt, idx), EYE, Td) for idx, Td in zip(cuts, T_depths)]


TDS = [dc.rigid(2.0, (0.1, 1.0, 0.3), (0.02, 0.0, 0.1)), dc.rigid(-3.0, (1.0, 0.2, 0.0), (0.0, 0.03, -0.05)), EYE,
       dc.rigid(1.0, (0.0, 0.3, 1.0), (0.01, 0.01, 0.01))]


def _iso_kernel(rc):
    """l^2 I with l the cloud's lengthscale: a member of a row's cluster (within 0.45 r_i, r_i >= the cut-off radius at l) is a
    hit, every other target is three radii away - the closed form of row_classes.py carries over to this kernel."""
    return (np.eye(3) * rc.ell ** 2).astype(np.float32)


def _expect_rows(rc, K, rows):
    """The device's record of the first add (the whole target) against the construction."""
    c = rc.counts
    n_ovf = int((rc.cand_counts > 64).sum())
    assert rows["K"] == K
    assert rows["empty"] == int((c == 0).sum())
    assert rows["full"] == int((c >= K).sum())
    assert rows["max_nnz"] == int(np.minimum(c, K).max())
    assert rows["run"] + rows["dense_slot"] == n_ovf
    assert rows["list"] == int(((c > 0) & (rc.cand_counts <= 64)).sum())


@pytest.mark.parametrize("K", [4, 64, 512])
def test_overflow_rows_slot_major_and_runs(K):
    """Two rows on each of 127 .. 2000 candidates (128-steps, WIDE_MIN 256 / 257, WIDE_CAP, LONG_CAP and beyond) and 64 empty
    rows, N = 98: the wide phase.  K = 512 leaves room beyond slot 64 and the wave-per-row rows are row-major runs; at K = 64
    and 4 there is none and they stay slot-major; every row of 127+ is cut at K."""
    P = cases.load_params("geometric_gpu")
    rc = rcl.overflow_family(P)
    Q = rc.params(K)
    src, frames = _row_class_frames(rc, TDS)
    _, _, s, fin, rows = _run(Q, src, frames, _iso_kernel(rc))
    _expect_rows(rc, K, rows[0])
    assert rows[0]["empty"] == 64 and rows[0]["list"] == 0 and rows[0]["full"] == (14 if K == 512 else 34)
    if K == 512:
        assert rows[0]["run"] == 34 and rows[0]["dense_slot"] == 0
    else:
        assert rows[0]["dense_slot"] == 34 and rows[0]["run"] == 0
    # the wide rows, from the device's record: 257 .. 1024 candidates have a long list and a block each (7 values x 2); the rows
    # of 1025+ are beyond LONG_CAP, scan all 22 500 targets and are too long for a block
    assert rows[0]["wide"] == 14
    assert (s.count == 0).any() and s.count.max() > 3


@pytest.mark.parametrize("K", [4, 64])
def test_list_rows(K):
    """64 rows on each of 0 .. 65 candidates: the thread-per-row lists (6 entries in LDS, networks of 8 .. 64), the rows of 65
    beyond them; K = 4 cuts most rows, K = 64 the rows of 64 and 65."""
    P = cases.load_params("geometric_gpu")
    rc = rcl.list_family(P)
    src, frames = _row_class_frames(rc, TDS)
    _, _, s, fin, rows = _run(rc.params(K), src, frames, _iso_kernel(rc))
    _expect_rows(rc, K, rows[0])
    assert rows[0]["empty"] == 64 and rows[0]["list"] == 14 * 64 and rows[0]["run"] + rows[0]["dense_slot"] == 64
    assert rows[0]["wide"] == 0   # (rows of 65 candidates)
    assert (s.count == 0).any() and ((s.count > 0) & (s.count <= 3)).any() and (s.count > 3).any()


@pytest.mark.parametrize("N", [1024, 1025])
def test_mixed_rows_at_the_wide_phase_boundary(N):
    """Rows of every class in one keyframe of 1024 (the last N of the solo-pair wide phase) and 1025 rows."""
    P = cases.load_params("geometric_gpu")
    rc = rcl.build(P, [300, 257, 256, 130, 70, 65, 64, 33, 9, 7, 4, 3, 2, 1], n_rows=N, seed=21)
    src, frames = _row_class_frames(rc, TDS)
    _, _, s, fin, rows = _run(rc.params(512), src, frames, _iso_kernel(rc))
    _expect_rows(rc, 512, rows[0])
    assert rows[0]["list"] == 8 and rows[0]["run"] + rows[0]["dense_slot"] == 6 and rows[0]["empty"] == N - 14
    assert rows[0]["wide"] == (2 if N == 1024 else 0)   # the rows of 300 and 257; at N = 1025 the launch is not the wide one
    assert (s.count == 3).any() and (s.count == 4).any()


def test_wide_row_over_all_targets():
    """One row over all but 24 of 1100 targets (beyond LONG_CAP: scanned literally, the wide phase), K = 304 / quarter."""
    P = cases.load_params("geometric_gpu")
    rc = rcl.wide_family(P, 1100)
    src, frames = _row_class_frames(rc, TDS)
    _, _, s, fin, rows = _run(rc.params(512), src, frames, _iso_kernel(rc))
    _expect_rows(rc, 512, rows[0])
    assert rows[0]["max_nnz"] == 512 and rows[0]["run"] + rows[0]["dense_slot"] >= 1
    assert rows[0]["wide"] == 1   # (the row of 1076 candidates: beyond LONG_CAP, so all M = 1100 <= 1216 targets, a quarter per wave)


def test_colour_list_rows():
    """The colour instantiation on the list classes (features that pass the colour kernel everywhere)."""
    P = cases.load_params("intensity_gpu")
    rc = rcl.list_family(P, colour=True)
    src, frames = _row_class_frames(rc, TDS)
    _, _, s, fin, rows = _run(rc.params(64), src, frames, _iso_kernel(rc), one_call=False)
    _expect_rows(rc, 64, rows[0])


# ---- against the oracle's association ----

def test_against_the_oracle_association(oracle):
    """Once with the oracle's association in place of the library's.  The patterns are pinned equal (test_gpu_parity.py), the
    values agree to rtol e = 2e-6 only (two exp routines).  d is a weighted mean of the observed depths and z0 with positive
    weights a_k and wbar = sum a / c; scaling every a_k by (1 + t_k), |t_k| <= e, scales wbar by a factor inside the same
    band, and a weighted mean whose weights move by a relative e moves by at most 2 e / (1 - e) times the spread (max - min)
    of what it averages.  Both sides then round in float32: twice the bound B_d = gamma_(2c+10) S of test_depthfilter_cpu.py.
    kept is compared exactly."""
    P, kf, frames = _keyframe_and_frames(cases.config3, 2000, 1025, (2000, 1200, 63), seed=7)
    kernel = dc.rotated_kernel(4.0)
    gpu = CvoGPU(params=P)
    kf_dev = gpu.upload(kf)
    ok = oracle.Cloud.from_pointcloud(kf)
    kf_xyz = kf.device_arrays()[0]
    n = len(kf_xyz)
    s = npd.State(n)
    zmin, zmax, S = kf_xyz[:, 2].astype(np.float64), kf_xyz[:, 2].astype(np.float64), np.abs(kf_xyz[:, 2].astype(np.float64))
    with gpu.depth_filter_open(kf_dev) as df:
        for pc, T, Td in frames:
            df.add(gpu.upload(pc), T, kernel, Td)
            rp, col, val, _ = oracle.association_non_isotropic(oracle.params_from(P), ok, oracle.Cloud.from_pointcloud(pc), T, kernel)
            y = pc.device_arrays()[0]
            npd.add(s, rp, col, val, y, Td)
            z = npd.depth_of(Td, y).astype(np.float64)
            r = np.abs(np.asarray(Td, np.float64)[2])
            mag = np.abs(y.astype(np.float64)) @ r[:3] + r[3]
            rows = np.repeat(np.arange(n), np.diff(rp))
            zmin, zmax, S = zmin.copy(), zmax.copy(), S.copy()
            np.minimum.at(zmin, rows, z[col])
            np.maximum.at(zmax, rows, z[col])
            np.maximum.at(S, rows, mag[col])
        out, kept, depth, nf = df.finish(return_kept=True)
        cnt = df.state()[2]
    xyz_s, kept_s, depth_s, nf_s = npd.finish(s, kf_xyz, 3)
    assert np.array_equal(cnt, s.count) and np.array_equal(kept, kept_s) and nf == nf_s and len(kept) > 100
    e = 2e-6
    k = 2.0 * s.count[kept] + 10.0
    bound = 2 * e / (1 - e) * (zmax - zmin)[kept] + 2 * (k * U / (1 - k * U)) * S[kept]
    err = np.abs(depth.astype(np.float64) - depth_s.astype(np.float64))
    print("oracle association: max error / bound =", float((err / bound).max()))
    assert np.all(err <= bound)
