"""k_kd_order (cvo_k_cloud.h) on the MI355X across its size classes: every NP from 1024 to 16384 (the renumbering pass
with 1, 2, 4, 8 and 16 positions per thread), both sides of every split unit (4 / 64 / 512) and of every power of two,
clouds full of ties, one launch over clouds of mixed sizes and attributes, and the attribute gathers per size class.

Three opinions on every ordering: the device (default context), its host twin (ORDER=virtual: std::nth_element) and the
numpy statement np_kd.order.  They agree on the point SET of every leaf - every aligned run of 4 sorted positions - not on
the order inside a leaf, which nothing reads.  Every comparison is exact; the one tolerance is TOL_IP_REL of
test_gpu_parity.py, on the float64 value of an inner product."""
import numpy as np
import pytest

import cases
import np_kd
import np_reference as npr
from test_gpu_parity import TOL_IP_REL
from unified_cvo_amd import CvoGPU, CvoPointCloud, synth

pytestmark = pytest.mark.gpu

SIZES = (8, 9, 12, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193,
         16383, 16384)


@pytest.fixture(scope="module")
def contexts():
    """(default context: the device orders; its host twin)"""
    d, v = CvoGPU(), CvoGPU()
    v.set_option("ORDER", "virtual")
    yield d, v
    d.close()
    v.close()


def _three_opinions(contexts, x, name):
    d, v = contexts
    n = x.shape[0]
    pc = CvoPointCloud.from_xyz(x)
    cd, cv = d.upload(pc), v.upload(pc)
    try:
        od, ov = cd.debug_order(), cv.debug_order()
    finally:
        cd.free()
        cv.free()
    assert np.array_equal(np.sort(od), np.arange(n)), name
    assert np.array_equal(np.sort(ov), np.arange(n)), name
    want = np_kd.leaf_sets(np_kd.order(x))
    assert np.array_equal(np_kd.leaf_sets(ov), want), (name, "host twin against the statement")
    assert np.array_equal(np_kd.leaf_sets(od), want), (name, "device against the statement")


@pytest.mark.parametrize("n", SIZES)
def test_every_size_class(contexts, n):
    """synth.geometric_pair sources: x in +-10 s and y in +-2 carry negative coordinates at every size, z (2 .. 2 + 28 s)
    none; s = (n / 10000)^(1/3)."""
    x = synth.geometric_pair(n, 7)[0]
    assert (x[:, 0] < 0).any() and (x[:, 1] < 0).any() and not (x[:, 2] < 0).any()
    _three_opinions(contexts, x, n)


@pytest.mark.parametrize("n", [600, 4097])
@pytest.mark.parametrize("kind", list(np_kd.DEGENERATE))
def test_degenerate_clouds(contexts, kind, n):
    """Ties along every axis (lattice, identical points, a plane, a line), ties between the axes (cube), subnormal to 1e30
    coordinates, and +0.0 / -0.0 - which the host twin's float comparison holds equal, so the device's integer key must too
    (test_kd_cpu.py shows that a plain bit-pattern key fills these leaves differently; with kd_ordered taking the raw bits,
    as it did before, the four signed-zero cases here fail on the MI355X, device against statement, and nothing else in
    this module does)."""
    _three_opinions(contexts, np_kd.DEGENERATE[kind](n), (kind, n))


def _mixed_clouds():
    """Eight clouds for one upload_many: every NP class, the three host-ordered kinds (fewer than 8 points, more than 16384,
    a NaN), every attribute kind."""
    rs = np.random.default_rng(31)
    geo = lambda n: np.where(rs.random((n, 1)) < 0.5, [[1.0, 0.0]], [[0.3, 0.9]]).astype(np.float32)
    soft = lambda x: (0.9 * synth.checkerboard_labels(x) + 0.1 / synth.NUM_CLASSES).astype(np.float32)
    xyz = {n: synth.geometric_pair(n, 20 + k)[0] for k, n in enumerate((8, 700, 1025, 16384, 5, 20000, 100, 4097))}
    xyz[100] = xyz[100].copy()
    xyz[100][17, 1] = np.nan
    colour = lambda x: synth.colour_features(x, rs).astype(np.float32)
    return [
        ("bare8", CvoPointCloud.from_xyz(xyz[8])),
        ("colour700", CvoPointCloud.from_arrays(xyz[700], colour(xyz[700]), None, geo(700))),
        ("soft1025", CvoPointCloud.from_arrays(xyz[1025], colour(xyz[1025]), soft(xyz[1025]), geo(1025))),
        ("onehot16384", CvoPointCloud.from_arrays(xyz[16384], None, synth.checkerboard_labels(xyz[16384]), geo(16384))),
        ("bare5", CvoPointCloud.from_xyz(xyz[5])),
        ("colour20000", CvoPointCloud.from_arrays(xyz[20000], colour(xyz[20000]), None, geo(20000))),
        ("nan100", CvoPointCloud.from_xyz(xyz[100])),
        ("geotype4097", CvoPointCloud.from_arrays(xyz[4097], None, None, geo(4097))),
    ]


@pytest.mark.parametrize("threads", [1, 4])
def test_one_launch_over_mixed_clouds(threads):
    """upload_many: one block per cloud, the dynamic LDS sized for the largest NP of the call (16384), blocks with NP = 1024
    next to it; the orderings are those of single uploads, attributes or not."""
    clouds = _mixed_clouds()
    gpu, host = CvoGPU(), CvoGPU()
    host.set_option("ORDER", "host")
    try:
        many = gpu.upload_many([pc for _, pc in clouds], threads=threads)
        assert len(many) == len(clouds)
        for (name, pc), m in zip(clouds, many):
            one = gpu.upload(pc)
            o = m.debug_order()
            assert m.n == pc.num_points() and np.array_equal(o, one.debug_order()), name
            if name in ("bare5", "nan100"):
                assert np.array_equal(o, np.arange(m.n)), name                      # the identity
            elif name == "colour20000":                                            # above KD_MAX_POINTS: the host's own rule
                h = host.upload(pc)
                assert np.array_equal(o, h.debug_order()) and np.array_equal(np.sort(o), np.arange(m.n))
                h.free()
            else:
                assert np.array_equal(np_kd.leaf_sets(o), np_kd.leaf_sets(np_kd.order(pc.positions()))), name
            one.free()
        for m in many:
            m.free()
    finally:
        gpu.close()
        host.close()


# ---- the attribute gathers inside k_kd_order, per size class ----

ELL = 0.3
GATHER_SIZES = (8, 65, 1025, 4097, 16384)


def _gather_case(kind, n):
    """(params, source of n points, target of n + 3) with the attributes of `kind`; the target is the source's scene after
    the synthetic motion, brought back (as float32 inputs), so that the identity pose overlaps them."""
    m = n + 3
    src, tgt, perm = synth.geometric_pair(n, 11, m=m)
    T = synth.gt_motion()
    tgt = ((tgt.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    rs = np.random.default_rng(100 + n)
    both = np.zeros((m, 3), np.float32)
    both[perm] = tgt                                               # (row i: the target point that was scene point i)
    fs = ft = ls = lt = None
    gs, gt_ = np.tile([[0.0, 1.0]], (n, 1)).astype(np.float32), np.tile([[0.0, 1.0]], (m, 1)).astype(np.float32)
    if kind == "colour":
        P = cases.load_params("intensity_gpu")
        f = synth.colour_features(both, rs)
        fs, ft = f[:n].astype(np.float32), np.clip(f + rs.normal(0, 0.01, f.shape), 0, 1).astype(np.float32)[perm]
    elif kind in ("soft", "onehot"):
        P = cases.load_params("semantic_img_gpu0")
        f = synth.colour_features(both, rs)
        fs, ft = f[:n].astype(np.float32), np.clip(f + rs.normal(0, 0.01, f.shape), 0, 1).astype(np.float32)[perm]
        l = synth.checkerboard_labels(both)
        lflip = synth.checkerboard_labels(both, flip=0.05, rng=rs)
        if kind == "soft":  # (half way to uniform: a pair of different classes stays above sp_thres, the rows' arithmetic counts)
            l, lflip = (0.5 * l + 0.5 / synth.NUM_CLASSES).astype(np.float32), (0.5 * lflip + 0.5 / synth.NUM_CLASSES).astype(np.float32)
        ls, lt = l[:n], lflip[perm]
    else:  # the parameters of test_single_iteration_geometric_type_and_range_ell
        P = cases.load_params("geometric_gpu")
        P.is_using_geometric_type = 1
        P.is_using_range_ell = 1
        gs = np.where(rs.random((n, 1)) < 0.5, [[1.0, 0.0]], [[0.0, 1.0]]).astype(np.float32)
        gt_ = np.where(rs.random((m, 1)) < 0.5, [[1.0, 0.0]], [[0.3, 0.9]]).astype(np.float32)
    return P, CvoPointCloud.from_arrays(src, fs, ls, gs), CvoPointCloud.from_arrays(tgt, ft, lt, gt_)


def _float64_inner_product(P, a, b, ell):
    """sum of np_reference.kernel_matrix, float64.  The matrix is evaluated in slabs of 256 source rows (sorted along z)
    against the targets within the distance cut-off of the slab (plus a margin) - every other entry is an exact zero of
    the same matrix (dense, 16384 x 16387 float64 entries are 2 GB for each of kernel_matrix's intermediate arrays).  Also returns the largest row count (the first-K truncation must not bind)."""
    x, y = a.positions(), b.positions()
    K = int(P.nearest_neighbors_max)
    sp, s2 = float(np.float32(P.sp_thres)), float(np.float32(P.sigma)) ** 2
    lmax = (float(np.linalg.norm(x.astype(np.float64), axis=1).max()) / 500.0 + 1.0) * ell
    reach = np.sqrt(-2.0 * lmax * lmax * np.log(sp / s2)) * 1.01 + 1e-3
    by = np.argsort(x[:, 2], kind="stable")
    opt = lambda arr, idx: None if arr is None or arr.shape[0] == 0 or arr.shape[1] == 0 else arr[idx]
    fa, fb = (a.features(), b.features()) if P.is_using_intensity else (None, None)
    la, lb = (a.labels(), b.labels()) if P.is_using_semantics else (None, None)
    total, widest = 0.0, 0
    for i0 in range(0, len(by), 256):
        rows = by[i0:i0 + 256]
        z0, z1 = x[rows, 2].min(), x[rows, 2].max()
        cols = np.flatnonzero((y[:, 2] >= z0 - reach) & (y[:, 2] <= z1 + reach))
        if len(cols) == 0:
            continue
        A, keep = npr.kernel_matrix(P, x[rows], y[cols], opt(fa, rows), opt(fb, cols), opt(la, rows), opt(lb, cols),
                                    a.geometric_types().reshape(-1, 2)[rows], b.geometric_types().reshape(-1, 2)[cols], K, ell)
        total += float(A.sum())
        widest = max(widest, int(keep.sum(axis=1).max()))
    return total, widest


@pytest.mark.parametrize("n", GATHER_SIZES)
@pytest.mark.parametrize("kind", ["colour", "soft", "onehot", "geotype"])
def test_attribute_gathers_per_size_class(kind, n):
    """Colour (5 -> 8 floats), class rows (19 -> 20), one-hot ids and geometric types are gathered into spatial order by
    k_kd_order itself.  <source, target> over clouds ordered by the device, by the host (ORDER=host, ORDER=virtual) and not
    at all (NO_SORT=1) is one bit pattern - a row gathered from the wrong point changes it - and that value is the float64
    sum of np_reference.kernel_matrix to the tolerance test_inner_product_and_function_angle holds the same call to."""
    P, a, b = _gather_case(kind, n)
    init = np.eye(4, dtype=np.float32)
    want, widest = _float64_inner_product(P, a, b, ELL)
    assert want > 0 and widest < P.nearest_neighbors_max, (want, widest)
    values = {}
    for opt, val in ((None, None), ("ORDER", "host"), ("ORDER", "virtual"), ("NO_SORT", "1")):
        g = CvoGPU(params=P)
        try:
            if opt:
                g.set_option(opt, val)
            da, db = g.upload(a), g.upload(b)
            values[(opt, val)] = np.float32(g.inner_product_gpu(da, db, init, ELL))
            assert g.debug_last_score_batch() == (1, 0, 1), (opt, val)      # the overlap kernel alone: no row exceeded K
            if opt is None:
                assert not np.array_equal(da.debug_order(), np.arange(n))   # (the device did reorder the rows it gathered)
        finally:
            g.close()
    got = values[(None, None)]
    print(f"{kind} n={n}: device {float(got)!r} float64 {want!r} rel {abs(float(got) - want) / want:.2e}")
    assert got > 0
    for k, v in values.items():
        assert v.view(np.uint32) == got.view(np.uint32), (k, float(v), float(got))
    assert float(got) == pytest.approx(want, rel=TOL_IP_REL, abs=1e-12)
