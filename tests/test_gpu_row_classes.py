"""The association kernels with rows placed exactly on their class and capacity limits (row_classes.py), against the
closed form, the float64 reference values and the oracle.

Limits covered (parameters / docstrings below name each):
  * k_assoc: the first 6 ELL entries of a row parked in LDS;
  * k_list: sort_and_store_list<8 / 16 / 32 / 64>; ASSOC_CAP32 = 32 / ASSOC_CAP16 = 64 (thread-per-row vs k_assoc_dense);
  * k_assoc_dense / k_coeff_dense: 128-candidate steps, 64-term batches, 128-slot replay blocks;
  * k_assoc_dense's wide phase: WIDE_MIN = 256 / 257, quarters of WIDE_CAP = 304, rows of up to 4 x 304 = 1216;
  * LONG_CAP = 1024 / 1025: cached long list vs literal scan;
  * M = 65535 / 65536: 16- vs 32-bit candidate lists, long lists on vs off;
  * K = c - 1, c, c + 1: first-K truncation, and k_overlap's void rule (more than K pairs);
  * SB_CHUNK_TILES = 65536 row tiles per k_overlap_table launch.
"""
import numpy as np
import pytest

import cases
import row_classes as rcl
from test_gpu_parity import _cmp_trace, _follow_oracle
from unified_cvo_amd import CvoGPU

pytestmark = pytest.mark.gpu

ASSOC_CAP16, ASSOC_CAP32, LONG_CAP = 64, 32, 1024
EYE = np.eye(4, dtype=np.float32)
# The device computes d^2 in float and exp() in float: the kernel value's relative error against float64 is a few float
# ulps of exp's argument (|d^2 / 2 l^2| <= 0.71 inside the clusters, so ~1e-7 absolute on it) plus exp's own ulp: 2e-6
# bounds both with room and is still a thousand times tighter than any wrong row, slot or column would be.
TOL_F64 = 2e-6


def _params(colour=False, K=512):
    P = cases.load_params("intensity_gpu" if colour else "geometric_gpu")
    P.nearest_neighbors_max = max(K, 512)
    return P


def _expected_classes(rc):
    """(overflow rows, literally scanned rows) of the first list build (k_list):
      * a row overflows when it has more candidates than min(row_max, ASSOC_CAP) (cvo_k_list.h:85), where row_max is
        ASSOC_CAP16 at the first build (cvo_update.h:362, INIT) and ASSOC_CAP is 64 for 16-bit lists, 32 for 32-bit ones
        (M >= 65536, cvo_sched.hip: idx16 = M < 65536);
      * an overflow row is scanned literally when it is beyond a long list (more than LONG_CAP candidates), or always when
        there are no long lists (M > 65535: cvo_sched.hip, long_lists = M <= 65535) - cvo_k_list.h:291."""
    cap = ASSOC_CAP16 if rc.M < 65536 else ASSOC_CAP32
    cand = rc.cand_counts  # (a row's class follows its geometric candidates; its hits may be fewer: test_gpu_feature_gates.py)
    ovf = cand > cap
    long_lists = rc.M <= 65535
    scan = ovf & (cand > LONG_CAP) if long_lists else ovf
    return int(ovf.sum()), int(scan.sum())


def _oracle_clouds(oracle, src, tgt):
    return oracle.Cloud.from_pointcloud(src), oracle.Cloud.from_pointcloud(tgt)


def _iteration0(oracle, rc, K, classes=True, tol_f64=TOL_F64):
    """One align iteration at (ell, K) from the identity: the ELL against the closed form (bit-exact pattern, values to
    TOL_F64) and the oracle (bit-exact pattern, values to an ulp), trace 0 against the oracle, and the row classes.  A cloud
    of a rejecting feature kind brings its own switches and cut-offs (and its caller the bound against float64)."""
    P = _params(rc.fsrc is not None, K) if rc.kind is None else rc.params(max(K, 512))
    src, tgt = rc.clouds()
    gpu = CvoGPU(params=P)
    g = gpu.align(src, tgt, EYE, max_iterations=1, ell0=rc.ell, K0=K, trace_capacity=2, trace_dense=2)
    mat, ind, nz = gpu.debug_last_ell(rc.N, K)
    cnz, cind, cmat = rc.closed_form(K)
    valid = np.arange(K)[None, :] < cnz[:, None]
    assert np.array_equal(nz, cnz), (K, np.flatnonzero(nz != cnz)[:8])
    assert np.array_equal(np.where(valid, ind, -1), cind), (K, np.flatnonzero((np.where(valid, ind, -1) != cind).any(1))[:8])
    assert np.allclose(np.where(valid, mat, 0), cmat, rtol=tol_f64, atol=0), K
    ox, oy = _oracle_clouds(oracle, src, tgt)
    o = oracle.iteration(oracle.params_from(P), ox, oy, EYE[:3, :3], EYE[:3, 3], rc.ell, K, want_ell=True)
    assert np.array_equal(nz, o["nonzeros"]) and np.array_equal(ind, o["ind"])
    assert np.allclose(mat, o["mat"], rtol=2e-7, atol=0)  # 1 float ulp: exp() of two libms
    assert len(g.trace) == 1
    _cmp_trace(g.trace[0], o["trace"])
    if classes:
        n_ovf, n_scan, dense = gpu.debug_row_classes()
        assert (n_ovf, n_scan, dense) == _expected_classes(rc) + (False,), K
    return gpu


K_SWEEP = (1, 6, 8, 64, 65, 128, 129, 256, 257, 304, 305, 512, 1024, 1216)


@pytest.mark.parametrize("K", K_SWEEP)
@pytest.mark.parametrize("family", ["list", "list_colour", "overflow"])
def test_iteration0_ell_on_every_row_class(oracle, family, K):
    """Rows of 0 .. 65 candidates (6 in LDS, networks 8 / 16 / 32 / 64, ASSOC_CAP16 = 64 / 65) and of 127 .. 2000
    (128-steps, WIDE_MIN 256 / 257, WIDE_CAP 304 / 305, 384 / 385, LONG_CAP 1023 / 1024 / 1025, 1215 / 1216 / 1217), solo
    pair, across the first-K limits."""
    P = _params(family.endswith("colour"))
    rc = {"list": lambda: rcl.list_family(P), "list_colour": lambda: rcl.list_family(P, colour=True),
          "overflow": lambda: rcl.overflow_family(P)}[family]()
    _iteration0(oracle, rc, K)


@pytest.mark.parametrize("K", [256, 304, 305, 384, 512])
@pytest.mark.parametrize("low", [True, False], ids=["low", "spread"])
@pytest.mark.parametrize("M", rcl.WIDE_M)
def test_wide_rows(oracle, M, low, K):
    """k_assoc_dense's wide phase (a solo pair with N <= 1024): a big row over all M targets when it is beyond LONG_CAP
    (n_cand = M), or its long list.  M in 1025 .. 1216 with K > 304 puts more than WIDE_CAP = 304 hits into one wave's
    quarter unless the quarters are at most 304 candidates long; 'low' fills the first quarter completely, 'spread'
    nearly so.  M = 1217 is beyond the wide phase (a wave per row)."""
    P = _params()
    _iteration0(oracle, rcl.wide_family(P, M, low=low), K)


@pytest.mark.parametrize("M", [1100, 1216])
def test_dense_regime_wide_rows(oracle, M):
    """More than half of the rows overflow and M <= 2048: the pair enters the dense regime after its first build and every
    row is evaluated over all M targets in the wide phase, row 0 with 400 hits on the lowest indices at K = 512."""
    P = _params()
    rc = rcl.dense_family(P, M)
    src, tgt = rc.clouds()
    gpu = CvoGPU(params=P)
    g = gpu.align(src, tgt, EYE, max_iterations=3, trace_capacity=3, trace_dense=3)
    ox, oy = _oracle_clouds(oracle, src, tgt)
    o = oracle.align(oracle.params_from(P), ox, oy, EYE, trace_capacity=3, trace_dense=3, max_iterations=3)
    assert g.iterations == o["iterations"] == 3 and len(g.trace) == len(o["trace"]) == 3
    for a, b in zip(g.trace, o["trace"]):
        _cmp_trace(a, b)
    assert gpu.debug_row_classes()[2]
    assert g.trace[0].nnz == int(np.minimum(rc.counts, P.nearest_neighbors_max).sum())
    assert cases.max_abs_diff(g.transform, o["transform"]) <= 1e-6


@pytest.mark.parametrize("n_pairs", [4, 8, 17])
def test_batch_contexts(oracle, n_pairs):
    """The list and overflow families as pairs of one align_batch (row_max_busy 8 / 24 / 64; k_coeff_dense's
    8-rows-per-wave mode from 8 pairs), a different shuffle per pair: every pair's exported association is the closed
    form and its trace the oracle's."""
    P = _params()
    P.is_exporting_association = 1
    rcs = [(rcl.list_family if p % 2 == 0 else rcl.overflow_family)(P, seed=100 + p) for p in range(n_pairs)]
    clouds = [rc.clouds() for rc in rcs]
    gpu = CvoGPU(params=P)
    res = gpu.align_batch([c[0] for c in clouds], [c[1] for c in clouds], [EYE] * n_pairs, max_iterations=1,
                          trace_capacity=2, trace_dense=2)
    K = P.nearest_neighbors_max
    same_stride = 0
    for p, (rc, (src, tgt), r) in enumerate(zip(rcs, clouds, res)):
        rp, col, val, kw, kr = gpu.align_association(rc.N, pair=p)
        assert kw == K, (p, kw)
        if kw == kr:  # (the overflow family: rows on K_max keep K; the list family's K drops to 1.2 x 65)
            crp, ccol = rc.csr(K)
            assert np.array_equal(rp, crp) and np.array_equal(col, ccol), p
            same_stride += 1
        erp, ecol, eval_ = _export_readback(rc, kw, kr)
        assert np.array_equal(rp, erp) and np.array_equal(col, ecol), (p, kw, kr)
        assert np.allclose(val, eval_, rtol=TOL_F64, atol=0), p
        ox, oy = _oracle_clouds(oracle, src, tgt)
        o = oracle.iteration(oracle.params_from(P), ox, oy, EYE[:3, :3], EYE[:3, 3], P.ell_init, K)
        assert len(r.trace) == 1
        _cmp_trace(r.trace[0], o["trace"])
    assert same_stride >= 1


def _export_readback(rc, kw, kr):
    """The closed form as the reference's export reads it (cvo_export.hip, cvo_align_association): the matrix written
    row-major with stride kw (the iteration's K) and read back with stride kr (the K the update chose for the next
    iteration), each row of nonzero count > 0 up to its first -1 entry."""
    nz, ind, mat = rc.closed_form(kw)
    fj, fa = ind.reshape(-1), mat.reshape(-1)
    rp, cols, vals = [0], [], []
    for i in range(rc.N):
        if nz[i]:
            j, a = fj[i * kr:min((i + 1) * kr, rc.N * kw)], fa[i * kr:min((i + 1) * kr, rc.N * kw)]
            end = np.flatnonzero(j == -1)
            n = end[0] if len(end) else len(j)
            cols.append(j[:n])
            vals.append(a[:n])
        rp.append(rp[-1] + (len(cols[-1]) if nz[i] else 0))
    return (np.array(rp, np.int64), np.concatenate(cols + [np.zeros(0, np.int64)]),
            np.concatenate(vals + [np.zeros(0)]))


@pytest.mark.parametrize("M", [65535, 65536])
def test_16_and_32_bit_candidate_lists(oracle, M):
    """The same clusters padded to M = 65535 (16-bit lists, ASSOC_CAP16 = 64, long lists) and M = 65536 (32-bit lists,
    ASSOC_CAP32 = 32, no long lists): rows of 33 .. 64 candidates go to the literal scan only in the 32-bit case."""
    P = _params()
    rc = rcl.bits_family(P, M)
    gpu = _iteration0(oracle, rc, 512)
    n_ovf, n_scan, _ = gpu.debug_row_classes()
    mid = int(((rc.counts > 32) & (rc.counts <= 64)).sum())
    assert mid > 0
    if M < 65536:
        assert n_scan == int((rc.counts > LONG_CAP).sum()) and n_ovf == int((rc.counts > 64).sum())
    else:
        assert n_scan == n_ovf == int((rc.counts > 32).sum())


def test_32_bit_lists_trajectory_and_verified_lists(oracle, monkeypatch):
    """30 iterations at M = 65536 with overflow rows against the oracle, then the same run with every reused list checked
    against the literal scan on the device (CVO_VERIFY_LISTS=1): bit-identical."""
    P = _params()
    rc = rcl.bits_family(P, 65536)
    src, tgt = rc.clouds()
    _follow_oracle(oracle, P, src, tgt, EYE, 30, "bits_65536")
    a = CvoGPU(params=P).align(src, tgt, EYE, max_iterations=30, trace_capacity=30, trace_dense=30)
    monkeypatch.setenv("CVO_VERIFY_LISTS", "1")
    gpu = CvoGPU(params=P)
    b = gpu.align(src, tgt, EYE, max_iterations=30, trace_capacity=30, trace_dense=30)
    assert gpu.debug_verified_rows() > 0
    assert np.array_equal(a.transform, b.transform) and a.iterations == b.iterations
    for x, y in zip(a.trace, b.trace):
        assert (x.nnz, x.B, x.C, x.D, x.E) == (y.nnz, y.B, y.C, y.D, y.E)


@pytest.mark.parametrize("family", ["list", "list_colour", "overflow", "wide_1100_low", "dense_1216"])
def test_trajectory_through_the_classes(oracle, family):
    """40 iterations on each family, iteration by iteration against the oracle."""
    P = _params(family.endswith("colour"))
    rc = {"list": lambda: rcl.list_family(P), "list_colour": lambda: rcl.list_family(P, colour=True),
          "overflow": lambda: rcl.overflow_family(P), "wide_1100_low": lambda: rcl.wide_family(P, 1100),
          "dense_1216": lambda: rcl.dense_family(P, 1216)}[family]()
    src, tgt = rc.clouds()
    _follow_oracle(oracle, P, src, tgt, EYE, 40, family)


@pytest.mark.parametrize("dk", [-1, 0, 1], ids=["K=cmax-1", "K=cmax", "K=cmax+1"])
def test_scores_at_the_K_limit(oracle, dk):
    """inner_product_gpu, both function_angle modes and inner_product_batch with nearest_neighbors_max = c_max - 1, c_max,
    c_max + 1 (clusters of up to 200 targets span several 64-target tiles).  A row voids k_overlap only with more than K
    pairs: then the list chain evaluates the call; a row of exactly K pairs does not."""
    P0 = _params()
    rc = rcl.score_family(P0)
    cmax = int(rc.counts.max())
    K = cmax + dk
    P = _params()
    P.nearest_neighbors_max = K
    src, tgt = rc.clouds()
    gpu = CvoGPU(params=P)
    ell = rc.ell
    want = rc.inner_product(K)
    ip = gpu.inner_product_gpu(src, tgt, EYE, ell)
    assert ip == pytest.approx(want, rel=1e-6)
    _, chain, _ = gpu.debug_last_score_batch()
    assert (chain > 0) == (cmax > K), (K, chain)
    fa = gpu.function_angle(src, tgt, EYE, ell, is_approximate=True)
    assert fa == pytest.approx(want / (np.sqrt(rc.N) * np.sqrt(rc.M)), rel=1e-6)
    ox, oy = _oracle_clouds(oracle, src, tgt)
    op = oracle.params_from(P)
    fe = gpu.function_angle(src, tgt, EYE, ell, is_approximate=False)
    assert fe == pytest.approx(oracle.function_angle(op, ox, oy, EYE, ell, False), rel=1e-5)
    T2 = EYE.copy()
    T2[0, 3] = 0.01
    b = gpu.inner_product_batch([src, src, src], [tgt, tgt, tgt], [EYE, T2, EYE], ell)
    assert b[0] == b[2] == np.float32(ip)
    assert b[1] == gpu.inner_product_gpu(src, tgt, T2, ell)
    assert b[1] == pytest.approx(oracle.inner_product(op, ox, oy, T2, ell), rel=1e-4)


def test_score_batch_chunks_on_row_tiles():
    """One inner_product_batch / exact function_angle_batch call of 450 jobs of a 10000-row source (157 row tiles each:
    70650 > SB_CHUNK_TILES = 65536, fewer than SB_CHUNK_JOBS = 1024 evaluations) is split into at least two
    k_overlap_table launches, and every value equals the single call's bit for bit."""
    P = _params()
    rc = rcl.build(P, [c for c in (5, 40, 90) for _ in range(20)], n_rows=10000, seed=7)
    src, tgt = rc.clouds()
    gpu = CvoGPU(params=P)
    ds, dt = gpu.upload(src), gpu.upload(tgt)
    n = 450
    Ts = []
    for k in range(n):
        T = EYE.copy()
        T[:3, 3] = (0.0004 * k, -0.0002 * (k % 7), 0.0003 * (k % 5))
        Ts.append(T)
    ip = gpu.inner_product_batch([ds] * n, [dt] * n, Ts, rc.ell)
    assert gpu.debug_last_score_batch()[2] >= 2
    fa = gpu.function_angle_batch([ds] * n, [dt] * n, Ts, rc.ell, is_approximate=False)
    assert gpu.debug_last_score_batch()[2] >= 2
    for k in range(n):
        assert ip[k] == np.float32(gpu.inner_product_gpu(ds, dt, Ts[k], rc.ell)), k
        assert fa[k] == np.float32(gpu.function_angle(ds, dt, Ts[k], rc.ell, is_approximate=False)), k
    assert ip[0] == pytest.approx(rc.inner_product(P.nearest_neighbors_max), rel=1e-6)


@pytest.mark.parametrize("K", [64, 65, 1024, 1025])
@pytest.mark.parametrize("family", ["list", "overflow"])
def test_edge_kernel_matrix(family, K):
    """fill_in_A_mat_gpu on frames under identity 3x4 poses: the closed form at ASSOC_CAP16 / LONG_CAP +-."""
    P = _params(K=K)
    rc = {"list": rcl.list_family, "overflow": rcl.overflow_family}[family](P)
    src, tgt = rc.clouds()
    gpu = CvoGPU(params=P)
    pose = np.hstack([np.eye(3), np.zeros((3, 1))])
    f1, f2 = gpu.transformed(gpu.upload(src), pose), gpu.transformed(gpu.upload(tgt), pose)
    mat, ind, nz, total = gpu.edge_kernel_matrix(f1, f2, rc.ell, K)
    cnz, cind, cmat = rc.closed_form(K)
    valid = np.arange(K)[None, :] < cnz[:, None]
    assert total == int(cnz.sum())
    assert np.array_equal(nz, cnz)
    assert np.array_equal(np.where(valid, ind, -1), cind)
    assert np.allclose(mat, cmat, rtol=TOL_F64, atol=0)
