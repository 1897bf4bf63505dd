"""The pair arithmetic's gates (geometric type, distance, colour, semantics, a > sp_thres on the product) where they REJECT,
in every instantiation (FEAT_GEO / COL / HOT / ALL) and every kernel family that evaluates pairs: k_assoc (thread per row),
k_assoc_dense (wave per row, wide rows, the dense regime), k_overlap / k_overlap_table, the list chain and k_verify.

a. iteration 0 on the row-class clouds of row_classes.py with a rejecting feature kind: a row's CANDIDATES sit on one limit,
   its HITS on another, so what follows candidates (row class, list capacity, quarters of a wide row) and what follows hits
   (ballot + prefix slots, LDS compaction, first-K) are told apart;
b. the scores on rows of 3 K candidates and K - 1 / K / K + 1 hits: k_overlap must void on hits, not candidates;
c. all 16 settings of (geometry, intensity, semantics, geometric_type) x label kinds with cut-offs moved so that every gate
   rejects (feature_mixes.py), through one iteration, a trajectory prefix and the project's bit-for-bit equalities;
d. the consumers of the matrix: association export, the multi-frame edge matrix, the IRLS normal equations.

Integer work (nonzeros, columns, nnz / max_nnz / K, iteration counts, path counters) is exact against the oracle, which
computes in the same floats; decisions are never compared with float64.  Values are within 2e-7 of the oracle and within
TOL_F64_FEATURED of the float64 closed form.
"""
import numpy as np
import pytest

import cases
import feature_mixes as fm
import np_multiframe as nm
import row_classes as rcl
from test_gpu_parity import _cmp_trace, _prefix, _single_iteration
from test_gpu_row_classes import EYE, LONG_CAP, _export_readback, _iteration0, _oracle_clouds
from test_gpu_speculation import _key, _run
from test_row_class_clouds import ORACLE_F64_DIST
from unified_cvo_amd import CvoGPU, CvoPointCloud

pytestmark = pytest.mark.gpu

# Values against float64.  TOL_F64 = 2e-6 of test_gpu_row_classes.py is derived for ONE factor.  With up to four the bound
# is measured on the reference side only: the oracle is at most ORACLE_F64_DIST = 6.1e-7 (measured 6.027e-7, on
# list-hot_pass) from the closed form over every featured cloud (test_row_class_clouds.py).  The device is within one float
# ulp per exp() of the oracle, less than the oracle's own float error, so it gets twice that distance: 1.22e-6.  A wrong
# factor, slot or column is off by orders of magnitude.
TOL_F64_FEATURED = 2 * ORACLE_F64_DIST
KINDS = rcl.FEATURE_KINDS
Pg = lambda: cases.load_params("geometric_gpu")


# ---- a. iteration 0, every row class x feature kind -----------------------------------------------------------------

# K on the hit counts of LIST_CH (5 6 7 | 15 16 17 | 31 32 33 | 63 and, in the overflow family, 64 65) and OVERFLOW_CH
# (127 128 129 | 255 256 257 | 304 305 | 384 385 | 1023 1024 1025 | 1216)
@pytest.mark.parametrize("family,K", [("list", K) for K in (6, 16, 32, 64)]
                         + [("overflow", K) for K in (6, 64, 128, 256, 304, 512, 1024, 1216)])
@pytest.mark.parametrize("kind", KINDS)
def test_iteration0_hits_and_candidates_on_different_limits(oracle, kind, family, K):
    """k_assoc's LDS-parked entries and list capacity (2 .. 64 candidates, 0 .. 63 hits) and k_assoc_dense's steps, wide
    quarters and long lists (65 .. 2000 candidates: 70 / 6, 300 / 40, 1100 / 70, 1216 with quarters of 303 / 0 / 152 / 5
    hits, every hit count on the limit below its candidate count's), solo, across first-K limits of the HITS; the row
    classes follow the candidates."""
    rc = {"list": rcl.list_family, "overflow": rcl.overflow_family}[family](Pg(), feature=kind)
    _iteration0(oracle, rc, K, tol_f64=TOL_F64_FEATURED)


@pytest.mark.parametrize("K", [304, 512])
@pytest.mark.parametrize("M,low", [(1100, True), (1216, True), (1216, False)], ids=["1100-low", "1216-low", "1216-spread"])
@pytest.mark.parametrize("kind", KINDS)
def test_wide_rows_with_rejected_candidates(oracle, kind, M, low, K):
    """The wide phase of k_assoc_dense on one big row: every quarter compacts fewer hits than it has candidates (three in
    four at M = 1100; at M = 1216 a quarter that keeps all but one, an empty one, a half, a handful), K below and above
    the hits."""
    _iteration0(oracle, rcl.wide_family(Pg(), M, low=low, feature=kind), K, tol_f64=TOL_F64_FEATURED)


@pytest.mark.parametrize("M", [1100, 1216])
@pytest.mark.parametrize("kind", KINDS)
def test_dense_regime_with_rejected_candidates(oracle, kind, M):
    """More than half of the rows overflow ON CANDIDATES (70 candidates, 6 / 33 / 64 / 70 hits; 400 candidates, 40 hits) and
    M <= 2048: the pair enters the dense regime, where every row is evaluated over all M targets; three iterations against
    the oracle, and iteration 0's nonzeros are the hits."""
    rc = rcl.dense_family(Pg(), M, feature=kind)
    P = rc.params(512)
    src, tgt = rc.clouds()
    gpu = CvoGPU(params=P)
    g = gpu.align(src, tgt, EYE, max_iterations=3, trace_capacity=3, trace_dense=3)
    ox, oy = _oracle_clouds(oracle, src, tgt)
    o = oracle.align(oracle.params_from(P), ox, oy, EYE, trace_capacity=3, trace_dense=3, max_iterations=3)
    assert g.iterations == o["iterations"] == 3 and len(g.trace) == len(o["trace"]) == 3
    for a, b in zip(g.trace, o["trace"]):
        _cmp_trace(a, b)
    assert gpu.debug_row_classes()[2]
    assert g.trace[0].nnz == int(rc.counts.sum())
    assert cases.max_abs_diff(g.transform, o["transform"]) <= 1e-6


@pytest.mark.parametrize("M", [65535, 65536])
@pytest.mark.parametrize("kind", KINDS)
def test_16_and_32_bit_lists_with_rejected_candidates(oracle, kind, M):
    """Rows of 20 .. 100 candidates keeping a third (and 1100 keeping 70) at M = 65535 (16-bit lists) / 65536 (32-bit lists,
    rows of 33 .. 64 candidates scanned literally although they have at most 22 hits)."""
    rc = rcl.bits_family(Pg(), M, feature=kind)
    gpu = _iteration0(oracle, rc, 512, tol_f64=TOL_F64_FEATURED)
    n_ovf, n_scan, _ = gpu.debug_row_classes()
    c = rc.cand_counts
    if M < 65536:
        assert n_scan == int((c > LONG_CAP).sum()) and n_ovf == int((c > 64).sum())
    else:
        assert n_scan == n_ovf == int((c > 32).sum()) and (kind == "hot_pass" or n_ovf > int((rc.counts > 32).sum()))


@pytest.mark.parametrize("n_pairs", [4, 8, 17])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_contexts_with_rejected_candidates(oracle, kind, n_pairs):
    """The featured list and overflow families as pairs of one align_batch (as test_batch_contexts), a different shuffle
    and different feature values per pair: every pair's exported association is the closed form's hits, the first four
    pairs' traces the oracle's."""
    rcs = [(rcl.list_family if p % 2 == 0 else rcl.overflow_family)(Pg(), seed=200 + p, feature=kind) for p in range(n_pairs)]
    P = rcs[0].params(512)
    P.is_exporting_association = 1
    clouds = [rc.clouds() for rc in rcs]
    gpu = CvoGPU(params=P)
    res = gpu.align_batch([c[0] for c in clouds], [c[1] for c in clouds], [EYE] * n_pairs, max_iterations=1,
                          trace_capacity=2, trace_dense=2)
    K = P.nearest_neighbors_max
    same_stride = 0
    for p, (rc, (src, tgt), r) in enumerate(zip(rcs, clouds, res)):
        rp, col, val, kw, kr = gpu.align_association(rc.N, pair=p)
        assert kw == K, (p, kw)
        if kw == kr:
            crp, ccol = rc.csr(K)
            assert np.array_equal(rp, crp) and np.array_equal(col, ccol), p
            same_stride += 1
        erp, ecol, eval_ = _export_readback(rc, kw, kr)
        assert np.array_equal(rp, erp) and np.array_equal(col, ecol), (p, kw, kr)
        assert np.allclose(val, eval_, rtol=TOL_F64_FEATURED, atol=0), p
        assert len(r.trace) == 1 and r.trace[0].nnz == int(np.minimum(rc.counts, K).sum()), p
        if p < 4:
            ox, oy = _oracle_clouds(oracle, src, tgt)
            o = oracle.iteration(oracle.params_from(P), ox, oy, EYE[:3, :3], EYE[:3, 3], rc.ell, K)
            _cmp_trace(r.trace[0], o["trace"])
    assert same_stride >= 1


# ---- b. scores with K around the hit counts ---------------------------------------------------------------------------

def _scores(gpu, src, tgt, T, ell):
    return (gpu.inner_product_gpu(src, tgt, T, ell), gpu.function_angle(src, tgt, T, ell, True),
            gpu.function_angle(src, tgt, T, ell, False))


@pytest.mark.parametrize("dh", [-1, 0, 1], ids=["h=K-1", "h=K", "h=K+1"])
@pytest.mark.parametrize("kind", KINDS)
def test_scores_void_on_hits_not_candidates(oracle, kind, dh):
    """Rows of 3 K = 192 candidates with K - 1, K or K + 1 hits: up to K hits the overlap kernel answers alone (no chain
    evaluation, however many candidates the row has), one hit more voids it and the list chain answers.  inner_product_gpu,
    both function_angle modes, inner_product_batch of five evaluations and the forced chain agree with each other as the
    project claims, with the closed form's first K hits and with the oracle."""
    K = 64
    rc = rcl.score_rows(Pg(), K, K + dh, kind)
    hmax = int(rc.counts.max())
    assert int(rc.cand_counts.max()) == 3 * K and hmax == (K + dh if kind != "hot_pass" else 3 * K)
    _iteration0(oracle, rc, K, tol_f64=TOL_F64_FEATURED)  # (the association's first K of the hits on the same rows)
    P = rc.params(K)
    src, tgt = rc.clouds()
    gpu = CvoGPU(params=P)
    ds, dt = gpu.upload(src), gpu.upload(tgt)
    ell = rc.ell
    want = rc.inner_product(K)
    ip = gpu.inner_product_gpu(ds, dt, EYE, ell)
    n_overlap, n_chain, _ = gpu.debug_last_score_batch()
    assert (n_chain > 0) == (hmax > K) and n_overlap >= 1, (K, hmax, n_overlap, n_chain)
    assert ip == pytest.approx(want, rel=1e-6)  # a float sum of values each within TOL_F64_FEATURED
    fa = gpu.function_angle(ds, dt, EYE, ell, is_approximate=True)
    assert fa == pytest.approx(want / (np.sqrt(rc.N) * np.sqrt(rc.M)), rel=1e-6)
    ox, oy = _oracle_clouds(oracle, src, tgt)
    op = oracle.params_from(P)
    assert ip == pytest.approx(oracle.inner_product(op, ox, oy, EYE, ell), rel=1e-4)
    fe = gpu.function_angle(ds, dt, EYE, ell, is_approximate=False)
    assert fe == pytest.approx(oracle.function_angle(op, ox, oy, EYE, ell, False), rel=1e-5)
    Ts = []
    for k in range(5):
        T = EYE.copy()
        T[:3, 3] = (0.004 * k, -0.003 * (k % 2), 0.002 * (k % 3))
        Ts.append(T)
    b = gpu.inner_product_batch([ds] * 5, [dt] * 5, Ts, ell)
    assert b[0] == np.float32(ip)
    for k in range(1, 5):
        assert b[k] == np.float32(gpu.inner_product_gpu(ds, dt, Ts[k], ell)), k
        assert b[k] == pytest.approx(oracle.inner_product(op, ox, oy, Ts[k], ell), rel=1e-4), k
    fast = _scores(gpu, ds, dt, Ts[1], ell)
    gpu.set_option("IP_CHAIN", "1")
    chain = _scores(gpu, ds, dt, Ts[1], ell)
    chain0 = gpu.inner_product_gpu(ds, dt, EYE, ell)
    gpu.set_option("IP_CHAIN", None)
    assert fast == pytest.approx(chain, rel=2e-7, abs=1e-30)
    assert ip == pytest.approx(chain0, rel=2e-7)
    if hmax > K:  # the chain answered both times
        assert ip == chain0


# ---- c. the switch matrix with moved cut-offs ------------------------------------------------------------------------

N_SLAB, N_SCENE, N_IT = 500, 800, 12


class _Bare(CvoPointCloud):
    """Positions only: no colour, label or geometric-type array reaches the upload (CvoPointCloud.from_xyz would still send
    its (1, 0) types), so a call that needs one reads the zero slab the device creates on demand."""

    def device_arrays(self):
        return np.ascontiguousarray(self.positions_, np.float32), None, None, None


def _mix_pair(labels, builder):
    """(GPU clouds, oracle clouds, init): for 'absent' the device gets bare positions and creates its zero slabs, the oracle
    gets explicit zero arrays."""
    d, init = fm.arrays(N_SLAB if builder == "slab" else N_SCENE, labels, builder=builder)
    ref = fm.clouds(d)
    dev = (_Bare.from_xyz(d["x"]), _Bare.from_xyz(d["y"])) if labels == "absent" else ref
    return dev, ref, init


class _Both:
    """An `oracle` for _single_iteration / _prefix that reads the reference clouds where the device was given bare ones."""

    def __init__(self, oracle, dev, ref):
        self._o, self._map = oracle, {id(dev[0]): ref[0], id(dev[1]): ref[1]}
        outer = self

        class Cloud:
            @staticmethod
            def from_pointcloud(pc):
                return oracle.Cloud.from_pointcloud(outer._map.get(id(pc), pc))
        self.Cloud = Cloud

    def __getattr__(self, name):
        return getattr(self._o, name)


@pytest.mark.parametrize("builder,labels", [("slab", l) for l in fm.LABEL_KINDS] + [("scene", "soft"), ("scene", "hot")],
                         ids=lambda v: v)
@pytest.mark.parametrize("mix", fm.MIXES, ids=fm.MIX_IDS)
def test_switch_matrix(oracle, monkeypatch, mix, builder, labels):
    """One setting of the four switches, MOVED cut-offs (every gate rejects: test_oracle_numpy.py asserts the shares), mixed
    geometric types, on a slab and on the clustered scene: one iteration at two (ell, K) states (ELL exact against the
    oracle); a 12-iteration prefix record by record; the same prefix with every reused list verified by k_verify (FEAT_ALL
    whatever the call's instantiation), with one-hot rows evaluated as class rows (NO_ONEHOT; on one-hot inputs the moved
    s_ell makes diff_ok false), as a pair of a batch, through a queue, and untraced (default) against traced - each
    bit-identical to the solo traced run."""
    dev, ref, init = _mix_pair(labels, builder)
    P = fm.params(mix)
    both = _Both(oracle, dev, ref)
    src, tgt = dev
    ell0 = fm.MOVED_STATES[0][0]
    P.ell_init = ell0
    for ell, K in fm.MOVED_STATES:
        o = oracle.iteration(oracle.params_from(P), both.Cloud.from_pointcloud(src), both.Cloud.from_pointcloud(tgt),
                             init[:3, :3], init[:3, 3], ell, K)
        if o["trace"].nnz == 0:  # ('absent' types: 0 / 0 = NaN drops every pair; the prefix below checks ret = -1)
            assert labels == "absent" and mix[3]
            continue
        _single_iteration(both, P, src, tgt, init, ell=ell, K=K)
    gpu = CvoGPU(params=P)
    ds, dt = gpu.upload(src), gpu.upload(tgt)
    g, o = _prefix(both, P, src, tgt, init, N_IT, gpu=gpu)
    for a, b in zip(g.trace, o["trace"]):
        _cmp_trace(a, b)
    assert cases.max_abs_diff(g.transform, o["transform"]) <= 1e-6
    if labels == "absent" and mix[3]:
        assert g.ret == -1 and g.iterations == 0
        return
    traced, _ = _run(gpu, ds, dt, init, "traced", N_IT)
    assert _key(traced) == _key(g)
    default, _ = _run(gpu, ds, dt, init, "default", N_IT)
    assert _key(default) == _key(traced)
    if labels in ("hot", "absent") and mix[2]:
        gpu.set_option("NO_ONEHOT", "1")
        general = gpu.align(ds, dt, init, max_iterations=N_IT, trace_capacity=N_IT, trace_dense=N_IT)
        gpu.set_option("NO_ONEHOT", None)
        assert _key(general) == _key(g)
        for a, b in zip(general.trace, g.trace):
            assert (a.nnz, a.max_nnz, a.B, a.C, a.D, a.E) == (b.nnz, b.max_nnz, b.B, b.C, b.D, b.E)
    init2 = init.copy()
    init2[:3, 3] += np.array([0.02, -0.01, 0.015], np.float32)
    solo2 = gpu.align(ds, dt, init2, max_iterations=N_IT)
    batch = gpu.align_batch([ds, ds, ds], [dt, dt, dt], [init, init2, init], max_iterations=N_IT)
    assert [_key(r) for r in batch] == [_key(traced), _key(solo2), _key(traced)]
    queued = gpu.align_stream([ds, ds], [dt, dt], [init2, init], slots=2, max_iterations=N_IT)
    assert [_key(r) for r in queued] == [_key(solo2), _key(traced)]
    gpu.close()
    monkeypatch.setenv("CVO_VERIFY_LISTS", "1")
    vgpu = CvoGPU(params=P)
    v = vgpu.align(src, tgt, init, max_iterations=N_IT, trace_capacity=N_IT, trace_dense=N_IT)
    assert _key(v) == _key(g)
    for a, b in zip(v.trace, g.trace):
        assert (a.nnz, a.max_nnz, a.B, a.C, a.D, a.E) == (b.nnz, b.max_nnz, b.B, b.C, b.D, b.E)
    if mix[0] and g.iterations == N_IT:
        assert vgpu.debug_verified_rows() > 0
    vgpu.close()


# ---- d. consumers of the matrix --------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_association_export_of_featured_overflow_rows(kind):
    """compute_association_gpu: the CSR of the featured overflow family is the closed form's hits, at K above and inside the
    hit counts."""
    for K in (1216, 300):
        rc = rcl.overflow_family(Pg(), feature=kind)
        gpu = CvoGPU(params=rc.params(K))
        src, tgt = rc.clouds()
        rp, col, val = gpu.compute_association_gpu(src, tgt, EYE, rc.ell)
        crp, ccol = rc.csr(K)
        assert np.array_equal(rp, crp) and np.array_equal(col, ccol), K
        want = np.concatenate([rc.values(i)[:K] for i in range(rc.N)])
        assert np.allclose(val, want, rtol=TOL_F64_FEATURED, atol=0), K
        gpu.close()


@pytest.mark.parametrize("kind", KINDS)
def test_edge_matrix_and_irls_normal_of_featured_overflow_rows(kind):
    """fill_in_A_mat_gpu on frames under identity poses at K = 304 (rows of 6 .. 1216 hits among 65 .. 2000 candidates) is
    the closed form, and k_irls_gather / k_irls_normal over that matrix (K > 64, rows of very different lengths) give
    np_multiframe.edge_normal's cost, gradient and Hessian to 1e-10."""
    K = 304
    rc = rcl.overflow_family(Pg(), feature=kind)
    src, tgt = rc.clouds()
    gpu = CvoGPU(params=rc.params(K))
    d1, d2 = gpu.upload(src), gpu.upload(tgt)
    pose = np.hstack([np.eye(3), np.zeros((3, 1))])
    f1, f2 = gpu.transformed(d1, pose), gpu.transformed(d2, pose)
    mat, ind, nz, total = gpu.edge_kernel_matrix(f1, f2, rc.ell, K)
    cnz, cind, cmat = rc.closed_form(K)
    valid = np.arange(K)[None, :] < cnz[:, None]
    assert total == int(cnz.sum()) and np.array_equal(nz, cnz)
    assert np.array_equal(np.where(valid, ind, -1), cind)
    assert np.allclose(mat, cmat, rtol=TOL_F64_FEATURED, atol=0)
    ang = 0.01
    q1 = np.hstack([np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]]),
                    np.array([[0.01], [-0.02], [0.005]])]).reshape(12)
    q2 = pose.reshape(12)
    cost, g, H = gpu.debug_irls_normal(d1, d2, q1, q2)
    x1, x2 = src.device_arrays()[0], tgt.device_arrays()[0]
    P1, P2, w = nm.edge_entries(mat, ind, x1, x2)
    c_np, g_np, H_np = nm.edge_normal(P1, P2, w, q1, q2)
    assert cost == pytest.approx(c_np, rel=1e-10)
    assert np.max(np.abs(g - g_np)) <= 1e-10 * np.max(np.abs(g_np))
    assert np.max(np.abs(H - H_np)) <= 1e-10 * np.max(np.abs(H_np))
    gpu.close()
