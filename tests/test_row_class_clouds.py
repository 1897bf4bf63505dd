"""The row-class clouds of row_classes.py (no GPU): their closed-form association equals the independent float64
reference (np_reference.kernel_matrix, dense, in row chunks) and the oracle's, on every family, and no foreign target
comes near a row.  The GPU tests (test_gpu_row_classes.py) then check the kernels against the same closed form."""
import numpy as np
import pytest

import cases
import np_reference as npr
import row_classes as rcl


def _params(colour=False, K=None):
    P = cases.load_params("intensity_gpu" if colour else "geometric_gpu")
    if K is not None:
        P.nearest_neighbors_max = K
    return P


def _families():
    Pg, Pc = _params(), _params(colour=True)
    fam = [("list", lambda: rcl.list_family(Pg)),
           ("list_colour", lambda: rcl.list_family(Pc, colour=True)),
           ("overflow", lambda: rcl.overflow_family(Pg)),
           ("dense", lambda: rcl.dense_family(Pg)),
           ("score", lambda: rcl.score_family(Pg))]
    fam += [(f"wide_{M}_{'low' if low else 'spread'}", (lambda M=M, low=low: rcl.wide_family(Pg, M, low=low)))
            for M in rcl.WIDE_M for low in (True, False)]
    fam += [(f"bits_{M}", (lambda M=M: rcl.bits_family(Pg, M))) for M in (65535, 65536)]
    return fam


FAMILIES = _families()
FAMILY_IDS = [f[0] for f in FAMILIES]


def _reference_pattern(rc, K, chunk=None):
    """np_reference.kernel_matrix over all N x M pairs, evaluated in row chunks (<= ~1 GB of float64 temporaries)."""
    chunk = chunk or max(1, min(rc.N, (1 << 30) // (8 * 4 * max(rc.M, 1))))
    nz = np.zeros(rc.N, np.uint32)
    ind = np.full((rc.N, K), -1, np.int64)
    mat = np.zeros((rc.N, K), np.float64)
    for a in range(0, rc.N, chunk):
        b = min(rc.N, a + chunk)
        fx = None if rc.fsrc is None else rc.fsrc[a:b]
        A, keep = npr.kernel_matrix(rc.P, rc.src[a:b], rc.tgt, fx, rc.ftgt, None, None, None, None, K, rc.ell)
        nz[a:b] = keep.sum(1)
        for r in range(b - a):
            j = np.flatnonzero(keep[r])
            ind[a + r, :len(j)] = j
            mat[a + r, :len(j)] = A[r, j]
    return nz, ind, mat


@pytest.mark.parametrize("name,make", FAMILIES, ids=FAMILY_IDS)
def test_counts_and_members(name, make):
    """Each row owns exactly its c_i targets, no target belongs to two rows, and the low_rows option puts the big row of
    the wide / dense families on the lowest original indices."""
    rc = make()
    allm = np.concatenate(rc.members)
    assert len(np.unique(allm)) == len(allm) and (allm.size == 0 or allm.max() < rc.M)
    assert all(np.all(np.diff(m) > 0) for m in rc.members)
    if name.startswith("wide") and name.endswith("low") or name == "dense":
        big = int(np.argmax(rc.counts))
        assert np.array_equal(rc.members[big], np.arange(rc.counts[big]))
    if name.startswith("bits"):
        assert rc.M == int(name.split("_")[1])
    if name == "list" or name == "list_colour":
        v, n = np.unique(rc.counts, return_counts=True)
        assert list(v) == list(rcl.LIST_VALUES) and (n == 64).all()


@pytest.mark.parametrize("name,make", FAMILIES, ids=FAMILY_IDS)
def test_no_foreign_target_near_a_row(name, make):
    """Every target outside row i's cluster is at least 2 r_i away (the construction gives more than 3 r_max)."""
    rc = make()
    assert rcl.foreign_distance(rc) >= 2.0


@pytest.mark.parametrize("name,make", FAMILIES, ids=FAMILY_IDS)
def test_closed_form_equals_float64_reference(name, make):
    """Same nonzeros, same columns, values to 1e-12, at a K below, at and above the largest row."""
    rc = make()
    cmax = int(rc.counts.max())
    for K in sorted({1, 6, 65, max(cmax - 1, 1), cmax, cmax + 1}):
        nz, ind, mat = rc.closed_form(K)
        rnz, rind, rmat = _reference_pattern(rc, K)
        assert np.array_equal(nz, rnz), K
        assert np.array_equal(ind, rind), K
        assert np.allclose(mat, rmat, rtol=1e-12, atol=0), K


@pytest.mark.parametrize("name,make", FAMILIES, ids=FAMILY_IDS)
def test_closed_form_equals_oracle(name, make, oracle):
    """The oracle's se_kernel and one oracle iteration (identity pose) give the closed-form pattern; values to 2e-6 (float
    d^2 and exp against float64)."""
    rc = make()
    cmax = int(rc.counts.max())
    P = _params(colour=rc.fsrc is not None, K=max(512, cmax + 1))
    op = oracle.params_from(P)
    src, tgt = rc.clouds()
    ox, oy = oracle.Cloud.from_pointcloud(src), oracle.Cloud.from_pointcloud(tgt)
    for K in sorted({6, 64, 65, cmax, cmax + 1}):
        nz, ind, mat = rc.closed_form(K)
        omat, oind, onz = oracle.se_kernel(op, ox, oy, K, rc.ell)
        assert np.array_equal(onz, nz), K
        assert np.array_equal(np.where(np.arange(K)[None, :] < nz[:, None], oind, -1), ind), K
        assert np.allclose(omat, mat, rtol=2e-6, atol=0), K
    K = min(cmax, P.nearest_neighbors_max)
    o = oracle.iteration(op, ox, oy, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), rc.ell, K, want_ell=True)
    nz, ind, _ = rc.closed_form(K)
    assert np.array_equal(o["nonzeros"], nz)
    assert np.array_equal(np.where(np.arange(K)[None, :] < nz[:, None], o["ind"], -1), ind)
    assert o["trace"].nnz == int(nz.sum())
