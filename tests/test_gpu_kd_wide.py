"""The multi-block ordering of clouds above 16384 points (ORDER=wide: cvo_k_kd_wide.h, finish_uploads) on the MI355X.

Three opinions on every ordering, as in test_gpu_kd_order.py: the ORDER=wide context, the host twin (ORDER=virtual) and the
numpy statement np_kd.order.  They agree on the point SET of every leaf - every aligned run of 4 sorted positions; the order
inside a leaf is free but the same on every call.  cvo_debug_cloud_order_route says who ordered a cloud: without it a silent
fall-back to the host twin would pass every leaf-set comparison.  Every comparison is exact: integer arrays, leaf sets,
float32 bit patterns."""
import threading

import numpy as np
import pytest

import cases
import np_kd
from test_gpu_ingest import Placed, bits, device_cloud, host_cloud
from test_gpu_kd_order import _gather_case
from unified_cvo_amd import CvoGPU, CvoPointCloud, synth

pytestmark = pytest.mark.gpu

SIZES = (16385, 16896, 20000, 32768, 32769, 33281, 65535, 65536, 65537, 70001, 131073, 262145)
EYE = np.eye(4, dtype=np.float32)
ELL = 0.3
HOST, BLOCK, WIDE = 0, 1, 2


def _context(order=None, params=None, **options):
    g = CvoGPU(params=params) if params is not None else CvoGPU()
    if order:
        g.set_option("ORDER", order)
    for k, v in options.items():
        g.set_option(k, v)
    return g


@pytest.fixture(scope="module")
def contexts():
    """(ORDER=wide, its host twin ORDER=virtual, a default context, ORDER=host)"""
    gs = _context("wide"), _context("virtual"), _context(), _context("host")
    yield gs
    for g in gs:
        g.close()


def _order_and_route(g, pc):
    c = g.upload(pc)
    try:
        return c.debug_order(), c.debug_order_route()
    finally:
        c.free()


def _three_opinions(contexts, x, name):
    w, v = contexts[:2]
    n = x.shape[0]
    pc = CvoPointCloud.from_xyz(x)
    (ow, route), (ov, route_v) = _order_and_route(w, pc), _order_and_route(v, pc)
    assert (route, route_v) == (WIDE, HOST), name
    assert np.array_equal(np.sort(ow), np.arange(n)), name
    assert np.array_equal(np.sort(ov), np.arange(n)), name
    want = np_kd.leaf_sets(np_kd.order(x))
    assert np.array_equal(np_kd.leaf_sets(ov), want), (name, "host twin against the statement")
    differ = int((np_kd.leaf_sets(ow) != want).any(axis=1).sum())
    assert differ == 0, (name, "wide against the statement", f"{differ} of {len(want)} leaves differ")
    assert np.array_equal(_order_and_route(w, pc)[0], ow), (name, "the same rows, another call")


@pytest.mark.parametrize("n", SIZES)
def test_every_size_class(contexts, n):
    """Five global levels at 16385 with leaves of 1024 (one with leaves of 16384) and one more from 32769 / 65537 / 131073 on,
    whatever the leaf; ids beyond 16 bits from 65537; tiles that end off the 2048 grid at every size but the powers of two."""
    _three_opinions(contexts, synth.geometric_pair(n, 7)[0], n)


@pytest.mark.parametrize("n", [20000, 40000])
@pytest.mark.parametrize("kind", list(np_kd.DEGENERATE))
def test_degenerate_clouds(contexts, kind, n):
    """Ties on the global cuts: `identical` puts every pivot among equals (the whole segment is one key: the prefix count alone
    decides), `lattice` a few hundred equals on every cut, the signed zeros - one key to kd_ordered - fall on the first cut
    (level 1) and on the second (level 2; at 40000 points 20480 | 19520, a global cut at every leaf capacity)."""
    _three_opinions(contexts, np_kd.DEGENERATE[kind](n), (kind, n))


def test_routing_edges(contexts):
    w, _, d, h = contexts
    x = {n: synth.geometric_pair(n, 7)[0] for n in (7, 16384, 20000)}
    ow, route = _order_and_route(w, CvoPointCloud.from_xyz(x[16384]))
    assert route == BLOCK and np.array_equal(ow, _order_and_route(d, CvoPointCloud.from_xyz(x[16384]))[0])
    ow, route = _order_and_route(w, CvoPointCloud.from_xyz(x[7]))
    assert route == HOST and np.array_equal(ow, np.arange(7))
    bad = x[20000].copy()
    bad[11717, 1] = np.nan
    ow, route = _order_and_route(w, CvoPointCloud.from_xyz(bad))
    assert route == HOST and np.array_equal(ow, np.arange(20000))
    g = _context("wide", NO_SORT=1)
    try:
        ow, route = _order_and_route(g, CvoPointCloud.from_xyz(x[20000]))
        assert route == HOST and np.array_equal(ow, np.arange(20000))
    finally:
        g.close()
    od, route = _order_and_route(d, CvoPointCloud.from_xyz(x[20000]))
    assert route == HOST and np.array_equal(od, _order_and_route(h, CvoPointCloud.from_xyz(x[20000]))[0])
    assert not np.array_equal(od, np.arange(20000))


def _mixed_clouds():
    rs = np.random.default_rng(33)
    geo = lambda n: np.where(rs.random((n, 1)) < 0.5, [[1.0, 0.0]], [[0.3, 0.9]]).astype(np.float32)
    soft = lambda x: (0.9 * synth.checkerboard_labels(x) + 0.1 / synth.NUM_CLASSES).astype(np.float32)
    colour = lambda x: synth.colour_features(x, rs).astype(np.float32)
    xyz = {n: synth.geometric_pair(n, 40 + k)[0] for k, n in enumerate((700, 16384, 16385, 40000, 5, 20000))}
    xyz[20000] = xyz[20000].copy()
    xyz[20000][9, 2] = np.nan
    return [
        ("colour700", BLOCK, CvoPointCloud.from_arrays(xyz[700], colour(xyz[700]), None, geo(700))),
        ("onehot16384", BLOCK, CvoPointCloud.from_arrays(xyz[16384], None, synth.checkerboard_labels(xyz[16384]), geo(16384))),
        ("soft16385", WIDE, CvoPointCloud.from_arrays(xyz[16385], colour(xyz[16385]), soft(xyz[16385]), geo(16385))),
        ("onehot40000", WIDE, CvoPointCloud.from_arrays(xyz[40000], colour(xyz[40000]), synth.checkerboard_labels(xyz[40000]), None)),
        ("bare5", HOST, CvoPointCloud.from_xyz(xyz[5])),
        ("nan20000", HOST, CvoPointCloud.from_arrays(xyz[20000], colour(xyz[20000]), None, geo(20000))),
    ]


@pytest.fixture(scope="module")
def mixed(contexts):
    """(the clouds, the order of a single upload of each under ORDER=wide): computed once."""
    clouds = _mixed_clouds()
    return clouds, [_order_and_route(contexts[0], pc)[0] for _, _, pc in clouds]


@pytest.mark.parametrize("threads", [1, 4])
def test_one_call_over_mixed_clouds(contexts, mixed, threads):
    """upload_many: one k_kd_order launch over the small clouds, the two wide clouds one after another on the same stream
    with tables of their own in one region, one synchronisation; twice, with the same arrays."""
    w = contexts[0]
    clouds, single = mixed
    seen = []
    for _ in range(2):
        many = w.upload_many([pc for _, _, pc in clouds], threads=threads)
        try:
            assert [m.debug_order_route() for m in many] == [route for _, route, _ in clouds]
            seen.append([m.debug_order() for m in many])
        finally:
            for m in many:
                m.free()
    for (name, route, pc), o1, o2, one in zip(clouds, seen[0], seen[1], single):
        assert np.array_equal(o1, one) and np.array_equal(o2, one), name
        if route == HOST:
            assert np.array_equal(o1, np.arange(len(o1))), name
        else:
            assert np.array_equal(np_kd.leaf_sets(o1), np_kd.leaf_sets(np_kd.order(pc.positions()))), name


@pytest.mark.parametrize("n", [16385, 40000])
@pytest.mark.parametrize("kind", ["colour", "soft", "onehot", "geotype"])
def test_attribute_gathers(kind, n):
    """k_cloud_gather behind the wide ordering: <source, target> at the identity is one bit pattern whoever ordered the
    clouds - a row gathered from the wrong point changes it.  (1, 0, 1): no row reached K, so no truncation lets the order in.
    (The value itself is held against float64 up to 16384 points by test_gpu_kd_order.py.)"""
    P, a, b = _gather_case(kind, n)
    values = {}
    for key, opts in (("wide", {"ORDER": "wide"}), ("default", {}), ("host", {"ORDER": "host"}), ("no-sort", {"NO_SORT": 1})):
        g = _context(params=P, **opts)
        try:
            da, db = g.upload(a), g.upload(b)
            assert da.debug_order_route() == db.debug_order_route() == (WIDE if key == "wide" else HOST), key
            values[key] = np.float32(g.inner_product_gpu(da, db, EYE, ELL))
            assert g.debug_last_score_batch() == (1, 0, 1), key
        finally:
            g.close()
    print(f"{kind} n={n}: " + ", ".join(f"{k} {float(v)!r}" for k, v in values.items()))
    assert values["wide"] > 0
    for k, v in values.items():
        assert bits(v) == bits(values["wide"]), (k, float(v), float(values["wide"]))


@pytest.mark.parametrize("n", [16385, 100000])
def test_from_the_device(contexts, n):
    """cvo_cloud_from_device under ORDER=wide: the ingest's x4 is ordered where it lies (route 2: no coordinate comes down, no
    order goes up), the cloud is the one cvo_cloud_upload makes of the same rows, and scores as a default context's does."""
    w, _, d, _ = contexts
    x = synth.geometric_pair(n, 9)[0]
    rs = np.random.default_rng(n)
    arrs = (x, synth.colour_features(x, rs).astype(np.float32), synth.checkerboard_labels(x).astype(np.float32), None)
    tgt_x = (x[:4096] + np.float32(0.01)).astype(np.float32)        # (overlaps the source: the score is not a bare zero)
    values = {}
    for name, g in (("wide", w), ("default", d)):
        g.write_params(cases.load_params("geometric_gpu"))
        h, dev, tgt = host_cloud(g, *arrs), device_cloud(g, *arrs), host_cloud(g, tgt_x)
        try:
            want = WIDE if name == "wide" else HOST
            assert (h.debug_order_route(), dev.debug_order_route()) == (want, want), name
            assert np.array_equal(dev.debug_order(), h.debug_order()), name
            values[name] = [bits(g.inner_product_gpu(c, tgt, EYE, ELL)) for c in (h, dev)]
            assert values[name][0].view(np.float32) > 0
        finally:
            for c in (h, dev, tgt):
                c.free()
    assert values["wide"][0] == values["wide"][1] == values["default"][0] == values["default"][1], values


def test_from_the_device_through_duplicate_rows(contexts):
    w = contexts[0]
    records = synth.geometric_pair(12000, 9)[0]
    rows = np.random.default_rng(5).integers(0, 12000, 20000).astype(np.int32)
    assert len(np.unique(rows)) < 12000                                # duplicates: equal points, ties on every axis
    with Placed(w) as p:
        dev = w.upload_device(p.rows(records), rows=(p.put(rows), len(rows)), n_records=len(records))
    h = host_cloud(w, records[rows])
    try:
        assert (dev.debug_order_route(), h.debug_order_route()) == (WIDE, WIDE)
        assert np.array_equal(dev.debug_order(), h.debug_order())
        assert np.array_equal(np_kd.leaf_sets(h.debug_order()), np_kd.leaf_sets(np_kd.order(records[rows])))
    finally:
        dev.free()
        h.free()


def test_one_solve(contexts):
    """No result depends on the ordering: a 20000 x 20000 solve under ORDER=wide is the default context's, bit for bit."""
    src, tgt, _ = synth.geometric_pair(20000, 3)
    a, b = CvoPointCloud.from_xyz(src), CvoPointCloud.from_xyz(tgt)
    init = synth.warm_start_delta().astype(np.float32)
    got = {}
    for name, g in (("wide", contexts[0]), ("default", contexts[2])):
        g.write_params(cases.load_params("geometric_gpu"))
        da, db = g.upload(a), g.upload(b)
        try:
            assert da.debug_order_route() == (WIDE if name == "wide" else HOST)
            r = g.align(da, db, init, max_iterations=50)
            got[name] = (r.iterations, r.transform.tobytes())
        finally:
            da.free()
            db.free()
    assert got["wide"][0] > 0 and got["wide"] == got["default"], (got["wide"][0], got["default"][0])


def test_two_threads_one_context(contexts):
    w = contexts[0]
    pcs = [CvoPointCloud.from_xyz(synth.geometric_pair(40000, 60 + k)[0]) for k in range(2)]
    serial = [_order_and_route(w, pc)[0] for pc in pcs]
    out, errors = [None, None], []

    def work(k):
        try:
            out[k] = _order_and_route(w, pcs[k])
        except Exception as e:  # noqa: BLE001 (reported below, on the test's thread)
            errors.append(e)

    ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for k in range(2):
        assert out[k][1] == WIDE and np.array_equal(out[k][0], serial[k]), k
