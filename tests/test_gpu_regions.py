"""The owner type of the library's allocations (Region, cvo_internal.h) on the MI355X: every owner gives its device memory
back, and a region that grows - and therefore moves - under a context changes no result of that context."""
import gc

import numpy as np
import pytest

import bki_cases as bc
import cases
import dfilter_cases as dc
import unified_cvo_amd as u
from unified_cvo_amd import CvoGPU, CvoPointCloud, CvoFrameGPU, disparity_filter_host, synth

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)


def _params():
    P = cases.load_params("geometric_gpu")
    P.multiframe_ell_init, P.multiframe_ell_min, P.multiframe_ell_decay_rate = 0.3, 0.1, 0.7
    P.multiframe_num_neighbors, P.multiframe_max_iters = 64, 3
    P.multiframe_iterations_per_ell, P.multiframe_iterations_per_solve, P.multiframe_min_nonzeros = 3, 8, 300
    return P


def _pair(n, pair_id=0):
    a, b, _ = synth.geometric_pair(n, pair_id)
    return CvoPointCloud.from_xyz(a), CvoPointCloud.from_xyz(b)


def _touch_every_owner():
    """One context through every owner at the smallest shape that reaches it; everything freed, the context closed."""
    g = CvoGPU(params=_params())
    g.set_option("DFILTER_HOST", 0)
    g.set_option("BKI_HOST", 0)
    a, b = _pair(300)
    da, db = g.upload_many([a, b])  # ordered on the device: the ordering's job table
    g.params.is_using_intensity = 1  # geometry-only clouds under the colour kernel: zero slabs; k_overlap: tile spheres
    g.inner_product_gpu(da, db, EYE, 0.5)
    g.params.is_using_intensity = 0
    g.function_angle(da, db, EYE, 0.5, is_approximate=False)  # three evaluations, by arguments: the score workspace
    g.inner_product_batch([da, db, da, db], [db, da, da, db], [EYE] * 4, 0.5)  # four: the score table and its staging
    assert g.debug_last_score_batch()[0] == 4
    g.align_batch([da] * 3, [db] * 3, [EYE] * 3, max_iterations=20)  # arena, control block, status mirrors
    moved = g.transformed(da, np.hstack([np.eye(3), np.full((3, 1), 0.01)]))
    q = g.open_queue(2, 300, 300, max_iterations=20)
    for _ in range(3):
        q.submit(da, db, EYE)
    done = []
    while q.pending():
        done.extend(q.poll(wait=2))
    assert len(done) == 3
    q.close()
    g.disparity_filter(dc.random_map(16, 24, seed=1))  # scratch and pinned staging
    assert g.debug_dfilter_stats()["on_device"]
    cfg = bc.growth()[0]
    m = g.map_open(u.MapConfig(**cfg.kwargs()), initial_voxels=16)
    rng = np.random.default_rng(3)
    xyz, feat, label, origin = bc.frame(rng, rng.uniform(-4, 4, (200, 3)).astype(np.float32), 2)
    m.insert((xyz, feat, label), origin=origin)
    stats = m.debug_stats()
    assert stats["on_device"] == 1 and stats["growths"] >= 1
    m.cloud()
    m.close()
    xs, _, X0 = _sequence2(200)
    mf = [CvoFrameGPU(g, CvoPointCloud.from_xyz(x), X0[f].reshape(3, 4)) for f, x in enumerate(xs)]
    g.align_multiframe(mf, [True, False], [(0, 1)])  # transformed frames, the driver's five transient regions
    for f in mf:
        f._init.free()
        f._transformed.free()
    for c in (da, db, moved):
        c.free()
    orphan = g.open_queue(2, 300, 300, max_iterations=20)  # left open: the context releases its device side
    g.L.cvo_ctx_destroy(g.ctx)  # (the raw C-ABI call: CvoGPU.close would close the queue first)
    g.ctx = None
    orphan.close()
    del g, orphan, mf, m, q
    gc.collect()


def _sequence2(n):
    xyz, gt = synth.scene_sequence(2, n, seed=5)
    return xyz, gt, np.stack([p.reshape(12) for p in gt])


def test_every_owner_returns_its_memory():
    """Free device memory (hipMemGetInfo through a probe context) is exactly where it was after each of three cycles that
    create a context, reach every owner - clouds and their zero slabs and tile spheres, the ordering's job table, score
    workspace / table / staging / results, arena, control block, status mirrors, a queue closed and a queue orphaned, the
    disparity filter's scratch and staging, a map whose table grows, the multi-frame driver's transient regions - and free
    everything.  hipMemGetInfo does not see pinned host memory: the owner type covers pinned and mapped regions by
    construction (one release() for the three kinds), and this test does not observe them."""
    probe = CvoGPU(params=cases.load_params("geometric_gpu"))
    try:
        for _ in range(2):  # (the runtime's own pools and the stream pool come up during the first cycles)
            _touch_every_owner()
        free0 = probe.debug_device_memory()[0]
        for _ in range(3):
            _touch_every_owner()
            assert probe.debug_device_memory()[0] == free0
    finally:
        probe.close()


def _fresh(call):
    g = CvoGPU(params=_params())
    g.set_option("DFILTER_HOST", 0)
    try:
        return call(g)
    finally:
        g.close()


def _same(r, s):
    return r.iterations == s.iterations and np.array_equal(r.transform.view(np.uint32), s.transform.view(np.uint32))


def test_a_region_that_moves_changes_no_result():
    """One context whose regions grow between calls; every output equals, bit for bit, a fresh context's."""
    g = CvoGPU(params=_params())
    g.set_option("DFILTER_HOST", 0)
    try:
        # control block and arena regrow (graphs dropped) between two solves of one pair
        a, b = _pair(300)
        big = [_pair(600, k) for k in range(3)]
        one = lambda c: c.align(a, b, EYE, max_iterations=20)
        three = lambda c: c.align_batch([p[0] for p in big], [p[1] for p in big], [EYE] * 3, max_iterations=20)
        r1, rb, r3 = one(g), three(g), one(g)
        assert r1.iterations > 0
        assert _same(r1, r3)
        assert _same(r1, _fresh(one))
        assert all(_same(x, y) for x, y in zip(rb, _fresh(three)))
        # the score workspace grows from one row tile to five
        s64, s300 = _pair(64), _pair(300, 1)
        ip = lambda pair: (lambda c: np.float32(c.inner_product_gpu(pair[0], pair[1], EYE, 0.5)))
        got = [ip(s64)(g), ip(s300)(g), ip(s64)(g)]
        want = [_fresh(ip(s64)), _fresh(ip(s300)), _fresh(ip(s64))]
        assert got[0] != 0 and got[1] != 0
        assert [v.tobytes() for v in got] == [v.tobytes() for v in want]
        # the disparity filter's scratch and pinned staging grow
        maps = [dc.random_map(16, 24, seed=2), dc.random_map(32, 48, seed=3), dc.random_map(16, 24, seed=2)]
        outs = []
        for d in maps:
            outs.append(g.disparity_filter(d))
            assert g.debug_dfilter_stats()["on_device"]
            assert dc.first_difference(outs[-1], disparity_filter_host(d)) == ""
        assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))
        # the ordering's job table grows from one job to three
        clouds = [_pair(300, k)[0] for k in range(3)]
        for batch in (clouds[:1], clouds):
            many = g.upload_many(batch)
            for pc, d in zip(batch, many):
                single = g.upload(pc)
                assert np.array_equal(d.debug_order(), single.debug_order())
                assert sorted(d.debug_order()) == list(range(300))
                single.free()
                d.free()
    finally:
        g.close()
