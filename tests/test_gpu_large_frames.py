"""The ordered compactions of the four front ends (voxel grid, RGB-D, FAST, stereo) above 1024 blocks.

All of them scan their per-block counts with compact_scan_counts (cvo_k_compact.h) - RGB-D, FAST and stereo in
k_compact_scan, the voxel grid in its own k_voxel_scan, which sums the insert's statistics in the same launch -: ONE block
of 1024 threads, thread t takes per = ceil(nb / 1024) consecutive counts.  Every entry point accepts 2^24 points or pixels (nb = 16384, per = 16); the
other modules stop at 977 blocks (per = 1).  Here: per = 2, 3 and 16 - threads left without counts, a last working thread
with ONE count, the write-back loop -, k_voxel_insert striding over more than 512 blocks into a table above 2^21 slots,
FULL's column-major enumeration above 2^20 pixels, and the extreme voxel indices +-(2^20 - 1).  The device routes are
forced and seen to have run (debug_*_stats) before a switch is restored.  Every comparison is exact.

The numpy statements are computed once per process (functools.lru_cache) and left unchanged.  Their times on one CPU
core (of a machine without a GPU), the larger part of every test here:
  voxel 2^20, 2^20 + 1, 2^21 + 1025            1.7 s, 1.9 s, 4.0 s (np_voxel.reference), shared by both pre-pass settings
  voxel 2^24                                   4.3 s (np_voxel.reference_packed) + 0.6 s for the draw
  FAST 1040 x 1024, 1025 x 2048, 1031 x 1040   3 s, 7 s, 3 s (select under both schedules + the score histogram), shared by
                                               both FAST_TILE settings
  RGB-D 1025 x 2048                            FULL 0.4 s per depth type, DSO_EDGES 0.6 s, recipe 2.6 s, frames 0.8 s each
  stereo 1025 x 2048                           FULL 0.4 s, CV_FAST 2.5 s, frame 0.7 s
(DSO_EDGES and CV_FAST stay at 1025 x 2048: their statements need well under 10 s there.)

Wall time of each test on an MI355X host (pytest --durations; this module and test_gpu_kd_order.py together: 81 tests
in 18.4 s; that host's CPU is faster than the one above, and the test that meets a statement first pays for it):
  test_voxel_select_across_the_scan_classes    [2^20-1] 0.95 s, [2^20+1-1] 0.85 s, [2^21+1025-1] 2.03 s; the three with
                                               pre-pass 0 (statement shared, the device side alone): under 5 ms each
  test_voxel_select_at_the_bound               2.50 s
  test_extreme_voxel_indices_keep_their_fields under 5 ms
  test_fast_select_above_1024_blocks           [1040-1024-1] 0.88 s, [1025-2048-1] 2.52 s, [1031-1040-1] 1.24 s; the three
                                               with FAST_TILE 0: under 5 ms each
  test_rgbd_full_in_column_major_order         [u16] 0.42 s, [f32] 0.35 s
  test_rgbd_dso_edges_cell_lists               0.17 s
  test_upload_rgbd_of_a_large_frame            0.90 s
  test_stereo_points_of_a_large_frame          [FULL] 0.44 s, [CV_FAST] 0.52 s

What discriminates: with the scan's per cut to max(1, nb / 1024) on a scratch build - the remainder blocks keep their
counts as offsets - the voxel cases at 2^20 + 1 and 2^21 + 1025, FAST at 1040 x 1024 and 1031 x 1040, every RGB-D test
and stereo FULL fail, and every test of test_gpu_voxel / rgbd / fast / stereo.py passes.  Voxel at 2^24 (a multiple of
1024 blocks) and FAST / CV_FAST at 1025 x 2048 do not see that mutation: the frame's last row is its last two blocks,
inside the detector's border, so their counts are 0; these cases run per = 16 and 3 without a remainder that matters."""
import functools

import numpy as np
import pytest

import cases
import np_fast
import np_voxel
import rgbd_cases as rc
import stereo_cases as sc
from test_gpu_fast import _check as fast_check
from unified_cvo_amd import CvoGPU, CvoPointCloud, RGBDFrame, StereoFrame, synth
from unified_cvo_amd.api import CV_FAST, DSO_EDGES, FULL

pytestmark = pytest.mark.gpu

THREADS = 1024          # points / pixels / cells per block of every compaction, and threads of the one scanning block
ROWS, COLS = 1025, 2048  # 2 099 200 pixels: 2050 blocks, per = 3, the last working thread (683) holds ONE count


def _blocks(n):
    return (n + THREADS - 1) // THREADS


def _per(nb):
    return (nb + THREADS - 1) // THREADS


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    yield g
    g.close()


# ---------------------------------------------------------------------------------------------------------------
# voxel grid
# ---------------------------------------------------------------------------------------------------------------
VOXEL_LEAF = 0.25
VOXEL_SIZES = {2 ** 20: (1024, 1), 2 ** 20 + 1: (1025, 2), 2 ** 21 + 1025: (2050, 3), 2 ** 24: (16384, 16)}  # n -> (nb, per)


def _voxel_draw(n, reference):
    """n uniform float32 points in a 4 : 1 : 4 box holding n / 1.6 voxels of side 0.25: with 1.6 points per voxel on
    average (Poisson) a grid keeps (1 - exp(-1.6)) / 1.6 = 50 % of them.  Returns the points and reference's selection."""
    side = (n / 1.6 / 16.0) ** (1.0 / 3.0) * VOXEL_LEAF
    rs = np.random.default_rng(770 + n % 1000)
    x = rs.random((n, 3), dtype=np.float32) * np.array([4 * side, side, 4 * side], np.float32) - np.array([2 * side, side / 2, 0], np.float32)
    want = reference(x, VOXEL_LEAF)
    assert 0.3 * n <= len(want) <= 0.9 * n, (n, len(want))
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


@functools.lru_cache(maxsize=None)
def _voxel_draw_shared(n):
    """The draw both pre-pass settings of one size share, against np_voxel.reference."""
    return _voxel_draw(n, np_voxel.reference)


def _voxel_check(gpu, n, prepass, x, want):
    nb, per = VOXEL_SIZES[n]
    assert (_blocks(n), _per(nb)) == (nb, per) and len(x) == n
    gpu.set_option("VOXEL_PREPASS", prepass)
    gpu.set_option("VOXEL_HOST", 0)
    try:
        kept = gpu.voxel_select(x, VOXEL_LEAF)
        st = gpu.debug_voxel_stats()
        assert st["capacity"] >= 2 * n and st["capacity"] & (st["capacity"] - 1) == 0, st     # the kernels ran
    finally:
        gpu.set_option("VOXEL_PREPASS", None)
        gpu.set_option("VOXEL_HOST", None)
    assert kept.dtype == np.int32 and len(kept) == len(want), (len(kept), len(want))
    assert np.array_equal(kept, want)
    assert st["occupied"] == len(kept), st
    assert len(kept) <= st["entered"] <= n and st["probes_total"] >= st["entered"], st
    if prepass == 0:
        assert st["entered"] == n, st
    assert st["probe_longest"] > 1, st
    if n > 2 ** 20:
        assert st["capacity"] > 2 ** 21      # (and k_voxel_insert's 512 blocks each took more than one trip)


@pytest.mark.parametrize("prepass", [1, 0])
@pytest.mark.parametrize("n", [2 ** 20, 2 ** 20 + 1, 2 ** 21 + 1025])
def test_voxel_select_across_the_scan_classes(gpu, n, prepass):
    """1024 blocks: the last size with one count per thread.  1025: two per thread, 511 threads idle.  2050: three per
    thread, thread 683 holds the one count that is left, 340 threads idle."""
    _voxel_check(gpu, n, prepass, *_voxel_draw_shared(n))


def test_voxel_select_at_the_bound(gpu):
    """2^24 points, the most cvo_voxel_select accepts: 16384 counts, 16 per thread, a table of 2^25 slots.  Against
    np_voxel.reference_packed; the 192 MB draw is used once and not kept."""
    _voxel_check(gpu, 2 ** 24, None, *_voxel_draw(2 ** 24, np_voxel.reference_packed))


def test_extreme_voxel_indices_keep_their_fields(gpu):
    """|k| = 2^20 - 1 and 2^20 - 2 on each axis (the others 0), leaf 0.25 (exact): three 21-bit fields of one key, each at
    its largest and smallest value.  With every extreme point a companion that a field leaking one bit into its neighbour
    would put into the same voxel (k - 2^20 on that axis, +1 on the next).  All in a 5000-point scene."""
    big = 2 ** 20
    extreme, companion = [], []
    for axis in range(3):
        for k in (big - 1, -(big - 1), big - 2, -(big - 2)):
            p = np.zeros(3)
            p[axis] = k * VOXEL_LEAF
            extreme.append(p)
            q = np.zeros(3)
            q[axis] = (k - big if k > 0 else k + big) * VOXEL_LEAF
            q[(axis + 1) % 3] = VOXEL_LEAF
            companion.append(q)
    x = np_voxel.scene(5000).copy()
    at = np.arange(12) * 397 + 101
    x[at] = np.array(extreme, np.float32)
    x[at + 50] = np.array(companion, np.float32)
    keys = np_voxel.voxel_keys(x, VOXEL_LEAF)
    assert np.abs(keys[at]).max() == big - 1 and len(np.unique(keys[at], axis=0)) == 12
    want = np_voxel.reference(x, VOXEL_LEAF)
    assert np.isin(at, want).all()
    for prepass in (1, 0):
        gpu.set_option("VOXEL_PREPASS", prepass)
        gpu.set_option("VOXEL_HOST", 0)
        try:
            kept = gpu.voxel_select(x, VOXEL_LEAF)
            st = gpu.debug_voxel_stats()
            assert st["capacity"] >= 2 * len(x) and st["occupied"] == len(want), st
        finally:
            gpu.set_option("VOXEL_PREPASS", None)
            gpu.set_option("VOXEL_HOST", None)
        assert np.array_equal(kept, want) and np.isin(at, kept).all(), prepass


# ---------------------------------------------------------------------------------------------------------------
# FAST
# ---------------------------------------------------------------------------------------------------------------
FAST_FRAMES = ((1040, 1024), (1025, 2048), (1031, 1040))   # 1040 blocks (per 2), 2050 (per 3), 1048 with cols % 64 != 0


@functools.lru_cache(maxsize=None)
def _fast_statement(rows, cols):
    img = sc.noisy_plane(rows, cols, seed=rows + cols)
    img.setflags(write=False)
    return img, {s: np_fast.select(img, s) for s in (np_fast.STEREO, sc.steer(0))}, np_fast.histogram(np_fast.score(img))


@pytest.mark.parametrize("tile", [1, 0])
@pytest.mark.parametrize("rows,cols", FAST_FRAMES)
def test_fast_select_above_1024_blocks(gpu, rows, cols, tile):
    """test_gpu_fast.py's _check (selection, schedule record, 257-bin histogram) on frames whose compaction has 1040, 2050
    and 1048 blocks; the statement is shared by both FAST_TILE settings."""
    assert _blocks(rows * cols) > THREADS and (cols % 64 != 0) == (cols == 1040)
    img, selections, hist = _fast_statement(rows, cols)
    gpu.set_option("STEREO_HOST", 0)
    gpu.set_option("FAST_TILE", tile)
    try:
        for sched, selection in selections.items():
            fast_check(gpu, img, sched, (rows, cols, sched, tile), (selection, hist))   # (asserts on_device itself)
    finally:
        gpu.set_option("FAST_TILE", None)
        gpu.set_option("STEREO_HOST", None)


# ---------------------------------------------------------------------------------------------------------------
# RGB-D
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rgbd_frame(depth):
    return RGBDFrame(**synth.rgbd_frame(kind="textured", rows=ROWS, cols=COLS, depth=depth))


@functools.lru_cache(maxsize=None)
def _rgbd_statement(depth, method):
    return rc.statement_points(_rgbd_frame(depth), method)


def _dso_cell_blocks(rows, cols):
    """Blocks of the selector's compaction: the cells of the six potentials 2 .. 7 (16 per 4 pot x 4 pot pixels), each
    list padded to whole blocks."""
    return sum(_blocks(-(-cols // (4 * pot)) * -(-rows // (4 * pot)) * 16) for pot in range(2, 8))


@pytest.mark.parametrize("depth", rc.DEPTHS)
def test_rgbd_full_in_column_major_order(gpu, depth):
    """FULL: every pixel with a depth in the order (i % h) * w + i / h, 2050 blocks."""
    f = _rgbd_frame(depth)
    assert _per(_blocks(f.rows * f.cols)) == 3
    want = _rgbd_statement(depth, FULL)
    assert len(want["pixel"]) > 2 ** 20
    gpu.set_option("RGBD_HOST", 0)
    try:
        got = gpu.rgbd_points(f, FULL)
        st = gpu.debug_rgbd_stats()
        assert st["on_device"]
    finally:
        gpu.set_option("RGBD_HOST", None)
    rc.assert_points_equal(got, want, ("FULL", depth))
    assert st["surface_points"] == len(want["pixel"]) and st["with_depth"] == want["with_depth"], st


def test_rgbd_dso_edges_cell_lists(gpu):
    """DSO_EDGES at 1025 x 2048: the six cell lists take 516 + 230 + 130 + 84 + 58 + 43 = 1061 blocks."""
    assert _dso_cell_blocks(ROWS, COLS) == 1061
    f = _rgbd_frame("u16")
    want = _rgbd_statement("u16", DSO_EDGES)
    gpu.set_option("RGBD_HOST", 0)
    try:
        got = gpu.rgbd_points(f, DSO_EDGES)
        st = gpu.debug_rgbd_stats()
        assert st["on_device"]
    finally:
        gpu.set_option("RGBD_HOST", None)
    rc.assert_points_equal(got, want, "DSO_EDGES")
    tried, counts = want["schedule"]
    assert st["potentials"] == tried and st["counts"] == counts, st
    assert st["edge_selected"] == counts[-1] and st["edge_points"] == len(want["pixel"])


def test_upload_rgbd_of_a_large_frame(gpu):
    """The per-frame recipe: selector (1061 blocks), FULL (2050), two voxel selections (31 and 1924 blocks)."""
    f = _rgbd_frame("f32")
    r = rc.statement_recipe(f, 0.1)
    gpu.set_option("RGBD_HOST", 0)
    try:
        d = gpu.upload_rgbd(f, 0.1)
        st = gpu.debug_rgbd_stats()
        assert st["on_device"]
    finally:
        gpu.set_option("RGBD_HOST", None)
    assert d.n == len(r["pixel"]) and np.array_equal(d.pixel, r["pixel"])
    assert np.array_equal(d.is_edge, r["is_edge"].astype(bool))
    assert st["with_depth"] == r["stats"]["with_depth"] and _blocks(st["surface_points"]) > THREADS
    assert st["edge_points"] == r["stats"]["edge"]["candidates"] and st["surface_points"] == r["stats"]["surface"]["candidates"]
    assert st["potentials"] == r["stats"]["edge"]["schedule"][0] and st["counts"] == r["stats"]["edge"]["schedule"][1]
    u = gpu.upload(CvoPointCloud.from_arrays(r["xyz"], r["feat"], None, r["geotype"]))
    assert np.array_equal(d.debug_order(), u.debug_order())
    d.free()
    u.free()


# ---------------------------------------------------------------------------------------------------------------
# stereo
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stereo_frame():
    return StereoFrame(**synth.stereo_frame(kind="textured", rows=ROWS, cols=COLS))   # (the NaN disparities stay in)


@functools.lru_cache(maxsize=None)
def _stereo_statement(method):
    return sc.points_of(_stereo_frame(), method)


@pytest.mark.parametrize("method", [FULL, CV_FAST], ids=["FULL", "CV_FAST"])
def test_stereo_points_of_a_large_frame(gpu, method):
    """FULL: 2 099 200 candidates in column-major order, 2050 blocks; CV_FAST: the detector's compaction over the 2050
    blocks of the frame, then its keypoints'."""
    f = _stereo_frame()
    want = _stereo_statement(method)
    assert np.isnan(f.disparity).any()
    if method == FULL:
        assert want["candidates"] == ROWS * COLS and len(want["pixel"]) > 2 ** 20
    gpu.set_option("STEREO_HOST", 0)
    try:
        got = gpu.stereo_points(f, method)
        st = gpu.debug_stereo_stats()
        assert st["on_device"]
    finally:
        gpu.set_option("STEREO_HOST", None)
    sc.assert_points_equal(got, want, method)
    assert st["candidates"] == want["candidates"] and st["kept"] == len(want["pixel"]), st
    if method == CV_FAST:
        tried, counts, used = want["schedule"]
        assert st["tried"] == tried and st["counts"] == counts and st["threshold_used"] == used, st
