"""CV_FAST selection on the MI355X: the kernels of cvo_k_fast.h (STEREO_HOST=0) against the numpy statement np_fast.py -
hand-made rings, widths and heights that leave partial blocks and waves, the schedule's debug record, the 257 counts.
Every comparison is exact."""
import os

import numpy as np
import pytest

import cases
import np_fast
import stereo_cases as sc
from unified_cvo_amd import CvoGPU, CvoError

pytestmark = pytest.mark.gpu

HANDMADE = sc.handmade()


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    g.set_option("STEREO_HOST", 0)
    yield g
    g.close()


def _check(gpu, img, sched, name, statement=None):
    """The device's selection, schedule record and histogram against the statement's.  statement: (np_fast.select(img,
    sched), the score histogram), when the caller has them (test_gpu_large_frames.py shares them between settings)."""
    (pix, used, tried, counts), hist = statement or (np_fast.select(img, sched), np_fast.histogram(np_fast.score(img)))
    got, got_used = gpu.fast_select(img, sched)
    st = gpu.debug_stereo_stats()
    assert st["on_device"], name
    assert np.array_equal(got, pix) and got_used == used, name
    assert st["tried"] == tried and st["counts"] == counts and st["threshold_used"] == used, (name, st["tried"], tried)
    assert np.array_equal(st["histogram"], hist), name
    assert st["candidates"] == st["kept"] == len(pix), name


@pytest.mark.parametrize("tile", [1, 0])
def test_handmade_rings(gpu, tile):
    gpu.set_option("FAST_TILE", tile)
    try:
        for name, (img, thresholds) in HANDMADE.items():
            for t in thresholds:
                _check(gpu, img, sc.steer(t), (name, t, tile))
                assert np.array_equal(gpu.fast_select(img, sc.steer(t))[0], np_fast.keypoints(img, t)), (name, t)
    finally:
        gpu.set_option("FAST_TILE", None)


@pytest.mark.parametrize("tile", [1, 0])
@pytest.mark.parametrize("rows,cols", [(7, 7), (7, 63), (7, 64), (7, 65), (7, 257), (7, 1241), (9, 63), (21, 65), (30, 257), (376, 65), (376, 1241)])
def test_partial_blocks_and_waves(gpu, rows, cols, tile):
    """Blocks cover 64 x 16 pixels: widths around one and several blocks, heights of 7 (every keypoint sits on the interior's
    only row), 21 and 30 (a partial second block row) and 376."""
    g = sc.noisy_plane(rows, cols, seed=rows + cols)
    gpu.set_option("FAST_TILE", tile)
    try:
        for sched in ((4, 10 ** 9, 0, 50), np_fast.STEREO, sc.steer(0), sc.steer(12)):
            _check(gpu, g, sched, (rows, cols, sched, tile))
    finally:
        gpu.set_option("FAST_TILE", None)


def test_schedule_record_on_every_branch(gpu):
    g = sc.noisy_plane(64, 96, seed=1)
    c = np_fast.counts_from_histogram(np_fast.histogram(np_fast.score(g)))
    for sched in ((9, 10 ** 9, 0, 13), (4, c[5] - 1, 0, 50), (9, 10 ** 9, c[4], 13), (4, c[5] - 1, c[5] - 1, 50), (4, 0, 0, 7), (2, 10 ** 9, 10 ** 9, 50)):
        _check(gpu, g, sched, sched)


def test_every_interior_pixel_a_corner_and_none(gpu):
    """tests/golden/fast_all_corners.npy: a 10 x 72 image (two blocks wide) found by a local search, in
    which every one of the 4 x 66 interior pixels is a corner at t = 0; and a constant plane, which has none."""
    none = np.full((40, 130), 77, np.uint8)
    assert np_fast.counts_from_histogram(np_fast.histogram(np_fast.score(none)))[0] == 0
    _check(gpu, none, np_fast.STEREO, "none")
    assert len(gpu.fast_select(none, np_fast.STEREO)[0]) == 0
    every = np.load(os.path.join(cases.ROOT, "tests", "golden", "fast_all_corners.npy"))
    rows, cols = every.shape
    assert cols > 64 and np.all(np_fast.score(every)[3:-3, 3:-3] > 0)
    _check(gpu, every, sc.steer(0), "every")
    got = gpu.fast_select(every, sc.steer(0))[0]
    v, u = np.meshgrid(np.arange(3, rows - 3), np.arange(3, cols - 3), indexing="ij")
    assert np.array_equal(got, (v * cols + u).reshape(-1))


def test_repeats_and_refusals(gpu):
    g = sc.noisy_plane(120, 300, seed=3)
    first = gpu.fast_select(g, np_fast.RGBD)
    for _ in range(10):
        again = gpu.fast_select(g, np_fast.RGBD)
        assert np.array_equal(again[0], first[0]) and again[1] == first[1]
    with pytest.raises(CvoError, match="schedule"):
        gpu.fast_select(g, (4, 10, 11, 50))
    with pytest.raises(CvoError, match="schedule"):
        gpu.fast_select(g, (-1, 10, 5, 50))
    assert np.array_equal(gpu.fast_select(g, np_fast.RGBD)[0], first[0])
