"""CV_FAST selection, CPU twin (cvo_fast_select_host) against the numpy statement np_fast.py: the detector on hand-made rings,
the score histogram against the per-threshold definition, every branch of the threshold schedule.  Exact.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import np_fast
import stereo_cases as sc
from unified_cvo_amd import CvoError, _capi, fast_select_host, synth

HANDMADE = sc.handmade()
BIG = 10 ** 9


def test_score_histogram_gives_the_count_at_every_threshold():
    """The two statements agree: the suffix sums of the 257-bin histogram of s equal the direct keypoint count at all 256
    thresholds, and s(p) > t is the direct decision pixel by pixel."""
    g = sc.noisy_plane(48, 64)
    s = np_fast.score(g)
    assert s.min() == -1 and np.all(s[:3] == -1) and np.all(s[:, -3:] == -1) and s.max() > 20
    counts = np_fast.counts_from_histogram(np_fast.histogram(s))
    assert np_fast.histogram(s).sum() == g.size and counts[0] > 1000 and counts[255] == 0
    for t in range(256):
        direct = np_fast.corners(g, t)
        assert counts[t] == np.count_nonzero(direct), t
        assert np.array_equal(direct, s > t), t


def test_run_of_9_on_every_ring():
    """np_fast._has_run_of_9 works on packed ring words; a plain loop over each of the 65536 rings decides the same."""
    rings = (np.arange(65536)[None, :] >> np.arange(16)[:, None] & 1).astype(bool)      # (16, 65536): bit k of ring r
    plain = [any(all(r >> ((k + j) % 16) & 1 for j in range(9)) for k in range(16)) for r in range(65536)]
    assert np.array_equal(np_fast._has_run_of_9(rings), plain) and sum(plain) == 1025


@pytest.mark.parametrize("name", list(HANDMADE))
def test_twin_equals_the_statement_on_handmade_rings(name):
    img, thresholds = HANDMADE[name]
    counts = np_fast.counts_from_histogram(np_fast.histogram(np_fast.score(img)))
    for t in thresholds:
        want = np_fast.keypoints(img, t)
        assert counts[t] == len(want), (name, t)
        pix, used, tried, _ = np_fast.select(img, sc.steer(t))
        assert np.array_equal(pix, want) and (used == t or counts[5] == 0), (name, t, tried)
        got, got_used = fast_select_host(img, sc.steer(t))
        assert np.array_equal(got, want) and got_used == used, (name, t)


def test_handmade_rings_are_what_their_names_say():
    k = lambda name, t: list(np_fast.keypoints(HANDMADE[name][0], t))
    centre = 3 * 7 + 3
    assert k("arc9", 49) == [centre] and k("arc9", 50) == [] and k("arc8", 0) == []      # 9 contiguous, strictly above t
    assert k("wrap", 49) == [centre] and k("dark_wrap", 59) == [centre] and k("dark", 59) == [4 * 7 + 3] and k("dark", 60) == []
    assert k("d_eq_t", 19) == [3 * 9 + 4] and k("d_eq_t", 20) == []                       # d == t is not a corner, d == t + 1 is
    assert k("centre0", 254) == [centre] and k("centre0", 255) == [] and k("centre255", 254) == [centre]
    assert k("t0", 0) == [centre] and k("t0", 5) == []
    b = k("borders", 109)
    assert {3 * 16 + 3, 3 * 16 + 12, 5 * 16 + 3, 5 * 16 + 12} <= set(b) and k("borders", 110) == []
    for name in ("no_interior_rows", "no_interior_cols"):
        assert np.all(np_fast.score(HANDMADE[name][0]) == -1)
        assert len(fast_select_host(HANDMADE[name][0], np_fast.STEREO)[0]) == 0


def test_all_corner_fixture():
    """tests/golden/fast_all_corners.npy (found by a local search): every interior pixel of the 10 x 72 image is a corner at 0."""
    import os
    import cases
    every = np.load(os.path.join(cases.ROOT, "tests", "golden", "fast_all_corners.npy"))
    assert every.shape == (10, 72) and every.dtype == np.uint8 and np.all(np_fast.score(every)[3:-3, 3:-3] > 0)
    got, used = fast_select_host(every, sc.steer(0))
    assert used == 0 and np.array_equal(got, np_fast.keypoints(every, 0)) and len(got) == 4 * 66


def _quirk_cases():
    """name -> (schedule, thresholds it must try) on a 64 x 96 noisy plane, from the plane's own counts c[t]."""
    g = sc.noisy_plane(64, 96, seed=1)
    c = np_fast.counts_from_histogram(np_fast.histogram(np_fast.score(g)))
    assert c[5] - c[6] >= 2 and c[6] > c[7] > c[8] > 0 and c[0] > c[1] > c[4] > c[5]
    return g, c, {
        "no loop: the result is at 5, not at thresh": ((9, BIG, 0, 13), [5]),
        "STEREO's first raise re-evaluates 5": ((4, c[5] - 1, 0, 50), [5, 5, 6]),
        "RGBD's first lowering goes to 8": ((9, BIG, c[4], 13), [5, 8, 7, 6, 5, 4]),
        "the second loop runs after the first overshot": ((4, c[5] - 1, c[5] - 1, 50), [5, 5, 6, 5]),
        "break_thresh ends the first loop above num_want": ((4, 0, 0, 7), [5, 5, 6, 7]),
        "0 ends the second loop below num_min": ((2, BIG, BIG, 50), [5, 1, 0]),
    }


def test_schedule_branches():
    g, c, cases = _quirk_cases()
    for name, (sched, want_tried) in cases.items():
        used, tried, counts = np_fast.schedule(lambda t: c[t], sched)
        assert tried == want_tried and counts == [int(c[t]) for t in want_tried] and used == want_tried[-1], (name, tried, counts)
        pix, used2, tried2, counts2 = np_fast.select(g, sched)  # the direct statement under the same schedule
        assert (used2, tried2, counts2) == (used, tried, counts) and len(pix) == c[used], name
        got, got_used = fast_select_host(g, sched)
        assert np.array_equal(got, pix) and got_used == used, name
    assert c[7] > 0  # (break_thresh stopped a loop that num_want = 0 would have kept running)


@pytest.mark.parametrize("kind,preset,tried", [("textured", np_fast.STEREO, [5, 5, 6, 7, 8, 9, 10, 11]), ("textured", np_fast.RGBD, [5, 10, 11, 12]),
                                               ("flat", np_fast.STEREO, [5, 3]), ("flat", np_fast.RGBD, [5, 8, 7, 6, 5, 4])])
def test_presets_on_a_kitti_sized_frame(kind, preset, tried):
    import np_rgbd
    f = synth.rgbd_frame(kind, rows=376, cols=1241)
    g = np_rgbd.gray_plane(f["image"]).astype(np.uint8)
    pix, used, got_tried, counts = np_fast.select(g, preset)
    assert got_tried == tried and used == tried[-1], (got_tried, counts)
    got, got_used = fast_select_host(g, preset)
    assert np.array_equal(got, pix) and got_used == used and len(got) == counts[-1]
    assert np.all(np.diff(got) > 0)  # row-major


def _raw(rows, cols, gray, sched, pixel=True):
    L = _capi.lib()
    px = np.full(64, -7, np.int32)
    n, used = C.c_int(-7), C.c_int(-7)
    s = _capi.cvo_fast_schedule_t(*sched) if sched is not None else None
    rc = L.cvo_fast_select_host(rows, cols, None if gray is None else gray.ctypes.data_as(C.POINTER(C.c_ubyte)), None if s is None else C.byref(s),
                                px.ctypes.data_as(C.POINTER(C.c_int)) if pixel else None, C.byref(n), C.byref(used))
    assert n.value == -7 and used.value == -7 and np.all(px == -7)  # nothing written on a refusal
    return rc


def test_refusals():
    g = np.zeros((7, 7), np.uint8)
    ok = np_fast.STEREO
    assert _raw(0, 7, g, ok) == _capi.CVO_E_INVALID and _raw(7, -1, g, ok) == _capi.CVO_E_INVALID
    assert _raw(7, 7, None, ok) == _capi.CVO_E_INVALID and _raw(7, 7, g, None) == _capi.CVO_E_INVALID
    assert _raw(7, 7, g, ok, pixel=False) == _capi.CVO_E_INVALID
    for bad in ((-1, 10, 5, 50), (4, -1, -2, 50), (4, 10, -1, 50), (4, 10, 5, -1), (4, 10, 11, 50), (256, 10, 5, 50)):
        assert _raw(7, 7, g, bad) == _capi.CVO_E_INVALID, bad
    assert _raw(4097, 4096, g, ok) == _capi.CVO_E_UNSUPPORTED  # more than 2^24 pixels (refused before the plane is read)
    with pytest.raises(CvoError):
        fast_select_host(g, (4, 10, 11, 50))
    pix, used = fast_select_host(np.zeros((3, 2), np.uint8), ok)  # smaller than 7 on a side: valid, no corners
    assert len(pix) == 0 and used == 0
