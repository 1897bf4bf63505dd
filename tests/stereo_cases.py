"""The frames the stereo and FAST tests share (CPU twin and device), the numpy statement's results on them - computed once
per process and left unchanged - and the hand-made FAST images."""
import functools

import numpy as np

import np_fast
import np_stereo
from unified_cvo_amd import StereoFrame, synth

# name -> kwargs of synth.stereo_frame
FRAMES = {
    "kitti": dict(kind="textured"),                               # 376 x 1241
    "flat": dict(kind="flat"),                                    # the FAST schedule lowers its threshold
    "narrow": dict(kind="textured", rows=140, cols=72),           # only v = 100 .. 110 survive
    "row130": dict(kind="textured", rows=130, cols=200),          # 100 <= v <= rows - 30: the one row v = 100
    "short": dict(kind="textured", rows=129, cols=200),           # fewer than 130 rows: empty
    "mono": dict(kind="textured", rows=200, cols=320, channels=1),
    "semantic": dict(kind="textured", num_classes=19),            # the 28000 preset (stops at 10, not 11), class 10 present
}
METHODS = (np_stereo.CV_FAST, np_stereo.DSO_EDGES, np_stereo.FULL)


@functools.lru_cache(maxsize=None)
def frame(name, shift=0.0, nan_pixels=True):
    return StereoFrame(**synth.stereo_frame(shift=shift, nan_pixels=nan_pixels, **FRAMES[name]))


def calib(f):
    return (f.fx, f.fy, f.cx, f.cy, f.baseline)


def points_of(f, method):
    return np_stereo.points(f.image, f.gray, f.disparity, calib(f), f.semantic, method)


@functools.lru_cache(maxsize=None)
def statement_points(name, method, shift=0.0):
    return points_of(frame(name, shift), method)


@functools.lru_cache(maxsize=None)
def statement_recipe(name, leaf, divisor=5):
    f = frame(name, 0.0, False)
    return np_stereo.recipe(f.image, f.gray, f.disparity, calib(f), f.semantic, leaf, divisor)


def _ring_image(rows, cols, x, y, centre, ring, background=None):
    """An image whose pixel (x, y) has value `centre` and ring values `ring` (16); everything else `background` (default:
    the centre value, so that no other pixel sees a contrast of its own making unless the ring creates one)."""
    img = np.full((rows, cols), centre if background is None else background, np.uint8)
    for (dx, dy), val in zip(np_fast.RING, ring):
        img[y + dy, x + dx] = val
    img[y, x] = centre
    return img


def _arc(start, length, inside, outside):
    return [inside if (k - start) % 16 < length else outside for k in range(16)]


def handmade():
    """name -> (image, thresholds at which the test compares the detector).  7 x 7 ... 9 x 16 images around one ring each."""
    out = {}
    out["arc9"] = (_ring_image(7, 7, 3, 3, 100, _arc(2, 9, 150, 100)), (0, 10, 49, 50))
    out["arc8"] = (_ring_image(7, 7, 3, 3, 100, _arc(2, 8, 150, 100)), (0, 10, 49))
    out["wrap"] = (_ring_image(7, 7, 3, 3, 100, _arc(12, 9, 150, 100)), (0, 10, 49, 50))      # ring pixels 12 .. 15, 0 .. 4
    out["d_eq_t"] = (_ring_image(7, 9, 4, 3, 100, _arc(0, 9, 120, 100)), (19, 20, 21))        # d = 20: a corner at 19, not at 20
    out["dark"] = (_ring_image(8, 7, 3, 4, 100, _arc(5, 9, 40, 100)), (0, 59, 60))
    out["dark_wrap"] = (_ring_image(7, 7, 3, 3, 100, _arc(10, 10, 40, 100)), (0, 59, 60))
    out["centre0"] = (_ring_image(7, 7, 3, 3, 0, _arc(0, 9, 255, 0)), (0, 200, 254, 255))     # p - t below 0; d = 255
    out["centre255"] = (_ring_image(7, 7, 3, 3, 255, _arc(7, 9, 0, 255)), (0, 200, 254, 255))  # p + t above 255
    out["t0"] = (_ring_image(7, 7, 3, 3, 100, _arc(0, 9, 101, 100)), (0, 5, 6))                 # d = 1: a corner at t = 0 only
    wide = np.full((9, 16), 90, np.uint8)
    for x, y in ((3, 3), (12, 3), (3, 5), (12, 5)):                                            # the interior's first / last row and column
        for dx, dy in np_fast.RING[:9]:
            wide[y + dy, x + dx] = 200
    out["borders"] = (wide, (0, 50, 109, 110))
    out["no_interior_rows"] = (np.tile(np.arange(40, dtype=np.uint8) * 6, (6, 1)), (0, 5))
    out["no_interior_cols"] = (np.ascontiguousarray(np.tile(np.arange(40, dtype=np.uint8) * 6, (6, 1)).T), (0, 5))
    return out


def steer(t):
    """A schedule whose last detector call is at threshold t, for t = 0, 5 or >= 6 (when the image has a keypoint at 5; with
    none it has none at t either, and the call at 5 stands): the lowering loop runs to 0 / no loop / one raise to break_thresh."""
    assert t == 0 or t >= 5
    return (1, 10 ** 9, 10 ** 9, 0) if t == 0 else ((5, 10 ** 9, 0, 0) if t == 5 else (t - 1, 0, 0, t))


def noisy_plane(rows, cols, seed=0, amplitude=40):
    rs = np.random.default_rng(77100 + seed)
    v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    base = 128 + 50 * np.sin(0.3 * u) * np.cos(0.2 * v)
    return np.clip(np.rint(base + rs.uniform(-amplitude, amplitude, (rows, cols))), 0, 255).astype(np.uint8)


def bits(a):
    """The bit patterns of float32 values, every NaN as one canonical pattern (IEEE 754 leaves a NaN's payload and sign to
    the implementation; the NaN-disparity rows are NaN on every route)."""
    a = np.ascontiguousarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


def assert_points_equal(pc, want, name):
    """Indices equal, float rows bit-equal (a NaN equals a NaN)."""
    assert np.array_equal(pc.pixel, want["pixel"]), name
    assert pc.num_points() == len(want["pixel"]), name
    assert np.array_equal(bits(pc.positions()), bits(want["xyz"])), name
    assert pc.features().shape == want["feat"].shape and np.array_equal(bits(pc.features()), bits(want["feat"])), name
    assert np.array_equal(bits(pc.geometric_types_), bits(want["geotype"])), name
    if want["label"] is not None:
        assert np.array_equal(bits(pc.labels()), bits(want["label"])), name
