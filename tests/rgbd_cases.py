"""The frames the RGB-D tests share (CPU twin and device), and the comparison against the numpy statement."""
import numpy as np

import np_rgbd
from unified_cvo_amd import RGBDFrame, synth

# name -> (kwargs of synth.rgbd_frame, the potentials the selector's schedule must try)
FRAMES = {
    "textured": (dict(kind="textured"), [3, 4, 5]),                         # stops at 5
    "smoother": (dict(kind="smoother"), [3, 4]),                            # stops at 4
    "flat": (dict(kind="flat"), [3, 2]),                                    # fewer than 6666 -> back to 2
    "edge": (dict(kind="edge"), [3, 4, 3]),                                 # falls back to 3 and ends above 10 000
    "noisy720": (dict(kind="noisy", rows=720, cols=1280), [3, 4, 5, 6, 7]),  # the times == 5 exit
    "kitti": (dict(kind="textured", rows=376, cols=1241), [3, 4, 5, 6, 7]),  # threshold aliasing, cols % 32 != 0
    "small": (dict(kind="textured", rows=150, cols=200), [3, 2]),           # reads block column 6 of 6
    "tiny": (dict(kind="textured", rows=20, cols=40), [3, 2]),              # no whole block: zero thresholds
    "mono": (dict(kind="textured", channels=1), None),
    "semantic": (dict(kind="textured", rows=240, cols=320, num_classes=19), None),
}
DEPTHS = ("u16", "f32")


def frame(name, depth="u16", **extra):
    kw = dict(FRAMES[name][0])
    kw.update(extra)
    return RGBDFrame(**synth.rgbd_frame(depth=depth, **kw))


def own_gray(f):
    """A frame whose caller-supplied gray plane differs from the formula (the green channel)."""
    g = np.ascontiguousarray(f.image[..., 1])
    assert not np.array_equal(g.astype(np.float32), np_rgbd.gray_plane(f.image))
    return RGBDFrame(f.image, f.depth, f.fx, f.fy, f.cx, f.cy, f.scaling_factor, gray=g, semantic=f.semantic)


def zero_depth(f):
    return RGBDFrame(f.image, np.zeros_like(f.depth), f.fx, f.fy, f.cx, f.cy, f.scaling_factor)


def statement_points(f, method):
    return np_rgbd.points(f.image, f.gray, f.depth, (f.fx, f.fy, f.cx, f.cy, f.scaling_factor), f.semantic, method)


def statement_recipe(f, leaf, divisor=4):
    return np_rgbd.recipe(f.image, f.gray, f.depth, (f.fx, f.fy, f.cx, f.cy, f.scaling_factor), f.semantic, leaf, divisor)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_points_equal(pc, want, name):
    """Indices equal, float rows bit-equal."""
    assert np.array_equal(pc.pixel, want["pixel"]), name
    assert pc.num_points() == len(want["pixel"]), name
    assert np.array_equal(bits(pc.positions()), bits(want["xyz"])), name
    assert pc.features().shape == want["feat"].shape and np.array_equal(bits(pc.features()), bits(want["feat"])), name
    assert np.array_equal(bits(pc.geometric_types_), bits(want["geotype"])), name
    if want["label"] is not None:
        assert np.array_equal(bits(pc.labels()), bits(want["label"])), name
