"""The frames the RGB-D tests share (CPU twin and device), and the comparison against the numpy statement."""
import functools

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
    with np.errstate(all="ignore"):  # (the depth edge cases multiply 0 by inf on purpose)
        return np_rgbd.points(f.image, f.gray, f.depth, (f.fx, f.fy, f.cx, f.cy, f.scaling_factor), f.semantic, method)


def statement_recipe(f, leaf, divisor=4):
    return np_rgbd.recipe(f.image, f.gray, f.depth, (f.fx, f.fy, f.cx, f.cy, f.scaling_factor), f.semantic, leaf, divisor)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_points_equal(pc, want, name, nan_coordinates=False):
    """Indices equal, float rows bit-equal.  nan_coordinates: where the statement's coordinate is a NaN a NaN is required,
    of any sign and payload (x86 and the device may differ there); every other coordinate is still compared bit for bit."""
    assert np.array_equal(pc.pixel, want["pixel"]), name
    assert pc.num_points() == len(want["pixel"]), name
    if nan_coordinates:
        nan = np.isnan(want["xyz"])
        assert np.array_equal(np.isnan(pc.positions()), nan), name
        assert np.array_equal(bits(pc.positions())[~nan], bits(want["xyz"])[~nan]), name
    else:
        assert np.array_equal(bits(pc.positions()), bits(want["xyz"])), name
    assert pc.features().shape == want["feat"].shape and np.array_equal(bits(pc.features()), bits(want["feat"])), name
    assert np.array_equal(bits(pc.geometric_types_), bits(want["geotype"])), name
    if want["label"] is not None:
        assert np.array_equal(bits(pc.labels()), bits(want["label"])), name


# ---- edge cases: the selector's block, cell and threshold edges (test_rgbd_cpu.py asserts that each reaches its edge) -------
#
# Every case is a builder of a small RGBDFrame: a gray plane (one channel unless its name says bgr or squares), a depth
# image and a calibration.  The constructed planes are mostly constant along y, so that g2 = dx^2 is set column by column.

POTS = tuple(range(2, 8))
# no considered pixel, then the first; no whole block, then one (and 1023 / 1024 / 1025 pixels); a ragged last block column
# and row; 1024 cells at potential 2 and one block column or row of cells more
STRUCTURE_SHAPES = ((7, 9), (8, 10), (9, 11), (31, 31), (32, 32), (33, 33), (31, 33), (25, 41), (63, 63), (64, 64), (65, 65), (33, 63),
                    (64, 95), (95, 64), (64, 65), (65, 64))
# rows and cols with remainders 0, 1 and 4 pot - 1 modulo 4 pot for every potential: 120 = 0 mod 8, 12, 20, 24 and 112 = 0
# mod 8, 16, 28, with their neighbours
RESIDUE_SHAPES = ((119, 120), (120, 121), (121, 119), (111, 112), (112, 113), (113, 111), (120, 112), (113, 119))
WIDE = (36, 3205)          # the widest accepted image of 36 rows: its threshold index reaches entry 199 of 200
WIDE_REFUSED = (36, 3206)  # ... and the first refused one: entry 200 of 200


def _noise(rows, cols):
    """Noise whose amplitude drifts over the image, so that neighbouring blocks have different thresholds."""
    rs = np.random.default_rng(5100000 + 4099 * rows + cols)
    y, x = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    amp = 4.0 + 60.0 * (0.5 + 0.5 * np.sin(0.09 * x + 0.13 * y))
    return np.clip(np.rint(128.0 + amp * rs.uniform(-1.0, 1.0, (rows, cols))), 0, 255).astype(np.uint8)


def _frame(image, depth=None, calib=None):
    image = np.ascontiguousarray(image, np.uint8)
    rows, cols = image.shape[:2]
    if depth is None:  # ordinary depths with holes
        i = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
        depth = (4000 + 61 * (i % 97)).astype(np.uint16)
        depth[i % 7 == 3] = 0
    fx, fy, cx, cy, scale = calib or (525.0 * cols / 640.0, 525.0 * rows / 480.0, 319.5 * cols / 640.0, 239.5 * rows / 480.0, 5000.0)
    return RGBDFrame(image, depth, fx, fy, cx, cy, scale)


def _profile(m, c=100, mid=128):
    """Gray levels g along x with |0.5 (g[x + 1] - g[x - 1])| = m[x] for 1 <= x <= len(m) - 2: each of the two interleaved
    chains steps towards `mid`, which keeps them inside 0 .. 255 for the magnitudes used here."""
    g = np.zeros(len(m), np.int64)
    g[0] = g[1] = c
    for x in range(1, len(m) - 1):
        g[x + 1] = g[x - 1] + (2 * int(m[x]) if g[x - 1] <= mid else -2 * int(m[x]))
    assert g.min() >= 0 and g.max() <= 255, (g.min(), g.max())
    return g


def _columns(m, rows=96, **kw):
    """A plane that is constant along y with column roots m[x] (dy = 0 everywhere)."""
    return np.tile(_profile(m, **kw), (rows, 1))


def _hist_flat():
    img = np.full((96, 96), 100, np.int64)
    img[10, 10] = 200  # (something to select, outside the block under test)
    return _frame(img)


def _hist_cap():
    """Pairs of columns 0, 0, 255, 255: |dx| = 127.5 everywhere off the border (single alternating columns have a zero
    central difference), every root 127, capped to bin 48."""
    return _frame(np.tile(np.where(np.arange(96) % 4 >= 2, 255, 0), (96, 1)))


def _hist_47_48_49():
    """The centre block's columns: 8 with root 47, 4 with 48, 20 with 49.  Capped at 48 the quantile is 48; capped at 47 it is
    47; not capped it would be 49."""
    m = np.full(96, 10)
    m[32:40], m[40:44], m[44:64] = 47, 48, 49
    return _frame(_columns(m))


def _quantile(extra):
    """Blocks with th = int(count * 0.5f + 0.5f) + extra pixels in bin 0 and the rest in bin 5: the centre block (count 1024,
    th 512), the top edge block (0, 1) (992, 496) and the corner block (2, 2) (961, 481).  Columns 32 .. 47 and 64 .. 79 are
    flat, 48 .. 63 and 80 .. 94 have |dx| = 5; column 64 of the corner block is moved between the bins row by row through the
    gray level of column 63, and single pixels of column 63 through column 64."""
    m = np.zeros(96, np.int64)
    m[48:64] = 5
    m[80:95] = 5
    img = _columns(m)
    for y in range(66, 66 + 15 - extra):   # corner block: 16 x 31 - 15 = 481 flat pixels, 482 with one row fewer
        img[y, 63] += 10                   # (y, 64): |dx| = 5
    if extra:
        img[45, 64] = img[45, 62]          # centre block: (45, 63) becomes flat, 513
        img[10, 64] = img[10, 62]          # top edge block: (10, 63) becomes flat, 497
    return _frame(img)


def _hist_wave_ramp():
    """Centre block: |dx| = x - 32 and |dy| = 0 on even, 40 on odd rows, so a wave's two block rows hold the roots 0 .. 31
    and 40 .. 48: 41 distinct bins."""
    m = np.zeros(96, np.int64)
    m[32:64] = np.arange(32)
    y = np.arange(96)
    q = np.where(y % 4 == 2, 80, 0)  # |0.5 (q[y + 1] - q[y - 1])| = 40 on odd rows, 0 on even ones
    img = _profile(m, c=60, mid=80)[None, :] + q[:, None]
    assert img.min() >= 0 and img.max() <= 255
    return _frame(img)


def _smooth_3x3():
    """Nine blocks of noise with nine amplitudes: nine distinct thresholds, so corner, edge and centre blocks average 4, 6
    and 9 different neighbours."""
    rs = np.random.default_rng(5200001)
    amp = np.repeat(np.repeat(np.array([[4, 28, 12], [44, 8, 36], [20, 52, 60]], np.float64), 32, axis=0), 32, axis=1)
    return _frame(np.clip(np.rint(128.0 + amp * rs.uniform(-1.0, 1.0, (96, 96))), 0, 255))


TIE_POKES = tuple((y, x) for y in range(8, 88, 9) for x in range(8, 88, 9))


def _sel_tie():
    """Single pixels raised by 60 on a flat plane: each leaves g2 = 900 at its four neighbours, and the cells that hold
    several of them differ from potential to potential."""
    img = np.full((96, 96), 100, np.int64)
    for y, x in TIE_POKES:
        img[y, x] += 60
    return _frame(img)


THRESHOLD_EQUAL, THRESHOLD_ABOVE = (20, 20), (40, 40)


def _sel_threshold():
    """A flat plane's smoothed threshold is 49 = 7^2.  (20, 20) has dx = 7, dy = 0: g2 = 49, not selected; (40, 40) has dx = 7,
    dy = 0.5: g2 = 49.25, the next multiple of 0.25, selected."""
    img = np.full((64, 64), 100, np.int64)
    img[20, 21] += 14
    img[40, 41] += 14
    img[41, 40] += 1
    return _frame(img)


BORDER_SHAPE = (64, 70)


def border_targets():
    """(y, x, is it considered) of the strong pixels of sel_border: x in {3, 4, w - 6, w - 5} and y in {3, 4, h - 4, h - 3}."""
    h, w = BORDER_SHAPE
    across = [(y, x, k in (1, 2)) for k, (x, y) in enumerate(zip((3, 4, w - 6, w - 5), (20, 30, 40, 50)))]
    down = [(y, x, k in (1, 2)) for k, (y, x) in enumerate(zip((3, 4, h - 4, h - 3), (20, 30, 40, 50)))]
    return across, down


def _sel_border():
    """g2 = 3600 at each target (its two neighbours along one axis are 40 and 160), 900 at the pixels around them."""
    img = np.full(BORDER_SHAPE, 100, np.int64)
    across, down = border_targets()
    for y, x, _ in across:
        img[y, x - 1], img[y, x + 1] = 40, 160
    for y, x, _ in down:
        img[y - 1, x], img[y + 1, x] = 40, 160
    return _frame(img)


def _sel_squares():
    """synth.rgbd_frame's staircases at 64 x 64: g2 = 25 and 169 inside histogrammed blocks (3 channels)."""
    return RGBDFrame(**synth.rgbd_frame(kind="textured", rows=64, cols=64))


def bgr_boundary_triples():
    """(B, G, R) with (1868 B + 9617 G + 4899 R + 8192) mod 2^14 equal to 0 - the level has just been reached - and to
    2^14 - 1 - it is just missed -, found by solving for R."""
    b, g = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    inv = pow(4899, -1, 1 << 14)
    out = []
    for target in (0, (1 << 14) - 1):
        r = ((target - (1868 * b + 9617 * g + 8192)) * inv) % (1 << 14)
        ok = r < 256
        out.append(np.stack([b[ok], g[ok], r[ok]], axis=1))
    return out


def _bgr_rounding():
    reached, missed = bgr_boundary_triples()
    both = np.concatenate([reached, missed])
    rs = np.random.default_rng(5200002)
    return _frame(both[rs.integers(0, len(both), 40 * 40)].reshape(40, 40, 3))


DEPTH_F32 = np.array([0.0, -0.0, np.nan, np.inf, -1.5, 1e-45, 1e30, 2.5, 0.75], np.float32)  # (1e-45: the smallest denormal)
DEPTH_U16 = np.array([0, 1, 65535, 5000, 12345], np.uint16)
DEPTH_CALIB = (50.0, 50.0, 12.0, 20.5, 1.0)  # cx = 12 exactly: u == cx under an infinite depth is 0 * inf


def _depth(values):
    rs = np.random.default_rng(5200003)
    depth = values[rs.integers(0, len(values), (40, 48))]
    if values.dtype == np.float32:
        depth[:, 12] = np.inf
    return _frame(_noise(40, 48), depth, DEPTH_CALIB if values.dtype == np.float32 else None)


def _shape_name(shape):
    return "shape_%dx%d" % shape


EDGE_CASES = {_shape_name(s): (lambda s=s: _frame(_noise(*s))) for s in STRUCTURE_SHAPES + RESIDUE_SHAPES + (WIDE,)}
EDGE_CASES.update({
    "hist_flat": _hist_flat, "hist_cap": _hist_cap, "hist_47_48_49": _hist_47_48_49,
    "quantile_at": lambda: _quantile(0), "quantile_above": lambda: _quantile(1),
    "hist_wave_ramp": _hist_wave_ramp, "smooth_3x3": _smooth_3x3,
    "sel_tie": _sel_tie, "sel_threshold": _sel_threshold, "sel_border": _sel_border, "sel_squares": _sel_squares,
    "bgr_rounding": _bgr_rounding,
    "depth_f32": lambda: _depth(DEPTH_F32), "depth_u16": lambda: _depth(DEPTH_U16),
})
NAN_COORDINATES = ("depth_f32",)  # cases whose statement holds NaN coordinates (assert_points_equal(nan_coordinates=True))


def refused_frame():
    return _frame(_noise(*WIDE_REFUSED))


def edge_order():
    """The cases in an order that alternates large and small frames, the widest immediately before 33 x 33: a context's
    scratch region is reused, and its thresholds zeroed again, across the largest changes of shape."""
    by_size = sorted(EDGE_CASES, key=lambda n: (-edge_frame(n).rows * edge_frame(n).cols, n))
    by_size.remove(_shape_name((33, 33)))
    order = []
    while by_size:
        order.append(by_size.pop(0))
        if len(order) == 1:
            order.append(_shape_name((33, 33)))
        elif by_size:
            order.append(by_size.pop())
    return order


@functools.lru_cache(maxsize=None)
def edge_frame(name):
    return EDGE_CASES[name]()


@functools.lru_cache(maxsize=None)
def edge_statement(name):
    """The statement's stages and points of an edge case, computed once and shared read-only: g2 (h, w), ths, sm, selected
    {potential: pixel indices}, points {method: np_rgbd.points}."""
    f = edge_frame(name)
    I = np_rgbd.gray_plane(f.image, f.gray)
    h, w = I.shape
    _, g2 = np_rgbd.gradient(I)
    ths, sm, _ = np_rgbd.thresholds(g2, h, w)
    out = dict(g2=g2.reshape(h, w), ths=ths, sm=sm, selected={p: np_rgbd.select(g2, sm, h, w, p) for p in POTS},
               points={m: statement_points(f, m) for m in (np_rgbd.DSO_EDGES, np_rgbd.FULL)})
    for a in (out["g2"], ths, sm) + tuple(out["selected"].values()):
        a.setflags(write=False)
    return out


def block_bins(g2, h, w, bx, by):
    """The 49 bin counts makeHists sees in block (bx, by), as np_rgbd.thresholds counts them."""
    jt, it = np.meshgrid(np.arange(32) + 32 * by, np.arange(32) + 32 * bx, indexing="ij")
    ok = ~((it > w - 2) | (jt > h - 2) | (it < 1) | (jt < 1))
    g = np.sqrt(np.asarray(g2, np.float32).reshape(h, w)[jt[ok], it[ok]]).astype(np.int64)
    return np.bincount(np.minimum(g, 48), minlength=49)


def first_difference(back, want):
    """None when a read-back (CvoGPU.debug_rgbd_readback) equals the statement's stages (edge_statement), else a message
    naming the first differing stage - g2, ths, sm, then the selections at the potentials 2 .. 7 - and its first differing
    index."""
    stages = [(k, bits(back[k]).reshape(-1), bits(want[k]).reshape(-1)) for k in ("g2", "ths", "sm")]
    stages += [("selection at potential %d" % p, np.asarray(back["selected"][p]), np.asarray(want["selected"][p])) for p in POTS]
    for stage, got, ref in stages:
        k = min(len(got), len(ref))
        bad = np.flatnonzero(got[:k] != ref[:k])
        if len(bad) == 0 and len(got) == len(ref):
            continue
        size = "" if len(got) == len(ref) else f" {len(got)} entries for {len(ref)},"
        if len(bad) == 0:
            return f"first differing stage {stage}:{size} equal up to entry {k}"
        i = int(bad[0])
        show = (lambda a: a[i:i + 1].view(np.float32)[0]) if got.dtype == np.uint32 else (lambda a: a[i])
        return f"first differing stage {stage}:{size} {len(bad)} entries differ, first at {i}: {show(got)} for {show(ref)}"
    return None
