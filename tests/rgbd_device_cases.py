"""What the device-frame RGB-D tests share (CPU twin and device): the three presentations of one plane of class scores, the
hand-made 4 x 8 frames at the exclusion rule's edges, and the comparison of rows against the numpy statement."""
import functools

import numpy as np

import np_rgbd
import np_rgbd_device as nd
import rgbd_cases as rc
from unified_cvo_amd import RGBDFrame

LAYOUTS = ("hwc", "chw", "slice")


def presentations(sem):
    """{name: (base array that owns the bytes, view of it that holds the scores, layout of the view)} of one (h, w, C) plane:
    H x W x C as it is, C x H x W, and a column slice of a wider array - pixel stride larger than 4 C, row stride padded."""
    sem = np.ascontiguousarray(sem, np.float32)
    h, w, c = sem.shape
    chw = np.ascontiguousarray(np.moveaxis(sem, 2, 0))
    wide = np.full((h, w + 3, c + 5), 7.5, np.float32)
    wide[:, 1:w + 1, 2:2 + c] = sem
    view = wide[:, 1:w + 1, 2:2 + c]
    assert view.strides[1] > 4 * c and view.strides[0] > w * view.strides[1]
    return {"hwc": (sem, sem, "hwc"), "chw": (chw, chw, "chw"), "slice": (wide, view, "hwc")}


def strides_of(view, layout):
    """(row, pixel, class) strides in bytes and the class count of a presentation's view."""
    r, p, c = (0, 1, 2) if layout == "hwc" else (1, 2, 0)
    return (view.strides[r], view.strides[p], view.strides[c]), view.shape[c]


def calib(f):
    return (f.fx, f.fy, f.cx, f.cy, f.scaling_factor)


def statement_points(f, method, semantic=None, layout="hwc"):
    with np.errstate(all="ignore"):
        return nd.points(f.image, f.gray, f.depth, calib(f), f.semantic if semantic is None else semantic, method, layout)


def statement_recipe(f, leaf, divisor=4):
    return nd.recipe(f.image, f.gray, f.depth, calib(f), f.semantic, leaf, divisor)


def assert_rows_equal(got, want, name, labels=True):
    """got: dict of xyz, feat, label, geotype (the twin's, or a downloaded cloud's); want: the statement's."""
    bits = rc.bits
    assert got["xyz"].shape == want["xyz"].shape, name
    assert np.array_equal(bits(got["xyz"]), bits(want["xyz"])), name
    assert got["feat"].shape == want["feat"].shape and np.array_equal(bits(got["feat"]), bits(want["feat"])), name
    assert np.array_equal(bits(got["geotype"]), bits(want["geotype"])), name
    if labels and want.get("label") is not None:
        assert got["label"] is not None and np.array_equal(bits(got["label"]), bits(want["label"])), name


# ---- the exclusion rule's edges: 4 x 8 frames, every pixel with a depth, so FULL keeps exactly what the rule keeps ----------

H, W = 4, 8


def _base(seed=0):
    rs = np.random.default_rng(7300000 + seed)
    image = rs.integers(0, 256, (H, W, 3)).astype(np.uint8)
    depth = (3000 + 37 * np.arange(H * W).reshape(H, W)).astype(np.uint16)
    return image, depth


def _frame(sem, seed=0):
    image, depth = _base(seed)
    return RGBDFrame(image, depth, 6.5, 6.25, 3.5, 1.5, 5000.0, semantic=None if sem is None else np.ascontiguousarray(sem, np.float32))


def _scores(classes, winners, seed):
    """(H, W, classes) distinct scores below 0.5 with 0.9 at winners[v, u] (-1: no winner is set)."""
    rs = np.random.default_rng(7310000 + seed)
    sem = (rs.permuted(np.tile(np.arange(classes, dtype=np.float32), (H, W, 1)), axis=2) + 1) / np.float32(4 * classes)
    for v in range(H):
        for u in range(W):
            if winners[v, u] >= 0:
                sem[v, u, winners[v, u]] = 0.9
    return sem.astype(np.float32)


def _checker(a, b):
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.where((v + u) % 2 == 0, a, b)
    out[H - 1, W - 1] = a if b == 10 else b  # (the last pixel of the frame is one of the kept kind in every case)
    return out


def _classes(n):
    return _frame(_scores(n, _checker(min(10, n - 1), 0), n), n)


def _shared(first, second, lone):
    """Half the pixels: the maximum shared by classes `first` and `second`; the others: class `lone` alone."""
    win = _checker(first, lone)
    sem = _scores(19, win, 100 + first + second)
    v, u = np.nonzero(win == first)
    sem[v, u, second] = 0.9
    return _frame(sem, 100 + first)


def _all_equal():
    """Half the pixels (and the last one): all 19 scores equal; the others: class 10 alone."""
    win = _checker(-1, 10)
    sem = _scores(19, win, 300)
    v, u = np.nonzero(win == -1)
    sem[v, u, :] = 0.25
    return _frame(sem, 300)


RULE_CASES = {
    "classes_1": lambda: _classes(1), "classes_10": lambda: _classes(10), "classes_11": lambda: _classes(11), "classes_19": lambda: _classes(19),
    "shared_10_12": lambda: _shared(10, 12, 4),   # first maximum 10: excluded
    "shared_3_10": lambda: _shared(3, 10, 10),    # first maximum 3: kept (the lone class 10 pixels are excluded)
    "all_equal": _all_equal,                      # first maximum 0: kept
}
# with 10 or fewer classes there is no class 10: the rule can exclude nothing there, and the test asserts exactly that
RULE_EXCLUDES = {name: name not in ("classes_1", "classes_10") for name in RULE_CASES}


@functools.lru_cache(maxsize=None)
def rule_frame(name):
    return RULE_CASES[name]()


def nan_frame():
    """19 classes; NaN scores at, before and after the maximum, and a row of NaN only."""
    win = _checker(10, 5)
    sem = _scores(19, win, 400)
    sem[0, 0, 10] = np.nan   # the winner itself: the next best wins
    sem[0, 1, 0] = np.nan    # best = 0 starts at a NaN: nothing is greater than a NaN, class 0 stays
    sem[0, 2, 18] = np.nan   # after the maximum
    sem[1, 1, 3] = np.nan    # before the maximum
    sem[2, 2, :] = np.nan
    return _frame(sem, 400)


def all_pixels():
    return np.arange(H * W, dtype=np.int32)


def border(pixel, h=H, w=W):
    v, u = np.asarray(pixel) // w, np.asarray(pixel) % w
    return (v < 1) | (u < 1) | (v > h - 2) | (u > w - 2)


FULL, DSO_EDGES = np_rgbd.FULL, np_rgbd.DSO_EDGES
