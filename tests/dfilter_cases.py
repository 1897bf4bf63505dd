"""Inputs of the disparity post-filter's tests (test_dfilter_cpu.py, test_gpu_dfilter.py, test_cpp_dfilter.py), the generator
of the golden fixture's map (scripts/make_dfilter_golden.py) and a cache of the statement's stages (np_dfilter.stages), computed
once per case and shared, read-only.  A case is (map, np_dfilter.Config).  TILE_W x TILE_H is the kernels' tile; the GPU tests
check it against what cvo_debug_dfilter_stats reports."""
import numpy as np

import np_dfilter
from np_dfilter import Config

F = np.float32
INV = F(-10.0)
TILE_W, TILE_H = 64, 4
_cache = {}


def golden_input():
    """The 80 x 96 map of tests/golden/dfilter_elas.npz, made so that every pass acts: a noisy plane with blocks offset by 1.5,
    3 and 9 (the mean's three weight classes), pin-holes, wrong single matches, islands of 199, 200 and 201 pixels, holes 3 and 4
    wide, holes that touch the line ends, and negative values other than -10."""
    rng = np.random.default_rng(7)
    H, W = 80, 96
    y, x = np.mgrid[0:H, 0:W]
    d = (12 + 0.05 * x + 0.1 * y + rng.uniform(-0.3, 0.3, (H, W))).astype(F)
    d[12:30, 40:60] += F(1.5)
    d[35:55, 8:30] += F(3.0)
    d[50:72, 60:86] += F(9.0)
    d[rng.random((H, W)) < 0.03] = INV
    wrong = rng.choice(H * W, 15, replace=False)
    d.flat[wrong] = (100 + rng.uniform(0, 50, 15)).astype(F)
    # islands: 25 x 8 = 200 pixels, one short, exact, one more; far (> 1) from the plane
    for x0, value, n in ((2, 60, 199), (34, 70, 200), (66, 80, 201)):
        d[2:10, x0:x0 + 25] = (value + rng.uniform(-0.2, 0.2, (8, 25))).astype(F)
        if n == 199:
            d[9, x0 + 24] = d[10, x0 + 24]
        if n == 201:
            d[10, x0 + 12] = F(value)
    d[33:38, 33:36] = INV   # 3 wide, 5 high: the row pass fills it
    d[42:46, 33:37] = INV   # 4 x 4: stays
    d[20:23, 70:75] = INV   # 3 high, 5 wide: the column pass fills it
    d[58:63, 0:2] = INV     # at a line end for the rows, too long for the columns: stays; and so on around the border
    d[58:63, W - 2:] = INV
    d[0:2, 48:53] = INV
    d[H - 2:, 48:53] = INV
    d[25, 5:8] = F(-2.5)
    d[64, 40] = F(-1.5)
    return d


def golden():
    key = "golden file"
    if key not in _cache:
        import os
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dfilter_elas.npz"))
        _cache[key] = {k: z[k] for k in z.files}
    return _cache[key]


def _blank(H, W):
    return np.full((H, W), INV, F)


def _hook(d, y, x, n, value=5.0):
    """n pixels: a bar along row y from column x to the right, 12 long at most, then down its last column"""
    a = min(n, 12)
    d[y, x:x + a] = F(value)
    d[y + 1:y + 1 + n - a, x + a - 1] = F(value)


def speckle_straddle(size=20, tw=TILE_W, th=TILE_H):
    """segments of size - 1, size and size + 1 pixels, each across a vertical and several horizontal tile borders"""
    d = _blank(3 * th + size + 8, 3 * tw + 8)
    for i, n in enumerate((size - 1, size, size + 1)):
        _hook(d, th - 1 + (i % 2), (i + 1) * tw - 6, n, 5.0 + i)
    return d, Config(1.0, size, 0, 0)


def serpentine(H=33, W=130, extra=0):
    """one segment winding through every row: long parent chains; speckle_size = its size + extra"""
    d = _blank(H, W)
    d[0::2, :] = F(7)
    for i, r in enumerate(range(1, H, 2)):
        d[r, W - 1 if i % 2 == 0 else 0] = F(7)
    return d, Config(1.0, int((d >= 0).sum()) + extra, 0, 0)


def comb(H=31, W=130, extra=0):
    d = _blank(H, W)
    d[0, :] = F(3)
    d[:, 0::2] = F(3)
    return d, Config(1.0, int((d >= 0).sum()) + extra, 0, 0)


def constant(H=256, W=256):
    return np.full((H, W), 12.5, F), Config(1.0, H * W, 0, 0)


def checkerboard(H=9, W=70):
    y, x = np.mgrid[0:H, 0:W]
    return np.where((x + y) % 2 == 0, F(0), F(5)).astype(F), Config(1.0, 2, 0, 0)


def sim_edge(sim=1.0):
    """row 0: neighbours exactly `sim` apart (they join); row 2: the next float above (they do not)"""
    d = _blank(4, 70)
    d[0, :] = np.arange(4, 74, dtype=F) * F(sim)
    d[2, 0::2] = F(4)
    d[2, 1::2] = np.nextafter(F(4) + F(sim), F(np.inf))
    return d, Config(sim, 3, 0, 0)


def random_map(H, W, seed=0, invalid=0.15, steps=(0.0, 1.5, 3.0, 9.0)):
    """a plane with per-pixel offsets from `steps` (the mean's weight classes), noise, and invalid pixels"""
    rng = np.random.default_rng(seed)
    d = (20 + rng.choice(np.array(steps, F), (H, W)) + rng.uniform(-0.3, 0.3, (H, W))).astype(F)
    d[rng.random((H, W)) < invalid] = INV
    return d


def blobs(H, W, seed=0):
    """patches of a few levels with pin-holes: segments of many sizes, holes of many widths"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 4, ((H + 5) // 6, (W + 8) // 9)).astype(F) * F(4)
    d = np.kron(coarse, np.ones((6, 9), F))[:H, :W] + rng.uniform(-0.4, 0.4, (H, W)).astype(F)
    d = d.astype(F) + F(10)
    d[rng.random((H, W)) < 0.08] = INV
    d[rng.random((H, W)) < 0.02] = F(-3)
    return d


def gap_widths(width=3):
    """runs of width and width + 1 in rows and columns, runs at both line ends, |d1 - d2| of exactly 3 and the float below"""
    d = np.full((12 + 2 * width, 40 + 4 * width), F(6), F)
    w = width
    d[1, 3:3 + w] = INV                      # filled by the row pass
    d[3:3 + w + 1, 10 + w:10 + 2 * w + 1] = INV  # (w + 1) x (w + 1): neither pass
    d[3:3 + w, 25 + 2 * w:26 + 3 * w] = INV  # w high, w + 1 wide: the column pass
    d[5, 0:2] = INV                          # touches the line's start
    d[5, -2:] = INV                          # ... and its end
    d[0:2, 20 + 2 * w] = INV
    d[-2:, 20 + 2 * w] = INV
    d[8 + w, 2] = F(5)
    d[8 + w, 3:5] = INV
    d[8 + w, 5] = F(8)                       # |d1 - d2| = 3: min
    d[10 + w, 2] = F(5)
    d[10 + w, 3:5] = INV
    d[10 + w, 5] = np.nextafter(F(8), F(0))  # just below 3: the mean of the two
    return d, Config(1.0, 0, width, 0)


def gap_L():
    """a hole the column pass closes only because the row pass ran first"""
    d = np.full((14, 24), F(9), F)
    d[5, 10:16] = INV
    d[5:9, 10] = INV
    d[:, 12] += F(1)  # (so the fills differ by column)
    d[5, 12] = INV
    return d, Config(1.0, 0, 3, 0)


def gap_long(L, columns=False):
    """width 5000 on lines of L pixels: one line filled end to end, one with invalid ends, one all invalid"""
    d = _blank(4, L)
    d[0, 0], d[0, L - 1] = F(2), F(4)
    d[1, 1], d[1, L - 2] = F(7), F(20)
    d[3, :] = np.where(np.arange(L) % 7 == 3, F(5), INV)
    return (np.ascontiguousarray(d.T) if columns else d), Config(1.0, 0, 5000, 0)


MEAN_SIZES = (7, 8, 9, 15, 16)


def mean_case(H, W, seed=0):
    return random_map(H, W, seed), Config(1.0, 0, 0, 1)


def cases(tw=TILE_W, th=TILE_H):
    """name -> (map, Config): every case of the CPU and GPU tests"""
    out = {
        "golden": (golden_input(), Config()),
        "speckle straddle": speckle_straddle(20, tw, th),
        "serpentine kept": serpentine(),
        "serpentine removed": serpentine(extra=1),
        "comb kept": comb(),
        "comb removed": comb(extra=1),
        "constant 256": constant(),
        "checkerboard": checkerboard(),
        "sim edge": sim_edge(),
        "all invalid": (_blank(10, 70), Config(1.0, 5, 3, 1)),
        "1x1": (np.array([[4.0]], F), Config(1.0, 1, 3, 1)),
        "1x1 removed": (np.array([[4.0]], F), Config(1.0, 2, 3, 1)),
        "1x70": (blobs(1, 70, 1), Config(1.0, 3, 3, 1)),
        "70x1": (blobs(70, 1, 2), Config(1.0, 3, 3, 1)),
        "gap widths 3": gap_widths(3),
        "gap widths 1": gap_widths(1),
        "gap L": gap_L(),
        "blobs": (blobs(50, 150, 3), Config(1.0, 20, 3, 1)),
        "blobs sim 0": (blobs(21, 67, 4), Config(0.0, 2, 2, 1)),
        "mean two tiles": mean_case(2 * th + 1, 2 * tw + 1, 5),
        "mean one tile": mean_case(2 * th + 1, tw + 1, 6),
        "mean tall": mean_case(3 * th + 9, 8, 7),
    }
    for L in (63, 64, 65, 129):
        out[f"gap 5000 rows {L}"] = gap_long(L)
        out[f"gap 5000 columns {L}"] = gap_long(L, True)
    for i, H in enumerate(MEAN_SIZES):
        for j, W in enumerate(MEAN_SIZES):
            out[f"mean {H}x{W}"] = mean_case(H, W, 10 + 5 * i + j)
    return out


def statement(name):
    """np_dfilter.stages of a case, cached"""
    if name not in _cache:
        d, cfg = cases()[name]
        st = np_dfilter.stages(d, cfg)
        for v in st.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = st
    return _cache[name]


def first_difference(got, want):
    """'' when the maps are equal bit for bit, else where they first differ"""
    a, b = np.ascontiguousarray(got, F).view(np.uint32), np.ascontiguousarray(want, F).view(np.uint32)
    if a.shape != b.shape:
        return f"shape {a.shape} != {b.shape}"
    bad = np.argwhere(a != b)
    if not len(bad):
        return ""
    v, u = bad[0]
    return f"{len(bad)} pixels differ, first at ({v}, {u}): {got[v, u]!r} != {want[v, u]!r}"


def refusals():
    """(what, map, config, code name)"""
    ok = np.full((5, 6), F(3), F)
    nan, inf, near = ok.copy(), ok.copy(), ok.copy()
    nan[2, 2], inf[1, 1], near[3, 3] = np.nan, np.inf, F(-1)
    return [("sim nan", ok, Config(float("nan")), "INVALID"), ("sim inf", ok, Config(float("inf")), "INVALID"), ("sim < 0", ok, Config(-0.5), "INVALID"),
            ("speckle_size < 0", ok, Config(1.0, -1), "INVALID"), ("ipol_gap_width < 0", ok, Config(1.0, 200, -1), "INVALID"),
            ("nan", nan, Config(), "INVALID"), ("inf", inf, Config(), "INVALID"), ("negative within sim", near, Config(), "INVALID")]
