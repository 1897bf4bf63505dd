"""Synthetic LiDAR scans the LiDAR tests share (CPU twin and device) and the numpy statement's results on them, computed once
per process and left unchanged.  Nothing is read from a file.

A generator casts n_scan rings of horizon_scan azimuth steps from the origin at a ground plane, a box of walls, pillars and
small clutter, in upstream's axes (x = -raw.y, y = -raw.z, z = raw.x).  Ring r sweeps the azimuth from just above 0 to just
below 360 degrees, so that the scan has exactly one 4 -> 1 quadrant transition between two rings; step s of a ring lies
within +-0.4 of column (s + H / 2) % H.  The returns are then edited per case, in the (ring, step) image."""
import functools

import numpy as np

import np_lidar
from unified_cvo_amd import LidarConfig, LidarScan

SENSOR_HEIGHT = 1.73
ELEV_LO, ELEV_HI = -24.8, 2.0
SMALL = dict(R=16, H=256)


class Image:
    """Returns of a scan by (ring, step): range `t` (NaN: no return) and intensity along the ray directions `d` (raw axes);
    `extra[(ring, step)]`: further returns of that step, after the first; `drop_rings`: rings that emit no point;
    `rings` may exceed R (a scan with more rings than the image has rows)."""

    def __init__(self, R, H, seed, rings=None, half=(12.0, 9.0)):
        rings = R if rings is None else rings
        g = np.random.default_rng(seed)
        self.R, self.H, self.rings = R, H, rings
        step = (ELEV_HI - ELEV_LO) / (max(R, 2) - 1)
        self.elev_step = step
        elev = np.radians(ELEV_LO + step * np.arange(rings))[:, None]
        jitter = g.uniform(-0.4, 0.4, (rings, H))
        jitter[:, 0] = g.uniform(0.05, 0.4, rings)
        theta = np.radians((np.arange(H)[None, :] + jitter) * (360.0 / H))
        self.d = np.stack([np.cos(elev) * np.cos(theta), np.cos(elev) * np.sin(theta), np.sin(elev) * np.ones_like(theta)], -1)
        self.t, self.inten = self._cast(g, half)
        self.extra = {}
        self.drop_rings = set()
        self.override = {}  # (ring, step) -> (x, y, z) float32 in upstream's axes, replacing the cast point

    def _cast(self, g, half):
        d = self.d
        with np.errstate(divide="ignore", invalid="ignore"):
            tg = np.where(d[..., 2] < 0, -SENSOR_HEIGHT / d[..., 2], np.inf)
            tw = np.minimum(np.where(d[..., 0] != 0, half[0] / np.abs(d[..., 0]), np.inf), np.where(d[..., 1] != 0, half[1] / np.abs(d[..., 1]), np.inf))
        t = np.minimum(tg, tw)
        hit = tg <= tw
        px, py, pz = (t * d[..., k] for k in range(3))
        inten = np.where(hit, 0.2 + 0.5 * ((np.floor(px) + np.floor(py)) % 2), 0.3 + 0.6 * ((np.floor(pz * 2) + np.floor((px + py) / 3)) % 2))
        # pillars (vertical cylinders) and clutter (spheres on the ground)
        for cx, cy, rad in ((5.0, 3.0, 0.4), (-4.0, 5.0, 0.5), (6.0, -4.0, 0.3), (-7.0, -3.5, 0.6), (2.5, -6.0, 0.35)):
            a = d[..., 0] ** 2 + d[..., 1] ** 2
            b = -(d[..., 0] * cx + d[..., 1] * cy)
            disc = b * b - a * (cx * cx + cy * cy - rad * rad)
            with np.errstate(invalid="ignore"):
                tp = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
            tp = np.where(tp > 0, tp, np.inf)
            near = tp < t
            t, inten = np.where(near, tp, t), np.where(near, 0.95, inten)
        for _ in range(12):
            cx, cy, rad = g.uniform(-9, 9), g.uniform(-7, 7), g.uniform(0.15, 0.4)
            if cx * cx + cy * cy < 4:
                continue
            c = np.array([cx, cy, -SENSOR_HEIGHT + rad])
            b = -(d @ c)
            disc = b * b - (c @ c - rad * rad)
            tp = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), np.inf)
            tp = np.where(tp > 0, tp, np.inf)
            near = tp < t
            t, inten = np.where(near, tp, t), np.where(near, 0.7, inten)
        return t, inten

    def col_step(self, col):
        return (col - self.H // 2) % self.H

    def carve(self, rows, cols):
        """No return in the given rows and columns (columns modulo H)."""
        for r in rows:
            for c in cols:
                self.t[r, self.col_step(c % self.H)] = np.nan

    def put(self, cells, rng, exact=False):
        """A return at `rng` in every (row, col) of `cells`; `exact`: the float32 range of the point IS rng (found by nudging z)."""
        for r, c in cells:
            s = self.col_step(c % self.H)
            self.t[r, s] = rng
            if exact:
                self.override[(r, s)] = self._snap(self.d[r, s], rng)

    @staticmethod
    def _snap(d, rng):
        raw = d * (rng / np.linalg.norm(d))
        p = np.array([-raw[1], -raw[2], raw[0]], np.float32)
        big = int(np.argmax(np.abs(p)))
        for k in range(64):
            q = p.copy()
            for _ in range(k // 2 + k % 2):
                q[big] = np.nextafter(q[big], np.float32(np.inf if k % 2 else -np.inf), dtype=np.float32)
            if np_lidar.frange(q[0:1], q[1:2], q[2:3])[0] == np.float32(rng):
                return q
        raise AssertionError("no float32 point of that range near the ray")

    def points(self):
        """-> xyzi (n, 4) float32 in scan order and, per point, its (ring, step)."""
        if not self.extra and not self.override:  # one return per step at the most: the same points without the loop
            hit = ~np.isnan(self.t)
            hit[sorted(self.drop_rings)] = False
            raw = self.d[hit] * self.t[hit][:, None]
            xyzi = np.stack([-raw[:, 1], -raw[:, 2], raw[:, 0], self.inten[hit]], -1).astype(np.float32)
            return xyzi, list(zip(*(a.tolist() for a in np.nonzero(hit))))
        out, where = [], []
        for r in range(self.rings):
            if r in self.drop_rings:
                continue
            for s in range(self.H):
                returns = ([] if np.isnan(self.t[r, s]) else [self.t[r, s]]) + self.extra.get((r, s), [])
                for k, t in enumerate(returns):
                    if k == 0 and (r, s) in self.override:
                        x, y, z = self.override[(r, s)]
                    else:
                        raw = self.d[r, s] * t
                        x, y, z = -raw[1], -raw[2], raw[0]
                    out.append((x, y, z, self.inten[r, s]))
                    where.append((r, s))
        return np.array(out, np.float32), where


def small_config(**kw):
    f = dict(n_scan=SMALL["R"], horizon_scan=SMALL["H"], ang_res_x=360.0 / SMALL["H"], ground_scan_ind=12,
             segment_alpha_x=float(np.radians(360.0 / SMALL["H"])), segment_alpha_y=float(np.radians((ELEV_HI - ELEV_LO) / (SMALL["R"] - 1))), beam_num=SMALL["R"])
    semantic = kw.pop("semantic", False)
    f.update(kw)
    return LidarConfig(semantic=semantic, **f)


TOP = SMALL["R"] - 1  # the top ring of the small image: above every ground row
BLOB_ROWS = (13, 14, 15)


def _blob(cells, rng=6.0, seed=3):
    """The small room with the cells (row, col) of an isolated blob: rows 12 .. 15 are empty around it."""
    im = Image(seed=seed, **SMALL)
    cols = [c for _, c in cells]
    im.carve(range(12, 16), range(min(cols) - 3, max(cols) + 4))
    im.put(cells, rng)
    return im


def _flat_top(seed=5):
    """The small room whose top ring is a cylinder of range exactly 8: curvature exactly 0 all around it."""
    im = Image(seed=seed, **SMALL)
    im.put([(TOP, c) for c in range(SMALL["H"])], 8.0, exact=True)
    return im


def _top_positions(im, cfg):
    """Sixths of the top ring and the column of every segmented position, from the statement on the image as it is."""
    xyzi, _ = im.points()
    st = np_lidar.select(xyzi, cfg, np_lidar.Rand(1))
    H = cfg.horizon_scan
    return [s for s in st["sixths"] if s[0] == TOP], {k: c % H for k, c in enumerate(st["seg_cell"]) if c // H == TOP}


def _build(name):
    """-> (Image, config, semantic or None, num_classes)"""
    sem, nc = None, 0
    cfg = small_config()
    if name == "room16":
        im = Image(seed=1, **SMALL)
    elif name == "hdl64":
        cfg = LidarConfig()
        im = Image(64, 1800, seed=2, half=(20.0, 15.0))
        _pilasters(im, 60)
    elif name == "cap":  # four rings of 1800 columns: a sixth with more than 20 edge candidates
        cfg = LidarConfig(n_scan=4, ground_scan_ind=0, beam_num=4)
        im = Image(4, 1800, seed=2, half=(20.0, 15.0))
        _pilasters(im, 3, range(1800))
    elif name == "seam":
        H = SMALL["H"]
        im = Image(seed=3, **SMALL)
        im.carve(range(12, 16), range(H - 5, H + 5))
        im.put([(r, c % H) for r in BLOB_ROWS for c in (H - 2, H - 1, H, H + 1)], 6.0)
    elif name == "size4":
        im = _blob([(13, 200), (13, 201), (14, 200), (14, 201)])
    elif name == "size5_valid":  # two non-seed cells in the seed's row: rows 13, 14, 15 count
        im = _blob([(13, 200), (13, 201), (13, 202), (14, 201), (15, 201)])
    elif name == "size5_seed_alone":  # the seed alone in its row: rows 14, 15 count, invalid
        im = _blob([(13, 201), (14, 201), (14, 202), (15, 201), (15, 202)])
    elif name == "size29":
        im = _blob([(13, c) for c in range(190, 205)] + [(14, c) for c in range(190, 204)])
    elif name == "size30":
        im = _blob([(14, c) for c in range(185, 215)])
    elif name == "collide":
        im = Image(seed=6, **SMALL)
        for r, s, ts in ((3, 40, [2.0, 3.5]), (9, 100, [7.0]), (14, 30, [0.5]), (14, 31, [5.0, 0.4]), (15, 200, [6.0, 6.5, 7.0])):
            im.extra[(r, s)] = ts
        for r, s in ((2, 10), (7, 77), (15, 128)):
            im.t[r, s] = 0.5  # under sensor_min_range: the cell stays empty
    elif name == "extra_rings":
        im = Image(seed=7, rings=SMALL["R"] + 3, **SMALL)
    elif name == "thin_ring":
        im = Image(seed=8, **SMALL)
        keep = set(range(100, 108)) | {0, SMALL["H"] - 1}
        for s in range(SMALL["H"]):
            if s not in keep:
                im.t[14, s] = np.nan
        im.drop_rings.add(15)
    elif name == "ties":
        im = _flat_top()
        im.put([(TOP, 188), (TOP, 203)], 8.0625, exact=True)
    elif name == "spill":
        im = _flat_top()
        sixths, col_of = _top_positions(im, cfg)
        ep = sixths[2][3]
        im.put([(TOP, col_of[ep - 2])], 8.125, exact=True)
        im.put([(TOP, col_of[ep + 2])], 8.0625, exact=True)
    elif name == "semantic":
        cfg = small_config(semantic=True)
        im = Image(seed=9, **SMALL)
        nc = 5
    elif name == "dark":
        im = Image(seed=10, **SMALL)
        g = np.random.default_rng(10)
        im.inten[g.random(im.inten.shape) < 0.05] = 0.0
    elif name in EDGE_CASES:
        im, cfg = _build_edge(name)
    else:
        raise KeyError(name)
    return im, cfg, sem, nc


def _pilasters(im, ring, steps=range(300, 940)):
    """A far wall with a 7 cm step every 12 columns over `steps` of `ring`: two edge candidates per step, steps farther
    apart than the suppression reaches, so a sixth (about 300 points) holds more than 20."""
    for s in steps:
        im.t[ring, s] = 40.0 + 0.07 * ((s // 12) % 2)


CASES = ("room16", "hdl64", "cap", "seam", "size4", "size5_valid", "size5_seed_alone", "size29", "size30", "collide", "extra_rings",
         "thin_ring", "ties", "spill", "semantic", "dark")
SMALL_CASES = tuple(c for c in CASES if c not in ("hdl64", "cap"))


# ---- Scans drawn for the kernels' structure, not for the algorithm's branches ("structural classes"):
# the sort sizes of k_lidar_pick, the four words of a component's row mask, the block / wave / lane boundaries of
# k_lidar_project's ring id, the merge orders of k_lidar_union, the empty results of the device route and the validator's
# limits.  A result may be empty here, so these are not in CASES.

def config_for(R, H, **kw):
    """A config for an R x H image of this generator: the angular steps of the image, one beam per row."""
    f = dict(n_scan=R, horizon_scan=H, ang_res_x=360.0 / H, segment_alpha_x=float(np.radians(360.0 / H)),
             segment_alpha_y=float(np.radians((ELEV_HI - ELEV_LO) / (max(R, 2) - 1))), beam_num=R, ground_scan_ind=0)
    f.update(kw)
    return LidarConfig(**f)


WIDE = {"wide700": 700, "wide1200": 1200, "wide2400": 2400, "wide4096": 4096}  # four rings, no ground rows: sixths of H / 6 entries
SKIP = {"skip%d" % d: d for d in (1, 2, 63, 65, 191, 193, 255)}  # room16 without its first d points: ring k starts at 256 k - d
LAST_OPENS = 15 * SMALL["H"] + 1  # room16 cut after the first point of ring 15
LONE_RING = 7  # one_point_ring: the ring that keeps one cell

# tall128's blobs, (row, col) cells with the seed (the lowest row-major cell) first -> (size, valid).  A component's rows are
# counted without its seed and sit in word row / 32 of the mask: three rows or more make a small component valid.
TALL_BLOBS = (
    (((31, 100), (31, 101), (32, 100), (33, 100), (33, 101)), True),     # rows 31 | 32, 33: words 0 and 1
    (((63, 140), (64, 140), (64, 141), (65, 140), (65, 141)), False),    # the seed alone in row 63: rows 64, 65 count
    (((63, 180), (63, 181), (64, 180), (65, 180), (65, 181)), True),     # row 63 in word 1, rows 64, 65 in word 2
    (((95, 60), (95, 61), (96, 60), (97, 60), (97, 61)), True),          # rows 95 | 96, 97: words 2 and 3
    (tuple((r, c) for r in (126, 127) for c in (20, 21, 22)), False),    # six cells, two rows of word 3
    (((125, 220), (125, 221), (126, 220), (127, 220), (127, 221)), True),  # three rows of word 3, the image's last row
)
SHAPES = {  # name -> (seed cell, size): one valid component each
    "serpent": ((13, 130), 243),  # two long rows joined at their far end: the trees of both rows merge last
    "comb": ((12, 130), 304),     # a spine below 61 teeth: every tooth is a tree of its own until the spine's row
    "loop": ((14, 0), 256),       # a full row: closes through the column seam
}
ALONE = {"blob30_alone": [(14, c) for c in range(185, 215)], "blob11_alone": [(14, c) for c in range(185, 196)],
         "blob5_alone": [(13, 200), (13, 201), (13, 202), (14, 201), (15, 201)]}

EDGE_CASES = (tuple(WIDE) + ("tall128", "tall128_ground") + tuple(SKIP) + ("last_opens", "one_point_ring") + tuple(SHAPES) +
              ("n1", "n3", "all_near") + tuple(ALONE) + ("R1", "w255", "w257", "max"))


def _keep_ring_ends(im, rows, H):
    """Carve whole rows but for a ring's first and last step (columns H / 2 and H / 2 - 1): the 4 -> 1 transitions stay, and
    with them the ring id of every later point."""
    im.carve(rows, [c for c in range(H) if c not in (H // 2 - 1, H // 2)])


def _build_edge(name):
    """-> (Image, config)"""
    R, H = SMALL["R"], SMALL["H"]
    cfg = small_config()
    if name in WIDE:
        im = Image(4, WIDE[name], seed=2, half=(20.0, 15.0))
        cfg = config_for(4, WIDE[name], ground_scan_ind=0)
        if name == "wide4096":  # at 100 m adjacent columns of a 4096-wide image are connected, at _pilasters' 40 m they are not
            for s in range(4096):
                im.t[3, s] = 100.0 + 0.07 * ((s // 12) % 2)
    elif name in ("tall128", "tall128_ground"):
        im = Image(128, H, seed=4)
        cfg = config_for(128, H, ground_scan_ind=20 if name == "tall128" else 127)
        for cells, _ in TALL_BLOBS:
            rows, cols = [r for r, _ in cells], [c for _, c in cells]
            im.carve(range(max(min(rows) - 2, 0), min(max(rows) + 3, 128)), range(min(cols) - 3, max(cols) + 4))
        for cells, _ in TALL_BLOBS:
            im.put(cells, 6.0)
    elif name in SKIP or name in ("last_opens", "n1", "n3", "all_near"):
        im = Image(seed=1, **SMALL)  # room16; case() cuts or scales its points
    elif name == "one_point_ring":
        # Two transitions cannot be adjacent (a point is not in quadrants 4 and 1), so a ring between two others has at least
        # two points, its first and its last step; the last one here is under sensor_min_range: the ring holds one cell.
        # (A ring of one point by its id is the first of skip255 and the last of last_opens.)
        im = Image(seed=1, **SMALL)
        for s in range(1, H - 1):
            im.t[LONE_RING, s] = np.nan
        im.t[LONE_RING, H - 1] = 0.5
    elif name in SHAPES:
        im = Image(seed=3, **SMALL)
        _keep_ring_ends(im, range(11 if name == "comb" else 12, 16), H)
        if name == "serpent":
            im.put([(r, c) for r in (13, 15) for c in range(130, 251)] + [(14, 250)], 6.0)
        elif name == "comb":
            cfg = small_config(ground_scan_ind=8)
            im.put([(15, c) for c in range(130, 251)] + [(r, c) for r in (12, 13, 14) for c in range(130, 251, 2)], 6.0)
        else:
            im.put([(14, c) for c in range(H)], 6.0)
    elif name in ALONE:
        # nothing but the blob holds a cell: every ring keeps its first and last step for the ring ids, under sensor_min_range
        im = Image(seed=3, **SMALL)
        im.t[:, :] = np.nan
        im.t[:, 0] = im.t[:, H - 1] = 0.5
        im.put(ALONE[name], 6.0)
    elif name == "R1":
        im = Image(1, H, seed=12)
        cfg = config_for(1, H, ground_scan_ind=0)
    elif name in ("w255", "w257"):
        W = int(name[1:])
        im = Image(R, W, seed=13)
        cfg = config_for(R, W, ground_scan_ind=12)
    elif name == "max":  # the largest image the validator admits
        im = Image(128, 4096, seed=8, half=(20.0, 15.0))
        cfg = config_for(128, 4096, ground_scan_ind=100)
    else:
        raise KeyError(name)
    return im, cfg


def _cut(name, xyzi):
    """The edge cases that edit the point list rather than the image."""
    if name in SKIP:
        return xyzi[SKIP[name]:]
    if name == "last_opens":
        return xyzi[:LAST_OPENS]
    if name in ("n1", "n3"):
        return xyzi[:int(name[1:])]
    if name == "all_near":  # every point under sensor_min_range; the intensities stay
        return xyzi * np.array([0.01, 0.01, 0.01, 1.0], np.float32)
    return xyzi


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (LidarScan, LidarConfig)"""
    im, cfg, sem, nc = _build(name)
    xyzi, where = im.points()
    if name in EDGE_CASES:
        xyzi = _cut(name, xyzi)
    if name == "semantic":
        g = np.random.default_rng(11)
        sem = g.integers(0, nc, len(xyzi)).astype(np.int32)
        sem[g.random(len(xyzi)) < 0.1] = -1
        starts = [i for i, (r, s) in enumerate(where) if s == 0]
        sem[starts[1::2]] = -1  # at ring starts: the transition point itself is skipped before its quadrant is looked at
    if name == "dark":
        for i, (r, s) in enumerate(where):
            if s == SMALL["H"] // 2 and r % 3 == 0:
                xyzi[i, 0] = 0.0
            if s == 50 and r >= 13:
                xyzi[i, 1] = 0.0
            if s == 70 and r % 4 == 1:
                xyzi[i, 2] = 0.0
    return LidarScan(xyzi, sem, nc), cfg


@functools.lru_cache(maxsize=None)
def statement(name, seed=1, no_spill=False):
    scan, cfg = case(name)
    return np_lidar.select(scan.xyzi, cfg, np_lidar.Rand(seed), scan.semantic, no_spill)


def component_of(st, cfg, row, col):
    cell = row * cfg.horizon_scan + col
    for c in st["comps"]:
        if cell in c["cells"]:
            return c
    return None


COUNTS = ("projected", "ground", "valid", "invalid", "segmented", "edges", "draws", "thinned", "edge_detected")  # debug_lidar_stats and the statement


def same_resident(gpu, d, want_cloud):
    """The resident cloud `d` orders as an ordinary upload of `want_cloud` does."""
    u = gpu.upload(want_cloud)
    try:
        assert d.n == u.n and np.array_equal(d.debug_order(), u.debug_order())
    finally:
        u.free()
