"""Score cases whose TILES are chosen: every structural edge of k_overlap (cvo_k_overlap.h) met on purpose.

Under NO_SORT=1 a cloud's tiles are its rows 64 t .. 64 t + 63 in original order, so a case decides which points share a
tile, where a tile's bounding sphere and box lie, how many pairs a row tile finds in a target tile and in which lanes.
A case is (params, source arrays, target arrays, pose 4x4 float32, ell).  Its float64 statement (`statement`) is the sum of
np_reference.kernel_matrix over y' = R^T (y - T) - the convention of np_reference.iteration, whatever matrix R is - and
comes with the pairs, the largest row count, the smallest relative distance of any pair from any gate it meets, the
smallest pair value and the geometric candidates (d^2 below the row's cut-off: what k_overlap parks in its pair list before
the features drop some).  tests/test_overlap_cases_cpu.py asserts on every case what keeps the GPU test from hiding a
failure (margin, visibility, no truncation, the intended limit); tests/test_gpu_overlap_edges.py runs them.

Lengths are in units of r = ell * cutoff_factor(P), the geometric cut-off radius of a row at the origin; a row's own radius
is (|x| / 500 + 1) r, which the statement uses and the margins absorb.

How far the rows in reach are spread.  A row in reach of a target cluster sits 0.1 r .. 0.9 r from it, so that its values
differ from its neighbours' - as far as visibility allows: one dropped pair has to move the sum by 100 tolerances, i.e.
(smallest pair value) / sum > 2e-4 (geometry) or 1.22e-4 (featured).  With sigma = 0.1 and sp_thres = 6e-4 the kernel falls
from 0.01 to 6e-4 over 0 .. r, a factor 9.5 over 0.1 r .. 0.9 r: about 1000 pairs can be spread that far (uniformly in
d^2: mean / smallest = 3.8), 2048 pairs over 0.1 r .. 0.5 r, 4096 pairs over 0.1 r .. 0.3 r (mean / smallest = 1.12,
1 / (4096 x 1.12) = 2.2e-4).  The `hot` settings of row_classes.FEATURE_SETTINGS have sigma = 3: the kernel falls by
1.5e4 over 0 .. r, and the rows in reach sit at 0.4 r .. 0.5 r (0.1 r .. 0.4 r without a satellite target).  With the colour
kernel (c_sigma^2 = 0.36 at best) the product falls below sp_thres from 0.75 r on: the colour layouts stop at 0.67 r.
"""
import math

import numpy as np

import cases
import np_reference as npr
import row_classes as rcl
from unified_cvo_amd import CvoPointCloud

ELL = 0.3
OV_QCAP = 1024       # cvo_k_overlap.h: pairs a wave's list holds
OV_LIST_CAP = 1024   # target tiles a block lists per round
OV_PASS = 512        # target tiles a block tests per pass (64 * OV_WAVES threads)
OFFSET = np.array([800.0, -300.0, 150.0])  # the far-from-origin cases (test_overlap_kernel_equals_the_list_chain's)
CLASS_A, CLASS_B = 3, 11


class Case:
    def __init__(self, name, P, src, tgt, T=None, ell=ELL, fsrc=None, ftgt=None, lsrc=None, ltgt=None, tol="geo", limit=None,
                 void=False, tags=()):
        self.name, self.P, self.ell = name, P, float(ell)
        self.src = np.ascontiguousarray(src, np.float32).reshape(-1, 3)
        self.tgt = np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
        self.T = np.eye(4, dtype=np.float32) if T is None else np.asarray(T, np.float32).reshape(4, 4)
        self.fsrc, self.ftgt, self.lsrc, self.ltgt = fsrc, ftgt, lsrc, ltgt
        self.tol = tol        # "geo" | "featured" | "far": which bound against float64 the GPU test uses
        self.limit = limit or {}  # the structural limit the case was built for (test_overlap_cases_cpu.py asserts it)
        self.void = void      # some row has more than K pairs: k_overlap is void, the list chain answers
        self.tags = tuple(tags)
        self._st = None

    @property
    def N(self):
        return self.src.shape[0]

    @property
    def M(self):
        return self.tgt.shape[0]

    def clouds(self):
        if self.fsrc is None and self.lsrc is None:
            return CvoPointCloud.from_xyz(self.src), CvoPointCloud.from_xyz(self.tgt)
        geo = lambda n: np.tile(np.array([[0.0, 1.0]], np.float32), (n, 1))
        return (CvoPointCloud.from_arrays(self.src, self.fsrc, self.lsrc, geo(self.N)),
                CvoPointCloud.from_arrays(self.tgt, self.ftgt, self.ltgt, geo(self.M)))

    def statement(self):
        if self._st is None:
            self._st = statement(self)
        return self._st

    def __repr__(self):
        return self.name


def radius(P, ell=ELL):
    return ell * rcl.cutoff_factor(P)


def moved_targets(case):
    """y' = R^T (y - T), float64, of the float32 inputs."""
    R, t = case.T[:3, :3].astype(np.float64), case.T[:3, 3].astype(np.float64)
    return (case.tgt.astype(np.float64) - t) @ R


def statement(case, slab=4096):
    """dict(total, pairs (i, j arrays), widest, margin, min_value, cand (i, j arrays), nearest: the two smallest d / r_i of
    all cross pairs, max_term: the largest |term| of R^T y - R^T T and of x).  Target slabs of `slab` columns (N = 64 x
    M = 65 599 as one dense matrix would be 100 MB per intermediate); with a row beyond K (the void case) the first-K
    truncation needs the whole row, and the matrix is taken in one piece."""
    P, ell = case.P, case.ell
    x = case.src.astype(np.float64)
    yp = moved_targets(case)
    K = int(P.nearest_neighbors_max)
    sp, s2 = float(np.float32(P.sp_thres)), float(np.float32(P.sigma)) ** 2
    l = rcl.range_ell(x, ell)
    thr = -2.0 * l * l * math.log(sp / s2)
    geo = lambda n: np.tile(np.array([[0.0, 1.0]], np.float32), (n, 1))
    if case.void:
        slab = case.M
    total, margin, min_value = 0.0, np.inf, np.inf
    counts = np.zeros(case.N, np.int64)
    pi, pj, ci, cj, near = [], [], [], [], [np.full(2, np.inf)]
    for c0 in range(0, case.M, slab):
        cols = slice(c0, min(case.M, c0 + slab))
        sl = lambda a: None if a is None else a[cols]
        A, keep = npr.kernel_matrix(P, x, yp[cols], case.fsrc, sl(case.ftgt), case.lsrc, sl(case.ltgt), geo(case.N),
                                    geo(yp[cols].shape[0]), K if case.void else case.M + 1, ell)
        total += float(A.sum())
        counts += keep.sum(1)
        i, j = np.nonzero(keep)
        pi.append(i)
        pj.append(j + c0)
        if len(i):
            min_value = min(min_value, float(A[i, j].min()))
        # the gates, restated: distance of every pair from each one it MEETS (a pair a gate rejects meets no later one)
        d2 = ((x[:, None, :] - yp[None, cols, :]) ** 2).sum(-1)
        alive = d2 < thr[:, None]
        m = np.abs(d2 - thr[:, None]) / thr[:, None]
        a = s2 * np.exp(-d2 / (2.0 * l[:, None] ** 2))
        i, j = np.nonzero(alive)
        ci.append(i)
        cj.append(j + c0)
        near.append(np.sort((np.sqrt(d2) / np.sqrt(thr)[:, None]).reshape(-1))[:2])
        if P.is_using_intensity:
            c2, cs2 = float(np.float32(P.c_ell)) ** 2, float(np.float32(P.c_sigma)) ** 2
            d2c = ((case.fsrc.astype(np.float64)[:, None, :] - case.ftgt.astype(np.float64)[None, cols, :]) ** 2).sum(-1)
            tc = -2.0 * c2 * math.log(sp / cs2)
            m = np.where(alive, np.minimum(m, np.abs(d2c - tc) / tc), m)
            alive = alive & (d2c < tc)
            a = a * cs2 * np.exp(-d2c / (2.0 * c2))
        if P.is_using_semantics:
            se2, ss2 = float(np.float32(P.s_ell)) ** 2, float(np.float32(P.s_sigma)) ** 2
            d2s = ((case.lsrc.astype(np.float64)[:, None, :] - case.ltgt.astype(np.float64)[None, cols, :]) ** 2).sum(-1)
            ts = -2.0 * se2 * math.log(sp / ss2)
            m = np.where(alive, np.minimum(m, np.abs(d2s - ts) / ts), m)
            alive = alive & (d2s < ts)
            a = a * ss2 * np.exp(-d2s / (2.0 * se2))
        m = np.where(alive, np.minimum(m, np.abs(a - sp) / sp), m)
        if not case.void:
            assert np.array_equal(alive & (a > sp), keep), case.name  # (the restated gates decide what the reference decides)
        margin = min(margin, float(m.min()))
    R, t = case.T[:3, :3].astype(np.float64), case.T[:3, 3].astype(np.float64)
    terms = np.abs(case.tgt.astype(np.float64))[:, None, :] * np.abs(R.T)[None, :, :]   # |Rinv_kc y_c|
    max_term = max(float(terms.max()), float(np.abs(R.T * t[None, :]).max()), float(np.abs(x).max()))
    return dict(total=total, pairs=(np.concatenate(pi), np.concatenate(pj)), widest=int(counts.max()), margin=margin,
                min_value=min_value, cand=(np.concatenate(ci), np.concatenate(cj)), nearest=np.sort(np.concatenate(near))[:2],
                max_term=max_term, counts=counts)


def tile_pair_counts(ij, n_xtiles, n_ytiles):
    """[row tile, target tile] counts of a pair list (i, j)."""
    out = np.zeros((n_xtiles, n_ytiles), np.int64)
    np.add.at(out, (ij[0] // 64, ij[1] // 64), 1)
    return out


# ---- parameters ---------------------------------------------------------------------------------------------------------
def params(feature=None, K=512):
    """feature None: configs/geometric_gpu.yaml; 'colour': configs/intensity_gpu.yaml (colour features that all pass);
    'hot': row_classes.FEATURE_SETTINGS['hot'] on the geometric configuration (one-hot classes, another class rejected)."""
    if feature == "hot":
        P = rcl.feature_params(cases.load_params("geometric_gpu"), "hot")
    else:
        P = cases.load_params("intensity_gpu" if feature == "colour" else "geometric_gpu")
    P.nearest_neighbors_max = int(K)
    return P


def _features(feature, n, m, seed):
    """colour: 5 channels within 0.02 of one colour (the colour kernel keeps every geometric hit: row_classes.build);
    hot: classes alternating between neighbouring rows and between neighbouring targets."""
    out = dict(fsrc=None, ftgt=None, lsrc=None, ltgt=None)
    if feature == "colour":
        rs = np.random.default_rng([seed, 5])
        base = np.array([0.5, 0.4, 0.6, 0.45, 0.55], np.float32)
        out["fsrc"] = (base + rs.uniform(-0.02, 0.02, (n, rcl.FD))).astype(np.float32)
        out["ftgt"] = (base + rs.uniform(-0.02, 0.02, (m, rcl.FD))).astype(np.float32)
    elif feature == "hot":
        for key, k in (("lsrc", n), ("ltgt", m)):
            lab = np.zeros((k, rcl.NC), np.float32)
            lab[np.arange(k), np.where(np.arange(k) % 2 == 0, CLASS_A, CLASS_B)] = 1.0
            out[key] = lab
    return out


def _dirs(rs, n):
    d = rs.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _ball(rs, n, rad):
    return _dirs(rs, n) * (rad * rs.random(n) ** (1.0 / 3.0))[:, None]


# ---- the parked-pair list -------------------------------------------------------------------------------------------------
SPREAD_ROWS = (0, 5, 10, 15, 16, 17, 30, 31, 33, 40, 41, 47, 48, 50, 60, 63)  # 16 rows, four in every quarter of the wave
QUEUE_LAYOUTS = ("1024", "1025", "4096", "quarters", "alternate")
QUEUE_FEATURES = (None, "colour", "hot")


def queue_case(layout, feature=None, K=512, seed=11):
    """One row tile against one target tile, its geometric candidates on a limit of the parked-pair list (OV_QCAP = 1024):
      1024       16 rows (SPREAD_ROWS) in reach of all 64 targets, 48 rows of nothing: the list's capacity, one group;
      1025       the same and row 20 in reach of ONE target (a satellite 0.5 r from the other 63): four quarters;
      4096       every row in reach of every target;
      quarters   1024 / 1 / 0 / 37: rows 0 .. 15 in reach of all, row 21 of one target, row 55 of 37;
      alternate  even rows in reach of all 64 targets, odd rows of none: consecutive lanes alternate between 0 and 64.
    Rows of nothing lie 6 r and more away.  `limit`: candidates of the tile pair, per quarter of the wave."""
    P = params(feature, K)
    steep = feature == "hot"  # sigma = 3: see the module docstring
    r = radius(P)
    rs = np.random.default_rng([seed, QUEUE_LAYOUTS.index(layout)])
    c = np.array([0.4, -0.3, 1.2])
    e = np.array([0.0, 0.0, 1.0])
    src = c + 6.0 * r * np.array([1.0, 0.0, 0.0]) + _ball(rs, 64, 0.5 * r) + np.arange(64)[:, None] * 0.05 * r  # nothing in reach
    tgt = c + _ball(rs, 64, 0.01 * r)
    ring = lambda n: np.stack([np.cos(a := rs.uniform(0, 2 * np.pi, n)), np.sin(a), np.zeros(n)], 1)
    if layout in ("1024", "1025"):
        # (rows in the plane through the cluster, perpendicular to the satellite's direction: rho from the cluster, sqrt(rho^2 +
        # sat^2) from the satellite - 0.1 r .. 0.87 r in all; steep: on the bisector plane, 0.4 r .. 0.5 r from both)
        sat, alpha, lone = (0.8, 0.4, 0.3) if steep else (0.5, 0.0, 0.6)
        rho = rs.permutation(np.linspace(0.0, 0.3, 16) if steep else np.sqrt(np.linspace(0.01, 0.2 if feature else 0.5, 16)))
        tgt[37] = c + sat * r * e
        src[list(SPREAD_ROWS)] = c + alpha * r * e + (rho * r)[:, None] * ring(16)
        if layout == "1025":
            src[20] = tgt[37] + lone * r * e
        quarters = [256, 256 + (layout == "1025"), 256, 256]
    elif layout in ("4096", "alternate"):
        rows = np.arange(64) if layout == "4096" else np.arange(0, 64, 2)
        hi = 0.3 if layout == "4096" else (0.4 if steep else 0.5)
        src[rows] = c + _dirs(rs, len(rows)) * (r * np.sqrt(rs.uniform(0.01, hi * hi, len(rows))))[:, None]
        quarters = [1024] * 4 if layout == "4096" else [512] * 4
    elif layout == "quarters":
        g, z_hi, beta = (0.35, 0.2, 0.5) if steep else (0.3, 0.6 if feature else 0.8, 0.6)
        corner = [np.array([np.cos(a), np.sin(a), 0.0]) for a in (0.0, 2 * np.pi / 3, 4 * np.pi / 3)]
        tgt[:37] = c + g * r * corner[0] + _ball(rs, 37, 0.01 * r)      # A
        tgt[37] = c + g * r * corner[1]                                  # the single target
        tgt[38:] = c + g * r * corner[2] + _ball(rs, 26, 0.01 * r)      # B
        src[:16] = c + (r * rs.uniform(0.0, z_hi, 16) * rs.choice([-1.0, 1.0], 16))[:, None] * e
        src[21] = c + (g + beta) * r * corner[1]
        src[55] = c + (g + beta) * r * corner[0]
        quarters = [1024, 1, 0, 37]
    else:
        raise KeyError(layout)
    name = f"queue-{layout}" + (f"-{feature}" if feature else "") + (f"-K{K}" if K != 512 else "")
    return Case(name, P, src, tgt, tol="featured" if feature else "geo", limit=dict(quarters=quarters),
                void=K < 64 and layout != "alternate", tags=("queue",), **_features(feature, 64, 64, seed))


BUSY_TILES = (8, 9)
CLASS_C = 7


def busy_queue_case(n_tiles, seed=16):
    """One row tile against n_tiles target tiles that EACH hold 4096 candidates: all 64 rows 0.1 r .. 0.3 r from one tight
    cluster of 64 n_tiles targets.  With 8 tiles every wave of the block is on a four-quarter tile at the same time - no
    wave's list is idle, a list that outgrew its 1024 entries would grow into one in use -, with 9 wave 0 goes on to a second
    one.  36 864 pairs could not be visible, so the one-hot classes (`hot`) keep few: rows alternate between two classes,
    and every tile holds ONE target of each of them, at a position of its own, among 62 of a third class; 64 pairs per
    tile, every one of them evaluated for a row of another lane."""
    P = params("hot")
    r = radius(P)
    rs = np.random.default_rng([seed, n_tiles])
    c = np.array([0.4, -0.3, 1.2])
    src = c + _dirs(rs, 64) * (r * np.sqrt(rs.uniform(0.01, 0.09, 64)))[:, None]
    M = 64 * n_tiles
    tgt = c + _ball(rs, M, 0.01 * r)
    f = _features("hot", 64, M, seed)
    cls = np.full(M, CLASS_C)
    for t in range(n_tiles):
        cls[64 * t + (5 * t + 3) % 64] = CLASS_A
        cls[64 * t + (11 * t + 40) % 64] = CLASS_B
    f["ltgt"] = np.zeros((M, rcl.NC), np.float32)
    f["ltgt"][np.arange(M), cls] = 1.0
    return Case(f"queue-busy-{n_tiles}", P, src, tgt, tol="featured", limit=dict(tiles=n_tiles, pairs=64 * n_tiles),
                tags=("busy",), **f)


# ---- partial tiles ----------------------------------------------------------------------------------------------------------
def partial_case(n, m, lone=None, seed=12):
    """N x M points in one tight cluster (radius 0.05 r): every pair a hit, at most 65 x 64.  lone='target': M = 65, targets
    0 .. 63 far away and target 64 - alone in tile 1 - the only one in reach of any row; lone='row': N = 65, row 64 the only
    row with pairs."""
    P = params()
    r = radius(P)
    rs = np.random.default_rng([seed, n, m, 0 if lone is None else 1])
    c = np.array([-0.5, 0.6, 1.0])
    far = c + np.array([0.0, 50.0 * r, 0.0])
    if lone is None:
        src, tgt = c + _ball(rs, n, 0.05 * r), c + _ball(rs, m, 0.05 * r)
        limit = dict(pairs=n * m)
    elif lone == "target":
        src = c + _dirs(rs, n) * (r * np.sqrt(rs.uniform(0.01, 0.81, n)))[:, None]
        tgt = np.concatenate([far + _ball(rs, m - 1, r), c[None]])
        limit = dict(pairs=n, only_target=m - 1)
    else:
        tgt = c + _dirs(rs, m) * (r * np.sqrt(rs.uniform(0.01, 0.81, m)))[:, None]
        src = np.concatenate([far + _ball(rs, n - 1, r), c[None]])
        limit = dict(pairs=m, only_row=n - 1)
    return Case(f"partial-{n}x{m}" + (f"-lone-{lone}" if lone else ""), P, src, tgt, limit=limit, tags=("partial",))


PARTIAL = [(1, 64), (63, 64), (64, 64), (65, 64), (64, 1), (64, 63), (64, 65)]


# ---- touching tiles -----------------------------------------------------------------------------------------------------------
def _rot(axis, angle):
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1.0 - math.cos(angle)) * Kx @ Kx


def _rot90(a):
    R = np.rint(_rot(np.eye(3)[a], math.pi / 2))
    return R


SHEAR = np.eye(3)
SHEAR[0, 0], SHEAR[1, 2] = 1.3, 0.2  # (test_overlap_kernel_equals_the_list_chain's matrix that is no rotation)
POSES = {
    "identity": (np.eye(3), (0.0, 0.0, 0.0)),
    "rot90x": (_rot90(0), (0.3, -0.2, 0.1)),
    "rot90y": (_rot90(1), (-0.1, 0.4, 0.2)),
    "rot90z": (_rot90(2), (0.2, 0.1, -0.3)),
    "generic": (_rot((1.0, -2.0, 0.5), 0.4), (0.3, 0.1, -0.2)),
    "reflection": (np.diag([1.0, -1.0, 1.0]), (0.1, 0.2, -0.1)),
    "stretch": (np.diag([2.0, 1.0, 0.5]), (0.2, -0.3, 0.1)),
    "shear": (SHEAR, (-0.2, 0.1, 0.3)),
    "far": (_rot((0.0, 0.0, 1.0), 0.05), None),  # offset OFFSET, the translation cancels the rotated coordinates
    "cyclic": (np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (0.1, -0.1, 0.2)),  # |R| is not symmetric
}
BALL_POSES = ("identity", "rot90x", "rot90y", "rot90z", "generic", "reflection", "stretch", "shear", "far")
THIN_POSES = ("rot90x", "rot90y", "rot90z", "generic", "cyclic")
S2, S3 = 1.0 / math.sqrt(2.0), 1.0 / math.sqrt(3.0)
DIRECTIONS = {"+x": (1, 0, 0), "-x": (-1, 0, 0), "+y": (0, 1, 0), "-y": (0, -1, 0), "+z": (0, 0, 1), "-z": (0, 0, -1),
              "xy": (S2, S2, 0), "y-z": (0, S2, -S2), "xyz": (S3, S3, S3), "-xy-z": (-S3, S3, -S3)}
THIN_DIRECTIONS = ("+x", "-y", "xyz")
PRINCIPAL = ("+principal", "-principal")
NON_ROTATIONS = ("stretch", "shear")
RHO = 5.0     # radius of a ball tile, in r
SEGMENT = 20.0  # length of a thin tile, in r
FS = (0.98, 1.02)


def _perp(u):
    a = np.eye(3)[int(np.argmin(np.abs(u)))]
    w = np.cross(u, a)
    return w / np.linalg.norm(w)


def _shape(rs, thin, tip, u, r):
    """64 points (in the source's frame) of a tile whose point 0.. is `tip`, which it reaches in direction u:
    a ball of radius RHO r centred RHO r behind the tip - its axis extremes among the points, so that the box's centre is the
    ball's and the sphere of the tile IS the ball - with nothing else in the cap within 1.5 r of the tip's plane; or a
    segment SEGMENT r long, perpendicular to u, with the tip at its end and the next point 2.5 r along."""
    if thin:
        w = _perp(u)
        t = np.concatenate([[0.0], np.sort(rs.uniform(2.5, SEGMENT, 62)), [SEGMENT]]) * r
        return tip + t[:, None] * w
    centre = tip - RHO * r * u
    pts = [tip]
    for a in range(3):
        for s in (-1.0, 1.0):
            p = centre + s * RHO * r * np.eye(3)[a]
            if np.linalg.norm(p - tip) > 1e-9 * r:
                pts.append(p)
    while len(pts) < 64:
        q = _ball(rs, 1, RHO * r)[0]
        if q @ u <= (RHO - 1.5) * r:
            pts.append(centre + q)
    return np.array(pts[:64])


def touching_case(pose, direction, f, thin_source=False, thin_target=False, seed=13):
    """Source tile and target tile touch at x* and y*: after the pose |x* - y*| = f r, every other cross pair beyond 2 r.
    The targets are laid out in the source's frame (y') and taken back, y = R^-T y' + T in float64, rounded to float32: the
    statement works on the rounded inputs.  Target tiles 0 and 2 hold nothing in reach (blobs 100 r away); tile 1 touches."""
    P = params()
    R, t = POSES[pose]
    principal = direction in PRINCIPAL
    if principal:  # A = R^T = U S V^T: the target's own direction v1 is stretched most, s1-fold, onto u1
        U, S, Vt = np.linalg.svd(np.asarray(R, np.float32).astype(np.float64).T)
        sign = 1.0 if direction == "+principal" else -1.0
        u, v1, s1 = sign * U[:, 0], sign * Vt[0], float(S[0])
        assert s1 > 1.2 and not (thin_source or thin_target), pose
    else:
        u = np.asarray(DIRECTIONS[direction], np.float64)
    far = pose == "far"
    origin = OFFSET if far else np.array([0.3, -0.2, 0.8])
    # the row's radius at its place (range ell), so that f is a fraction of x*'s own cut-off
    r0 = radius(P)
    rs = np.random.default_rng([seed, list(POSES).index(pose), (list(DIRECTIONS) + list(PRINCIPAL)).index(direction), int(thin_source),
                                int(thin_target)])
    xstar = origin.copy()
    r = r0 * (np.linalg.norm(np.float32(xstar).astype(np.float64)) / 500.0 + 1.0)
    src = _shape(rs, thin_source, xstar, u, r)
    ystar = xstar + f * r * u
    tile = _shape(rs, thin_target, ystar, -u, r)
    w = _perp(u)
    before = xstar + 100.0 * r * w + _ball(rs, 64, r)
    after = xstar - 100.0 * r * w + 30.0 * r * u + _ball(rs, 64, r)
    yp = np.concatenate([before, tile, after])
    if far:
        t = OFFSET - R @ OFFSET
    t = np.asarray(t, np.float64)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t
    # back through the float32 pose the device gets: y' = R^T (y - T)  <=>  y = R^-T y' + T (R y' + T for a rotation)
    A = T[:3, :3].astype(np.float64).T
    y = yp @ np.linalg.inv(T[:3, :3].astype(np.float64)) + T[:3, 3].astype(np.float64)
    limit = dict(pairs=1 if f < 1 else 0, f=f)
    if principal:
        # The touching tile is a ball of radius RHO r in the target's OWN frame, which the pose makes an ellipsoid: y* is its
        # far end along the longest moved axis, s1 RHO r from the moved centre, while the tile's record says RHO r.  Its other
        # points keep 1.5 r behind y*'s plane, as seen after the pose.
        pts = [-RHO * r * v1]
        for a in range(3):
            for sg in (-1.0, 1.0):
                q = sg * RHO * r * np.eye(3)[a]
                if np.linalg.norm(q - pts[0]) > 1e-9 * r and (A @ q) @ (-u) <= (s1 * RHO - 1.5) * r:
                    pts.append(q)
        while len(pts) < 64:
            q = _ball(rs, 1, RHO * r)[0]
            if (A @ q) @ (-u) <= (s1 * RHO - 1.5) * r:
                pts.append(q)
        own_tip = np.linalg.solve(A, ystar) + T[:3, 3].astype(np.float64)
        y[64:128] = own_tip + RHO * r * v1 + np.array(pts)
        limit.update(stretch=s1)
    name = f"touch-{pose}-{direction}-{f}" + ("-thinsrc" if thin_source else "") + ("-thintgt" if thin_target else "")
    return Case(name, P, src, y, T=T, tol="far" if far else "geo", limit=limit, tags=("touch", pose))


def touching_cases(pose):
    """Ten directions; for the matrices that are no rotation also the two ends of the axis the pose stretches most, with the
    target a ball in its OWN frame: without `stretch` in the first cull's reach these are culled."""
    return [touching_case(pose, d, f) for d in list(DIRECTIONS) + (list(PRINCIPAL) if pose in NON_ROTATIONS else []) for f in FS]


def thin_cases(pose):
    return [touching_case(pose, d, f, thin_source=ts, thin_target=not ts) for d in THIN_DIRECTIONS for f in FS for ts in (False, True)]


# ---- the tile list ----------------------------------------------------------------------------------------------------------
TILE_COUNTS = (512, 513, 1024, 1025, 1026)
FILLINGS = ("far", "shell")


def special_tiles(n_tiles):
    """Target tiles that hold pairs: the first and last of a 512-tile pass, of a 1024-tile round, and the cloud's last."""
    return sorted({t for t in (0, OV_PASS - 1, OV_PASS, OV_LIST_CAP - 1, OV_LIST_CAP, n_tiles - 1) if t < n_tiles})


def list_rows(P):
    """The row tile of the tile-list cases: 64 rows on a 4 x 4 x 4 grid of spacing 3 r (a target within 0.9 r of one row is at
    least 2.1 r from every other)."""
    r = radius(P)
    g = np.stack(np.unravel_index(np.arange(64), (4, 4, 4)), 1).astype(np.float64)
    return (g - 1.5) * 3.0 * r + np.array([0.2, -0.1, 0.5])


def list_case(n_tiles, filling, n_rows=64, seed=14):
    """64 rows against M = 64 n_tiles - 37 targets (the last tile is partial: 27 points).  special_tiles(n_tiles) hold 3 .. 5
    pairs each - targets 0.1 r .. 0.9 r from a row of their own, at the first positions of their tile, in the last tile at its
    last positions.  Every other target is
      far    in a block of its tile's own (4 x 4 x 4, spacing 4 r) on a block grid that starts 60 r away: nearly every tile
             is culled by its sphere and box;
      shell  in a patch (radius 0.4 r) around a body centre of the rows' grid - inside the row tile's reach, 2.2 r and more from
             every row, its box r and more: every tile is listed and the second cull rejects it."""
    P = params()
    r = radius(P)
    rs = np.random.default_rng([seed, n_tiles, FILLINGS.index(filling)])
    rows = list_rows(P)
    M = 64 * n_tiles - 37
    t = np.arange(M) // 64
    if filling == "far":
        b = np.stack(np.unravel_index(np.arange(n_tiles), (11, 11, 11)), 1).astype(np.float64)
        k = np.stack(np.unravel_index(np.arange(M) % 64, (4, 4, 4)), 1).astype(np.float64)
        tgt = 60.0 * r + b[t] * 16.0 * r + k * 4.0 * r
    else:
        body = (np.stack(np.unravel_index(np.arange(27), (3, 3, 3)), 1).astype(np.float64) - 1.0) * 3.0 * r + rows.mean(0)
        tgt = body[t % 27] + _ball(rs, M, 0.4 * r)
    pairs, row = [], 0
    for s in special_tiles(n_tiles):
        k = 3 + (s % 3)
        last = min(64, M - 64 * s)
        pos = 64 * s + (np.arange(k) if s != n_tiles - 1 else last - 1 - np.arange(k))
        for j in pos:
            i = row % n_rows
            row += 7
            tgt[j] = rows[i] + _dirs(rs, 1)[0] * r * math.sqrt(rs.uniform(0.01, 0.81))
            pairs.append((i, int(j)))
    return Case(f"list-{n_tiles}-{filling}" + (f"-n{n_rows}" if n_rows != 64 else ""), P, rows[:n_rows], tgt,
                limit=dict(pairs=sorted(pairs), tiles=special_tiles(n_tiles)), tags=("list",))


# ---- nothing in reach ---------------------------------------------------------------------------------------------------------
def nothing_case(seed=15):
    """Two clouds of three tiles each, 40 r apart: exactly 0.0, not void."""
    P = params()
    r = radius(P)
    rs = np.random.default_rng(seed)
    return Case("nothing", P, _ball(rs, 150, 3 * r), np.array([40.0 * r, 0, 0]) + _ball(rs, 170, 3 * r), limit=dict(pairs=0),
                tags=("nothing",))


def reversed_list_case():
    """list_case(1025, 'far') with the clouds exchanged: 1025 row tiles against one target tile."""
    big = list_case(1025, "far")
    return Case("list-1025-far-reversed", big.P, big.tgt, big.src, limit=dict(pairs=sorted((j, i) for i, j in big.limit["pairs"])),
                tags=("reversed",))


def angle_cases():
    """The <X, Y> evaluations of the exact function_angle jobs: ONE point, the first row of list_case(1025, 'far'), against
    its 1025 target tiles, and the reverse."""
    full = list_case(1025, "far")
    want = [(i, j) for i, j in full.limit["pairs"] if i == 0]
    return (Case("angle-1xM", full.P, full.src[:1], full.tgt, limit=dict(pairs=want), tags=("angle",)),
            Case("angle-Mx1", full.P, full.tgt, full.src[:1], limit=dict(pairs=[(j, i) for i, j in want]), tags=("angle",)))


def all_cases():
    """Every case that goes through the statement."""
    out = [queue_case(l, f) for l in QUEUE_LAYOUTS for f in QUEUE_FEATURES]
    out += [queue_case("1025", None, K=63), queue_case("1025", None, K=64)]
    out += [busy_queue_case(n) for n in BUSY_TILES]
    out += [partial_case(n, m) for n, m in PARTIAL] + [partial_case(64, 65, "target"), partial_case(65, 64, "row")]
    for pose in BALL_POSES:
        out += touching_cases(pose)
    for pose in THIN_POSES:
        out += thin_cases(pose)
    out += [list_case(n, f) for n in TILE_COUNTS for f in FILLINGS]
    out.append(nothing_case())
    out.append(reversed_list_case())
    out += list(angle_cases())
    return out
