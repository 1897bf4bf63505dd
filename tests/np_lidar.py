"""The LiDAR front end, stated in numpy from upstream's text: CvoPointCloud(PointCloud<PointXYZI>::Ptr, n, beams, LOAM) and its
semantic twin (CvoPointCloud.cpp:964-1136) = LidarPointSelector::edge_detection (LidarPointSelector.cpp:38-136), then
LeGoLoamPointSelection::cloudHandler (LeGoLoamPointSelection.cpp:61-85).  Shares no code with the library: the CPU twin
(cvo_lidar_select_host) and the kernels (cvo_lidar_select) must return exactly what `select` returns.

Where upstream's text leaves a choice, or is broken, this is what is stated (DESIGN.md section 3 repeats the list):

1. Index convention.  The non-semantic overload labels a point with (uint32_t) intensity where the semantic one uses the point
   index (LidarPointSelector.cpp:186 against :229), so its LeGO-LOAM half would return index 0 or 1 for every point.  The
   point index is used in both.
2. edge_detection's end points.  The semantic loop reads points[i - 1] at i = 0 and points[i + 1] at i = n - 1; both loops run
   1 .. n - 2 here.  The ring state machine is literal: the `continue` on a 4 -> 1 transition skips the update of
   previous_quadrant, so from the first transition on every quadrant-1 point is skipped until ring_num reaches
   beam_num - 1; in the semantic overload an unlabelled point is skipped the same way (before the quadrant is looked at).
3. Uninitialised reads.  cloudLabel[k], cloudNeighborPicked[k], cloudCurvature[k] and cloudSmoothness[k] are never written for
   k < 5 and k >= size - 5 while ring 0's first sixth starts at 4: they read as 0 / 0 / 0 / (value 0, ind 0).
4. std::sort ties.  by_value leaves equal curvatures in unspecified order: the order is (value, then segmented index).
5. Dead branch.  Ground cells get labelMat = -1 and never enter the segmented cloud, so segmentedCloudGroundFlag is false
   everywhere and the flat-surface loop (:770-804) never picks: it is not stated, `select` asserts that no segmented cell is
   ground.
6. Transcendentals.  No decision rests on a libm call.  atan2(y, x) > segmentTheta is y > tan(theta) x for x > 0, true for
   x <= 0 with y > 0, false otherwise ((0, 0) included); |angle - mount| <= 10 and |angle - mount| > 3 of groundRemoval are
   tan(mount - 10) h <= dy <= tan(mount + 10) h and dy > tan(mount + 3) h or dy < tan(mount - 3) h with h the horizontal
   length: all in double against constants the config carries (cvo_lidar_config_derive).  abs is the floating-point one.
   The column of a point needs an angle: `atan2_deg` below, IEEE add / multiply / divide in double in a fixed order, within
   1e-7 degrees of the true value.  sqrt of a float is the correctly rounded float root.
7. The validity quirk.  lineCountFlag is set for pushed cells only (:463), never for the seed: the row count of a component is
   the number of distinct rows among its members other than its lowest row-major cell (the seed: the scan is row-major and the
   neighbour criterion symmetric, so the components do not depend on the visiting order).
8. Cell collisions.  The last point in index order wins a cell (:261-271), among those that pass the ring, column and
   minimum-range tests.
9. A non-finite coordinate is refused by the library (upstream mis-indexes after dropping NaNs); nothing to state.
"""
import collections

import numpy as np

F32 = np.float32
INVALID = 999999


class Rand:
    """glibc's default rand(): srandom_r / random_r for TYPE_3 (degree 31, separation 3), restated."""

    def __init__(self, seed=1):
        seed = int(seed) & 0xffffffff
        if seed == 0:
            seed = 1
        word = seed - (1 << 32) if seed >= (1 << 31) else seed
        self.r = [seed]
        for _ in range(30):
            hi = cdiv(word, 127773)  # C's truncating division and remainder
            lo = word - hi * 127773
            word = 16807 * lo - 2836 * hi
            if word < 0:
                word += 2147483647
            self.r.append(word & 0xffffffff)
        self.f, self.b, self.count = 3, 0, 0
        for _ in range(310):
            self.next()
        self.count = 0

    def next(self):
        v = (self.r[self.f] + self.r[self.b]) & 0xffffffff
        self.r[self.f] = v
        self.f += 1
        if self.f >= 31:
            self.f = 0
            self.b += 1
        else:
            self.b += 1
            if self.b >= 31:
                self.b = 0
        self.count += 1
        return v >> 1


def atan2_deg(y, x):
    """atan2 in degrees from add, multiply and divide in double, every operation rounded on its own.  a = min / max of the
    magnitudes; above tan(pi / 8) folded by atan a = 45 + atan((a - 1) / (a + 1)); the odd Taylor series to t^19 by Horner
    (truncation below 0.4143^21 / 21 = 4.4e-10 rad = 2.6e-8 degrees); then the octant.  (0, 0) is 0."""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    ay, ax = np.abs(y), np.abs(x)
    hi, lo = np.where(ax > ay, ax, ay), np.where(ax > ay, ay, ax)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = lo / hi
    fold = a > 0.41421356237309503
    with np.errstate(invalid="ignore"):
        t = np.where(fold, (a - 1.0) / (a + 1.0), a)
    s = t * t
    p = np.full_like(s, -1.0 / 19.0)
    for c in (1.0 / 17.0, -1.0 / 15.0, 1.0 / 13.0, -1.0 / 11.0, 1.0 / 9.0, -1.0 / 7.0, 1.0 / 5.0, -1.0 / 3.0, 1.0):
        p = p * s + c
    d = np.where(fold, 45.0, 0.0) + (p * t) * 57.295779513082323
    d = np.where(ay > ax, 90.0 - d, d)
    d = np.where(x < 0, 180.0 - d, d)
    d = np.where(y < 0, -d, d)
    return np.where(hi == 0.0, 0.0, d)


def quadrant(x, z):
    """get_quadrant on u = z, v = -x."""
    u, v = np.asarray(z, F32), -np.asarray(x, F32)
    q = np.zeros(u.shape, np.int32)
    q[(u >= 0) & (v < 0)] = 4
    q[(u < 0) & (v <= 0)] = 3
    q[(u <= 0) & (v > 0)] = 2
    q[(u > 0) & (v >= 0)] = 1
    return q


def frange(x, y, z):
    return np.sqrt(x * x + y * y + z * z, dtype=F32)


def column(x, z, ang_res_x, H):
    h = atan2_deg(z.astype(np.float64), (-x).astype(np.float64)).astype(F32)
    q = (h.astype(np.float64) - 90.0) / np.float64(F32(ang_res_x))
    r = np.where(q < 0, -np.floor(-q + 0.5), np.floor(q + 0.5))
    c = -r + float(H // 2)
    c = np.where(c >= H, c - H, c)
    return np.where((c >= 0) & (c < H), c, -1).astype(np.int64)


def cdiv(a, b):
    """C's integer division."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def edge_detection(xyzi, cfg, semantic=None):
    n = len(xyzi)
    x, y, z, it = (xyzi[:, k].astype(F32) for k in range(4))
    quad = quadrant(x, z)
    sel = np.zeros(n, bool)
    if n >= 3:
        d = xyzi[1:, :3].astype(F32) - xyzi[:-1, :3].astype(F32)
        norm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2], dtype=F32)
        depth = np.maximum(norm[:-1], norm[1:]).astype(np.float64)
        di = np.abs(it[1:] - it[:-1])
        inten = np.maximum(di[:-1], di[1:]).astype(np.float64)
        c = slice(1, n - 1)
        sel[c] = (((inten > cfg.intensity_bound) | (depth > cfg.depth_bound)) & (it[c] > 0) & (x[c] != 0) & (y[c] != 0) & (z[c] != 0) &
                  (frange(x[c], y[c], z[c]).astype(np.float64) < cfg.distance_bound))
    out, prev, ring = [], int(quad[0]), 0
    for i in range(1, n - 1):
        if semantic is not None and semantic[i] == -1:
            continue
        q = int(quad[i])
        if q == 1 and prev == 4 and ring < cfg.beam_num - 1:
            ring += 1
            continue
        if sel[i]:
            out.append(i)
        prev = q
    return out


def _connected(ra, rb, same_row, cfg):
    d1, d2 = (float(ra), float(rb)) if ra > rb else (float(rb), float(ra))
    yy = d2 * (cfg.sin_alpha_x if same_row else cfg.sin_alpha_y)
    xx = d1 - d2 * (cfg.cos_alpha_x if same_row else cfg.cos_alpha_y)
    if xx > 0.0:
        return yy > cfg.tan_theta * xx
    return yy > 0.0


def lego(xyzi, cfg, rand, no_spill=False):
    """cloudHandler -> dict: `index` / `is_edge` in upstream's output order and every intermediate the tests look at."""
    R, H = cfg.n_scan, cfg.horizon_scan
    n = len(xyzi)
    x, y, z = (xyzi[:, k].astype(F32) for k in range(3))
    # copyPointCloud: the ring is the number of 4 -> 1 transitions so far
    quad = quadrant(x, z)
    trans = np.zeros(n, np.int64)
    trans[1:] = (quad[1:] == 1) & (quad[:-1] == 4)
    ring = np.cumsum(trans)
    # projectPointCloud
    col = column(x, z, cfg.ang_res_x, H)
    rng = frange(x, y, z)
    ok = (ring < R) & (col >= 0) & ~(rng < F32(cfg.sensor_min_range))
    win = np.full(R * H, -1, np.int64)
    cell = ring * H + col
    win[cell[ok]] = np.nonzero(ok)[0]  # (ascending indices, the last assignment stands)
    full = win >= 0
    rmat = np.where(full, rng[np.maximum(win, 0)], np.finfo(F32).max).astype(F32)
    # groundRemoval
    ground = np.zeros(R * H, bool)
    for i in range(cfg.ground_scan_ind):
        lo, up = np.arange(i * H, (i + 1) * H), np.arange((i + 1) * H, (i + 2) * H)
        both = full[lo] & full[up]
        pl, pu = xyzi[np.maximum(win[lo], 0), :3].astype(F32), xyzi[np.maximum(win[up], 0), :3].astype(F32)
        dx, dy, dz = pu[:, 0] - pl[:, 0], pu[:, 1] - pl[:, 1], pu[:, 2] - pl[:, 2]
        h = np.sqrt((dx * dx + dz * dz).astype(np.float64))
        slope = (dy.astype(np.float64) <= cfg.tan_ground_hi * h) & (dy.astype(np.float64) >= cfg.tan_ground_lo * h)
        hs = np.sqrt((pl[:, 0] * pl[:, 0] + pl[:, 2] * pl[:, 2]).astype(np.float64))
        ly = pl[:, 1].astype(np.float64)
        off = (ly > cfg.tan_self_hi * hs) | (ly < cfg.tan_self_lo * hs)
        g = both & slope & off
        ground[lo[g]] = True
        ground[up[g]] = True
    label = np.where(ground | ~full, -1, 0).tolist()
    rl = rmat.tolist()  # (floats hold every float32 exactly)
    # cloudSegmentation / labelComponents
    count, comps = 1, []
    for seed in range(R * H):
        if label[seed] != 0:
            continue
        queue, pushed, rows = collections.deque([seed]), [seed], set()
        while queue:
            frm = queue.popleft()
            fr, fc = divmod(frm, H)
            label[frm] = count
            for dr, dc in ((-1, 0), (0, 1), (0, -1), (1, 0)):
                r, c = fr + dr, fc + dc
                if r < 0 or r >= R:
                    continue
                if c < 0:
                    c = H - 1
                if c >= H:
                    c = 0
                to = r * H + c
                if label[to] != 0:
                    continue
                if _connected(rl[frm], rl[to], dr == 0, cfg):
                    queue.append(to)
                    label[to] = count
                    rows.add(r)
                    pushed.append(to)
        valid = len(pushed) >= 30 or (len(pushed) >= cfg.segment_valid_point_num and len(rows) >= cfg.segment_valid_line_num)
        comps.append(dict(seed=seed, cells=pushed, valid=valid))
        if valid:
            count += 1
        else:
            for c in pushed:
                label[c] = INVALID
    # the segmented cloud
    seg_col, seg_pt, seg_cell, start, end = [], [], [], [], []
    for i in range(R):
        start.append(len(seg_pt) - 1 + 5)
        for j in range(H):
            c = i * H + j
            if label[c] > 0 or ground[c]:
                if label[c] == INVALID or ground[c]:
                    continue
                seg_col.append(j)
                seg_pt.append(int(win[c]))
                seg_cell.append(c)
        end.append(len(seg_pt) - 1 - 5)
    S = len(seg_pt)
    assert not ground[np.array(seg_cell, np.int64)].any() if S else True  # departure 5
    sr = rmat[np.array(seg_cell, np.int64)] if S else np.zeros(0, F32)
    # calculateSmoothness
    curv = np.zeros(S, F32)
    if S > 10:
        i = np.arange(5, S - 5)
        d = sr[i - 5] + sr[i - 4]
        for o in (-3, -2, -1):
            d = d + sr[i + o]
        d = d - sr[i] * F32(10)
        for o in (1, 2, 3, 4, 5):
            d = d + sr[i + o]
        with np.errstate(over="ignore"):
            curv[i] = d * d
    curv_l = curv.tolist()
    smooth = [(0.0, 0)] * S
    for i in range(5, S - 5):
        smooth[i] = (curv_l[i], i)
    picked, lab = [0] * S, [0] * S
    # markOccludedPoints
    srl = sr.tolist()
    for i in range(5, S - 6):
        d1, d2 = sr[i], sr[i + 1]
        if abs(seg_col[i + 1] - seg_col[i]) < 10:
            if float(d1 - d2) > 0.3:
                for o in range(-5, 1):
                    picked[i + o] = 1
            elif float(d2 - d1) > 0.3:
                for o in range(1, 7):
                    picked[i + o] = 1
        a, b = float(abs(F32(sr[i - 1] - sr[i]))), float(abs(F32(sr[i + 1] - sr[i])))
        if a > 0.02 * srl[i] and b > 0.02 * srl[i]:
            picked[i] = 1
    occluded = sum(picked)
    # extractFeatures
    index, is_edge, n_edge, n_thin, draws, capped, sixths = [], [], 0, 0, 0, 0, []
    thr = float(F32(cfg.edge_threshold))
    for i in range(R):
        for j in range(6):
            sp = cdiv(start[i] * (6 - j) + end[i] * j, 6)
            ep = cdiv(start[i] * (5 - j) + end[i] * (j + 1), 6) - 1
            if sp >= ep:
                continue
            sixths.append((i, j, sp, ep))
            smooth[sp:ep] = sorted(smooth[sp:ep])  # (value, then index)
            largest = 0
            for k in range(ep, sp - 1, -1):
                ind = smooth[k][1]
                if picked[ind] == 0 and curv_l[ind] > thr:
                    largest += 1
                    if largest <= 20:
                        lab[ind] = 2 if largest <= 2 else 1
                        index.append(seg_pt[ind])
                        is_edge.append(1)
                        n_edge += 1
                    else:
                        capped += 1
                        break
                    picked[ind] = 1
                    for o in range(1, 6):
                        if abs(seg_col[ind + o] - seg_col[ind + o - 1]) > 10:
                            break
                        if not no_spill or sp <= ind + o <= ep:
                            picked[ind + o] = 1
                    for o in range(-1, -6, -1):
                        if abs(seg_col[ind + o] - seg_col[ind + o + 1]) > 10:
                            break
                        if not no_spill or sp <= ind + o <= ep:
                            picked[ind + o] = 1
            for k in range(sp, ep + 1):
                if lab[k] <= 0:
                    draws += 1
                    if rand.next() % 4 == 0:
                        index.append(seg_pt[k])
                        is_edge.append(0)
                        n_thin += 1
    return dict(index=index, is_edge=is_edge, projected=int(full.sum()), ground=int(ground.sum()),
                valid=sum(c["valid"] for c in comps), invalid=sum(not c["valid"] for c in comps), segmented=S, edges=n_edge,
                draws=draws, thinned=n_thin, occluded=occluded, capped=capped, comps=comps, sixths=sixths, curvature=curv,
                seg_cell=seg_cell, seg_pt=seg_pt, win=win, ring=ring, ground_cells=ground)


def select(xyzi, cfg, rand, semantic=None, no_spill=False):
    """What cvo_lidar_select returns: (indices, is_edge) plus the statement's intermediates.  `rand` (a Rand) is advanced."""
    xyzi = np.ascontiguousarray(xyzi, F32).reshape(-1, 4)
    first = edge_detection(xyzi, cfg, semantic)
    before = rand.count
    out = lego(xyzi, cfg, rand, no_spill)
    keep = [k for k, i in enumerate(out["index"]) if semantic is None or semantic[i] != -1]
    out["index"] = np.array(first + [out["index"][k] for k in keep], np.int32)
    out["is_edge"] = np.array([1] * len(first) + [out["is_edge"][k] for k in keep], bool)
    out["edge_detected"] = len(first)
    assert rand.count - before == out["draws"]
    return out


def rows(xyzi, index, semantic=None, num_classes=0):
    """The constructor's rows for the selected points: xyz, F = 1 intensity, type (1, 0), one-hot labels."""
    xyzi = np.ascontiguousarray(xyzi, F32).reshape(-1, 4)
    out = dict(xyz=xyzi[index, :3].copy(), feat=xyzi[index, 3:4].copy(), geotype=np.tile(np.array([1, 0], F32), (len(index), 1)))
    if semantic is not None:
        lab = np.zeros((len(index), num_classes), F32)
        lab[np.arange(len(index)), np.asarray(semantic)[index]] = 1
        out["label"] = lab
    return out
