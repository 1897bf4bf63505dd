"""The statement of the disparity post-filter (cvo_disparity_filter): libelas's removeSmallSegments, gapInterpolation and
adaptiveMean (elas.cpp, full-resolution branch, in that order) restated in numpy float32, one IEEE operation at a time.  A map is
(rows, cols) float32; a pixel is invalid when it is negative, and the passes write invalid pixels as -10.

Not restated, because upstream's StaticStereo never turns them on: param.subsampling, the add_corners extrapolation, median.

Departure from libelas (the only one): adaptiveMean's D_tmp comes from malloc and is written only at invalid pixels and where
the horizontal pass stores a result, yet the vertical pass reads all of it - column 3 and rows 0-2 and H-3 .. H-1 are never
written.  libelas's output therefore depends on heap contents in column 3, rows 4-6 and rows H-6 .. H-4.  Here D_tmp starts as
a copy of D_copy.  tests/golden/dfilter_elas.npz pins everything else against libelas's compiled passes.

For H < 7 or W < 8 libelas's ring initialisation reads past the row or the map without using what it read; here the loops are
simply empty."""
import numpy as np

F = np.float32
INVALID = F(-10.0)
ABS_BITS = np.uint32(0x4F000000)  # the bit pattern of (float)0x7FFFFFFF, which is what _mm_set1_ps(0x7FFFFFFF) makes


class Config:
    def __init__(self, speckle_sim_threshold=1.0, speckle_size=200, ipol_gap_width=3, adaptive_mean=1):
        self.speckle_sim_threshold, self.speckle_size = float(speckle_sim_threshold), int(speckle_size)
        self.ipol_gap_width, self.adaptive_mean = int(ipol_gap_width), int(adaptive_mean)


def speckle(d, sim, size):
    """removeSmallSegments: the literal sequential flood fill, seeds in column-major order -> (map, segments of valid pixels,
    valid pixels removed).  A negative seed is a segment of its own."""
    d = np.array(d, F)
    H, W = d.shape
    sim = F(sim)
    segments = removed = 0
    if size <= 1:  # (seg_list_count < speckle_size never holds)
        return d, 0, 0
    done = np.zeros((H, W), bool)
    for u in range(W):
        for v in range(H):
            if done[v, u]:
                continue
            seg = [(u, v)]
            i = 0
            while i < len(seg):
                cu, cv = seg[i]
                for nu, nv in ((cu - 1, cv), (cu + 1, cv), (cu, cv - 1), (cu, cv + 1)):
                    if 0 <= nu < W and 0 <= nv < H and not done[nv, nu] and d[nv, nu] >= 0:
                        if np.abs(F(d[cv, cu] - d[nv, nu])) <= sim:
                            seg.append((nu, nv))
                            done[nv, nu] = True
                i += 1
                done[cv, cu] = True
            valid = d[v, u] >= 0
            segments += int(valid)
            if len(seg) < size:
                removed += len(seg) if valid else 0
                for su, sv in seg:
                    d[sv, su] = INVALID
    return d, segments, removed


def _gap_line(line, width):
    """one row or column, in place -> pixels filled"""
    count = filled = 0
    n = len(line)
    for j in range(n):
        if line[j] >= 0:
            if 1 <= count <= width:
                first, last = j - count, j - 1
                if first > 0 and last < n - 1:
                    d1, d2 = line[first - 1], line[last + 1]
                    line[first:j] = F(F(d1 + d2) / F(2)) if np.abs(F(d1 - d2)) < F(3) else min(d1, d2)
                    filled += count
            count = 0
        else:
            count += 1
    return filled


def gap(d, width):
    """gapInterpolation: rows, then columns on the rows' result -> (map, pixels filled)"""
    d = np.array(d, F)
    filled = 0
    for v in range(d.shape[0]):
        filled += _gap_line(d[v, :], width)
    for u in range(d.shape[1]):
        filled += _gap_line(d[:, u], width)
    return d, filled


def _weights(val, cur):
    """max(0, 4 - bits_as_float(bits(val - cur) & 0x4F000000))"""
    t = (np.asarray(val - cur, F).view(np.uint32) & ABS_BITS).view(F)
    return np.maximum(F(0), F(4) - t)


def _mean_pass(src, dst, lo, hi):
    """One pass along axis 1 of `src`: for every row and every centre c in lo .. hi the ring libelas holds when it stores
    centre c - slot k is the value at the coordinate x of c - 4 .. c + 3 with x % 8 == k -, lanes k = slot k + slot k + 4, the four
    lanes summed from the left, one division.  Stores into dst[:, c] where the weight sum is positive and the result >= 0."""
    if hi < lo:
        return
    c = np.arange(lo, hi + 1)
    k = np.arange(8)
    x = (c[:, None] - 4) + ((k[None, :] - (c[:, None] - 4)) % 8)  # (centres, 8)
    val = src[:, x]                                               # (rows, centres, 8)
    cur = src[:, c][:, :, None]
    with np.errstate(over="ignore", invalid="ignore"):
        w = _weights(val, cur)
        f = (val * w).astype(F)
        wl, fl = w[..., :4] + w[..., 4:], f[..., :4] + f[..., 4:]
        ws = ((wl[..., 0] + wl[..., 1]) + wl[..., 2]) + wl[..., 3]
        fs = ((fl[..., 0] + fl[..., 1]) + fl[..., 2]) + fl[..., 3]
        q = np.where(ws > 0, fs / np.where(ws > 0, ws, F(1)), F(-1)).astype(F)
    assert w.dtype == F and ws.dtype == F and fs.dtype == F
    keep = (ws > 0) & (q >= 0)
    block = dst[:, lo:hi + 1]
    block[keep] = q[keep]


def mean(d):
    """adaptiveMean -> (map, D_tmp after the horizontal pass).  Horizontal: rows 3 .. H - 4, centres 4 .. W - 4, from D_copy into
    D_tmp; vertical: columns 3 .. W - 4, centres 4 .. H - 4, from D_tmp into D (libelas's loops u = 7 .. W - 1 store centre u - 3)."""
    d = np.array(d, F)
    H, W = d.shape
    copy = np.where(d < 0, INVALID, d).astype(F)
    tmp = copy.copy()  # (the departure)
    if H >= 7:
        _mean_pass(copy[3:H - 3, :], tmp[3:H - 3, :], 4, W - 4)
    if W >= 7:
        # columns as rows: the transposes are views, the stores land in d
        _mean_pass(tmp.T[3:W - 3, :], d.T[3:W - 3, :], 4, H - 4)
    return d, tmp


def stages(d, cfg=None):
    """-> dict(speckle, gap, mean_tmp, out, counts): the map after each pass, and (segments, removed, filled)"""
    cfg = cfg or Config()
    a, segments, removed = speckle(d, cfg.speckle_sim_threshold, cfg.speckle_size)
    b, filled = gap(a, cfg.ipol_gap_width)
    c, tmp = mean(b) if cfg.adaptive_mean else (b.copy(), None)
    return dict(speckle=a, gap=b, mean_tmp=tmp, out=c, counts=(segments, removed, filled))


def dfilter(d, cfg=None):
    return stages(d, cfg)["out"]
