"""The statement of the stereo matcher (cvo_stereo_disparity, include/cvo_hip.h): semi-global matching over a census cost, in
numpy.  Integers throughout; the only float operations are the sub-pixel term's one division and one addition, in float32.
The CPU twin and the kernels of cvo_k_sgm.h equal what this file computes exactly.  This is the project's own matcher, not
upstream's libelas and not any other SGM implementation: parity with either is unpinned.

  census     9 wide x 7 high, replicate border, 62 bits `neighbour < centre` in row-major window order (centre skipped), first
             neighbour most significant
  cost       C(v, u, d) = popcount(cL[v, u] ^ cR[v, u - d]) for u - d >= 0, else 62
  paths      DIRECTIONS in this order, the first `paths` of them; q = p - r the predecessor, m = min_k L(q, k):
             L(p, d) = C(p, d) + min(L(q, d), L(q, d - 1) + p1, L(q, d + 1) + p1, m + p2) - m; terms outside [0, D) left out;
             q outside the image: L(p, d) = C(p, d).  L <= 62 + p2 <= 255, S = sum of the L <= 2040: asserted
  winner     d* = first argmin S, s1 = S(d*), s2 = min S over |d - d*| > 1; invalid when s2 (100 - uniqueness) < 100 s1
  sub-pixel  0 < d* < D - 1 and den = S(d* - 1) + S(d* + 1) - 2 s1 > 0: disp = float(d*) + float(S(d* - 1) - S(d* + 1)) / float(2 den);
             otherwise disp = float(d*)
  left-right lr_max_diff >= 0: dR(v, x) = first argmin_d S(v, x + d, d) over x + d < cols; invalid when u - d* < 0 or
             |dR(v, u - d*) - d*| > lr_max_diff
  output     float32, invalid = -10
"""
import numpy as np

DIRECTIONS = ((0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))
INVALID = np.float32(-10.0)
CENSUS_BITS = 62
DEFAULTS = dict(max_disparity=128, p1=10, p2=120, uniqueness=5, lr_max_diff=1, paths=8)

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def popcount64(x):
    return _POP8[np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (8,))].sum(-1, dtype=np.uint8)


def census(img):
    """(rows, cols) uint8 -> (rows, cols) uint64"""
    img = np.asarray(img, np.uint8)
    rows, cols = img.shape
    pad = np.pad(img, ((3, 3), (4, 4)), mode="edge")
    out = np.zeros(img.shape, np.uint64)
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            nb = pad[3 + dy:3 + dy + rows, 4 + dx:4 + dx + cols]
            out = (out << np.uint64(1)) | (nb < img).astype(np.uint64)
    return out


def cost_volume(cl, cr, D):
    """(rows, cols, D) uint8"""
    rows, cols = cl.shape
    C = np.full((rows, cols, D), CENSUS_BITS, np.uint8)
    for d in range(min(D, cols)):
        C[:, d:, d] = popcount64(cl[:, d:] ^ cr[:, :cols - d])
    return C


def _step(c, lq, p1, p2):
    """One path step for a batch of pixels: c, lq (n, D) int32 -> L (n, D)"""
    m = lq.min(1, keepdims=True)
    best = np.minimum(lq, m + p2)
    best[:, 1:] = np.minimum(best[:, 1:], lq[:, :-1] + p1)
    best[:, :-1] = np.minimum(best[:, :-1], lq[:, 1:] + p1)
    return c + best - m


def path(C, dv, du, p1, p2):
    """L_r of one direction, (rows, cols, D) int32"""
    rows, cols, D = C.shape
    c = C.astype(np.int32)
    L = c.copy()  # (pixels whose predecessor is outside keep L = C)
    if dv == 0:
        us = range(1, cols) if du > 0 else range(cols - 2, -1, -1)
        for u in us:
            L[:, u] = _step(c[:, u], L[:, u - du], p1, p2)
    else:
        vs = range(1, rows) if dv > 0 else range(rows - 2, -1, -1)
        lo, hi = max(0, du), cols + min(0, du)  # the columns u with 0 <= u - du < cols
        for v in vs:
            if hi > lo:
                L[v, lo:hi] = _step(c[v, lo:hi], L[v - dv, lo - du:hi - du], p1, p2)
    assert L.min() >= 0 and L.max() <= CENSUS_BITS + p2 <= 255
    return L


def aggregate(C, p1, p2, paths):
    S = np.zeros(C.shape, np.int32)
    for dv, du in DIRECTIONS[:paths]:
        S += path(C, dv, du, p1, p2)
    assert S.max() <= 2040
    return S.astype(np.uint16)


def right_argmin(S):
    """dR (rows, cols) int32"""
    rows, cols, D = S.shape
    R = np.full((rows, cols, D), 0xFFFF, np.int32)
    for d in range(min(D, cols)):
        R[:, :cols - d, d] = S[:, d:, d]
    return R.argmin(2).astype(np.int32)


def select(S, uniqueness, lr_max_diff):
    """-> (disparity float32, d* int32, valid bool)"""
    rows, cols, D = S.shape
    S = S.astype(np.int32)
    ds = S.argmin(2).astype(np.int32)
    s1 = np.take_along_axis(S, ds[..., None], 2)[..., 0]
    far = np.abs(np.arange(D, dtype=np.int32)[None, None, :] - ds[..., None]) > 1
    s2 = np.where(far, S, 1 << 30).min(2)
    valid = ~(s2 * (100 - uniqueness) < s1 * 100)
    inner = (ds > 0) & (ds < D - 1)
    sm = np.take_along_axis(S, np.clip(ds - 1, 0, D - 1)[..., None], 2)[..., 0]
    sp = np.take_along_axis(S, np.clip(ds + 1, 0, D - 1)[..., None], 2)[..., 0]
    den = sm + sp - 2 * s1
    sub = inner & (den > 0)
    disp = ds.astype(np.float32)
    num = (sm - sp).astype(np.float32)
    den2 = np.where(sub, 2 * den, 1).astype(np.float32)
    disp = np.where(sub, disp + num / den2, disp).astype(np.float32)
    if lr_max_diff >= 0:
        dR = right_argmin(S)
        x = np.arange(cols, dtype=np.int32)[None, :] - ds
        inside = x >= 0
        dr = np.take_along_axis(dR, np.clip(x, 0, cols - 1), 1)
        valid &= inside & (np.abs(dr - ds) <= lr_max_diff)
    return np.where(valid, disp, INVALID).astype(np.float32), ds, valid


def check_config(max_disparity=128, p1=10, p2=120, uniqueness=5, lr_max_diff=1, paths=8):
    return (max_disparity in (64, 128, 256) and 0 <= p1 <= p2 <= 193 and 0 <= uniqueness <= 99 and paths in (4, 8))


def stages(left, right, max_disparity=128, p1=10, p2=120, uniqueness=5, lr_max_diff=1, paths=8):
    """Every stage: dict(census_left, census_right, S, d, valid, disparity)"""
    assert check_config(max_disparity, p1, p2, uniqueness, lr_max_diff, paths)
    left, right = np.asarray(left, np.uint8), np.asarray(right, np.uint8)
    assert left.ndim == 2 and left.shape == right.shape
    cl, cr = census(left), census(right)
    S = aggregate(cost_volume(cl, cr, max_disparity), p1, p2, paths)
    disp, ds, valid = select(S, uniqueness, lr_max_diff)
    return dict(census_left=cl, census_right=cr, S=S, d=ds, valid=valid, disparity=disp)


def disparity(left, right, **config):
    return stages(left, right, **config)["disparity"]
