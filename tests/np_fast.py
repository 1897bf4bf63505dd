"""numpy statement of the CV_FAST point selection (cvo_fast_select): cv::FAST(gray, keypoints, t, nonmax = false) with
TYPE_9_16, and the reference's adaptive threshold schedule (CvoPointCloud.cpp:273-312), taken literally.  Shares no code
with the library.  Parity with an OpenCV binary is not pinned: the definition below is OpenCV's
documented one - segment test on the radius-3 Bresenham ring, 9 contiguous pixels, strict comparisons.

Two independent statements of the detector: `corners` decides one threshold at a time by run lengths of the comparison
bits; `score` computes s(p) = max over the 16 arcs and the 2 signs of the min of +-d_k over the arc, and p is a corner at t
iff s(p) > t - so one pass and a 257-bin histogram of s give the keypoint count at every threshold."""
import numpy as np

# ring offsets (dx, dy) in OpenCV's order
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
        (-2, 2), (-1, 3)]
# (thresh, num_want, num_min, break_thresh)
RGBD, STEREO, STEREO_SEMANTIC = (9, 15000, 12000, 13), (4, 24000, 15000, 50), (4, 28000, 15000, 50)


def ring_differences(gray):
    """(16, h - 6, w - 6) int16: d_k = I_k - I_p for every interior pixel p (3 <= x < w - 3, 3 <= y < h - 3)."""
    I = np.asarray(gray, np.uint8).astype(np.int16)
    h, w = I.shape
    if h < 7 or w < 7:
        return np.zeros((16, max(h - 6, 0), max(w - 6, 0)), np.int16)
    centre = I[3:h - 3, 3:w - 3]
    return np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - centre for dx, dy in RING])


def _has_run_of_9(bits):
    """bits (16, ...) bool around the ring: is there a cyclic run of 9 set bits?"""
    m = np.zeros(bits.shape[1:], np.uint32)  # the ring as a word: bit k = bits[k], bits 16 .. 31 the ring again
    for k in range(16):
        m |= bits[k].astype(np.uint32) << np.uint32(k)
    m |= m << np.uint32(16)
    run = m.copy()                           # bit k of run: bits k .. k + 8 of the doubled ring are all set
    for j in range(1, 9):
        run &= m >> np.uint32(j)
    return (run & np.uint32(0xFFFF)) != 0


def corners(gray, t, d=None):
    """The direct statement: (h, w) bool, the keypoints of cv::FAST at threshold t (clamped to 0 .. 255).  d: the ring
    differences of `gray`, when the caller has them."""
    t = min(max(int(t), 0), 255)
    h, w = np.asarray(gray).shape
    out = np.zeros((h, w), bool)
    d = ring_differences(gray) if d is None else d
    if d.shape[1] and d.shape[2]:
        out[3:h - 3, 3:w - 3] = _has_run_of_9(d > t) | _has_run_of_9(d < -t)
    return out


def keypoints(gray, t):
    """Pixel indices v * w + u of the keypoints at t, row-major (the driver truncates kp.pt to ints: they are integers)."""
    return np.flatnonzero(corners(gray, t).reshape(-1)).astype(np.int32)


def score(gray):
    """The score statement: (h, w) int64, s(p) clamped below at -1; -1 outside the interior."""
    h, w = np.asarray(gray).shape
    s = np.full((h, w), -1, np.int64)
    d = ring_differences(gray).astype(np.int64)
    if d.shape[1] and d.shape[2]:
        best = np.full(d.shape[1:], -256, np.int64)
        for k in range(16):
            arc = d[[(k + j) % 16 for j in range(9)]]
            best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
        s[3:h - 3, 3:w - 3] = np.maximum(best, -1)
    return s


def histogram(s):
    """257 bins: pixels with s = -1, 0, ..., 255."""
    return np.bincount((np.asarray(s).reshape(-1) + 1).astype(np.int64), minlength=257)


def counts_from_histogram(hist):
    """count[t] for t = 0 .. 255: pixels with s > t."""
    suffix = np.concatenate([np.cumsum(hist[::-1])[::-1], [0, 0]])
    return np.array([suffix[t + 2] for t in range(256)], np.int64)


def schedule(count, preset):
    """CvoPointCloud.cpp:278-302 over count(t): returns (threshold of the last call, thresholds tried, counts).
    QUIRKS: the first call is always at 5; `thresh` starts at the preset's value, so STEREO's first raise re-evaluates 5 and
    RGBD's first lowering goes to 8; with no loop taken the result is the one at 5; the second loop runs after the first
    one, whatever that one did; break_thresh ends the first loop even above num_want, 0 the second even below num_min.
    (A lowering loop that would pass below 0 ends there; upstream's would not end.)"""
    thresh, want, nmin, brk = preset
    tried, counts = [], []

    def run(t):
        c = int(count(min(max(t, 0), 255)))
        tried.append(t)
        counts.append(c)
        return c

    n = run(5)
    while n > want:
        thresh += 1
        n = run(thresh)
        if thresh == brk:
            break
    while n < nmin:
        thresh -= 1
        n = run(thresh)
        if thresh <= 0:
            break
    return min(max(tried[-1], 0), 255), tried, counts


def select(gray, preset):
    """The CV_FAST branch of select_points_from_image: (pixel indices, threshold used, thresholds tried, counts), every
    count taken with the direct statement."""
    d = ring_differences(gray)
    used, tried, counts = schedule(lambda t: int(np.count_nonzero(corners(gray, t, d))), preset)
    return np.flatnonzero(corners(gray, used, d).reshape(-1)).astype(np.int32), used, tried, counts
