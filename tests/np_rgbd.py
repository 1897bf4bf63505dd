"""numpy statement of the RGB-D front end (cvo_rgbd_points / cvo_cloud_upload_rgbd): one function per stage of the
reference's recipe, following it literally (file:line relative to the upstream repository).  Shares no code with the
library.  Frames are plain arrays:

    image  (h, w) or (h, w, 3) uint8, BGR byte order for 3 channels (as cv::Mat), AFTER RawImage's denoising
    gray   None or (h, w) uint8: overrides the BGR -> gray formula
    depth  (h, w) uint16 or float32
    calib  (fx, fy, cx, cy, scaling_factor)
    semantic  None or (h, w, num_classes) float32

The quirks that are part of the contract are marked QUIRK."""
import numpy as np

NUM_WANT = 10000
DSO_EDGES, FULL = 2, 8  # cvo::CvoPointCloud::PointSelectionMethod
F32 = np.float32


class Unsupported(Exception):
    pass


def gray_plane(image, gray=None):
    """RawImage.cpp:32-39.  1 channel: as it is.  3 channels: OpenCV 3's 8-bit COLOR_BGR2GRAY,
    (1868 B + 9617 G + 4899 R + 8192) >> 14 (OpenCV 4 uses 15-bit constants and may differ by one level at rare pixels:
    a caller-supplied `gray` overrides the formula)."""
    if gray is not None:
        return np.asarray(gray, np.uint8).astype(F32)
    image = np.asarray(image, np.uint8)
    if image.ndim == 2:
        return image.astype(F32)
    b, g, r = (image[..., k].astype(np.int64) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(F32)


def gradient(intensity):
    """RawImage.cpp:55-82: central differences x 0.5, zero on the first / last row and column.  Returns
    (gradient_ interleaved (dx, dy) per pixel, flat 2 h w; gradient_square flat h w).  On 8-bit input every value is a
    multiple of 0.25 below 2^16: exact in float32, so no contraction can change it."""
    I = np.asarray(intensity, F32)
    h, w = I.shape
    dx = np.zeros((h, w), F32)
    dy = np.zeros((h, w), F32)
    if h > 2 and w > 2:
        dx[1:-1, 1:-1] = F32(0.5) * (I[1:-1, 2:] - I[1:-1, :-2])
        dy[1:-1, 1:-1] = F32(0.5) * (I[2:, 1:-1] - I[:-2, 1:-1])
    g2 = dx * dx + dy * dy
    return np.stack([dx, dy], axis=-1).reshape(-1), g2.reshape(-1)


def _hist_quantile(hist, below=0.5):
    """computeHistQuantil (CvoPixelSelector.cpp:72-80): hist[0] = count, hist[1 + g] = bin g; 90 bins are scanned."""
    th = int(F32(hist[0]) * F32(below) + F32(0.5))
    for i in range(90):
        th -= int(hist[i + 1])
        if th < 0:
            return i
    return 90


def thresholds(g2, h, w):
    """makeHists (CvoPixelSelector.cpp:83-148): (ths, thsSmoothed, thsStep); both arrays have (w/32)(h/32) + 100
    zero-initialised entries (:62-63)."""
    w32, h32 = w // 32, h // 32
    size = w32 * h32 + 100
    ths = np.zeros(size, F32)
    sm = np.zeros(size, F32)
    G = np.asarray(g2, F32).reshape(h, w)
    for y in range(h32):
        for x in range(w32):
            blk = G[32 * y:32 * y + 32, 32 * x:32 * x + 32]
            jt, it = np.meshgrid(np.arange(32) + 32 * y, np.arange(32) + 32 * x, indexing="ij")
            ok = ~((it > w - 2) | (jt > h - 2) | (it < 1) | (jt < 1))
            g = np.sqrt(blk[ok]).astype(np.int64)  # int g = sqrtf(.): truncation of the correctly rounded root
            g = np.minimum(g, 48)
            hist = np.zeros(100, np.int64)
            hist[0] = g.shape[0]
            hist[1:50] = np.bincount(g, minlength=49)[:49]
            ths[x + y * w32] = F32(_hist_quantile(hist) + 7)
    for y in range(h32):
        for x in range(w32):
            s, n = F32(0), F32(0)
            for yy in (y - 1, y, y + 1):
                for xx in (x - 1, x, x + 1):
                    if 0 <= xx < w32 and 0 <= yy < h32:
                        n += F32(1)
                        s += ths[xx + yy * w32]  # (small integers: the order of the sum does not matter)
            m = F32(s / n)
            sm[x + y * w32] = F32(m * m)
    return ths, sm, w32


def threshold_index(h, w):
    """(h, w) int array: (x >> 5) + (y >> 5) * thsStep, read literally (CvoPixelSelector.cpp:355).  QUIRK: when w or h is
    not a multiple of 32 this aliases into the next block row or into the zero slack of the allocation."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return (x >> 5) + (y >> 5) * (w // 32)


def considered(h, w):
    """Pixels select() looks at: 4 <= x < w - 5, 4 <= y <= h - 4 (:352)."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return (x >= 4) & (x < w - 5) & (y >= 4) & (y <= h - 4)


def select(g2, sm, h, w, pot):
    """select (CvoPixelSelector.cpp:270-426) at thFactor = 1 with the direction distribution off: per pot x pot cell the
    first pixel in row-major order within the cell with the largest g2 strictly above its threshold; output in the
    reference's nesting - blocks of 4 pot, then 2 pot, then pot, each row-major, clipped at the image edge.  The random
    pattern only picks a direction that is not used, and the heat map's sub-selection does not touch output_uv: rand()
    is not modelled.  Returns pixel indices v * w + u."""
    G = np.asarray(g2, F32).reshape(h, w)
    ok = considered(h, w)
    idx = threshold_index(h, w)
    if ok.any() and int(idx[ok].max()) >= sm.shape[0]:
        raise Unsupported("threshold index leaves the allocation")
    th = sm[np.minimum(idx, sm.shape[0] - 1)]
    val = np.where(ok & (G > th), G, F32(-1))
    ncy, ncx = -(-h // pot), -(-w // pot)
    pad = np.full((ncy * pot, ncx * pot), F32(-1))
    pad[:h, :w] = val
    cells = pad.reshape(ncy, pot, ncx, pot).transpose(0, 2, 1, 3).reshape(ncy, ncx, pot * pot)
    arg = np.argmax(cells, axis=2)  # (the first of equal maxima: `dirNorm > bestVal2` is strict)
    best = np.take_along_axis(cells, arg[..., None], axis=2)[..., 0]
    cy, cx = np.meshgrid(np.arange(ncy), np.arange(ncx), indexing="ij")
    py, px = cy * pot + arg // pot, cx * pot + arg % pot
    nbx = -(-w // (4 * pot))
    key = ((((cy // 4) * nbx + cx // 4) * 2 + (cy % 4) // 2) * 2 + (cx % 4) // 2) * 4 + (cy % 2) * 2 + cx % 2
    hit = best > 0
    order = np.argsort(key[hit], kind="stable")
    return (py[hit] * w + px[hit])[order].astype(np.int32)


def dso_select(intensity):
    """dso_select_pixels (CvoPixelSelector.cpp:430-453) with num_want = 10000: returns (pixel indices, potentials tried,
    count at every potential tried).  recursionsLeft is 0 in every call: makeHeatMaps never recurses."""
    h, w = intensity.shape
    _, g2 = gradient(intensity)
    _, sm, _ = thresholds(g2, h, w)
    tried, counts = [3], []
    uv = select(g2, sm, h, w, 3)
    counts.append(len(uv))
    times = 1
    while len(uv) > NUM_WANT:
        uv = select(g2, sm, h, w, 3 + times)
        tried.append(3 + times)
        counts.append(len(uv))
        times += 1
        if times == 5:
            break
    if len(uv) < NUM_WANT // 3 * 2:
        uv = select(g2, sm, h, w, 3 + times - 2)
        tried.append(3 + times - 2)
        counts.append(len(uv))
    return uv, tried, counts


def candidates(image, gray, method):
    """select_points_from_image for RGBD (CvoPointCloud.cpp:320-375): (pixel indices, geometric type of the method).
    FULL: QUIRK column-major, u outer over columns, v inner over rows."""
    image = np.asarray(image)
    h, w = image.shape[:2]
    if method == FULL:
        u, v = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
        return (v * w + u).reshape(-1).astype(np.int32), (F32(0.5), F32(0.5)), None
    uv, tried, counts = dso_select(gray_plane(image, gray))
    return uv, (F32(0.9), F32(0.1)), (tried, counts)


def points(image, gray, depth, calib, semantic, method):
    """CvoPointCloud(ImageRGBD, Calibration, method) (CvoPointCloud.cpp:459-553).  Returns a dict: pixel (n,), xyz (n, 3),
    feat (n, channels + 2), label (n, num_classes) or None, geotype (n, 2), schedule (tried, counts) or None."""
    image = np.asarray(image, np.uint8)
    h, w = image.shape[:2]
    ch = 1 if image.ndim == 2 else 3
    fx, fy, cx, cy, scale = (F32(c) for c in calib)
    pix, gt, schedule = candidates(image, gray, method)
    dep = np.asarray(depth).reshape(-1)[pix]
    keep = (dep != 0) & ~np.isnan(dep.astype(F32))
    if semantic is not None:
        sem = np.asarray(semantic, F32).reshape(h * w, -1)
        keep &= np.argmax(sem[pix], axis=1) != 10  # (maxCoeff: the first maximum; class 10 = unlabeled)
    pix = pix[keep]
    dep = dep[keep]
    u, v = (pix % w).astype(F32), (pix // w).astype(F32)
    z = (dep.astype(F32) / scale).astype(F32)
    x = (((u - cx) * z).astype(F32) / fx).astype(F32)
    y = (((v - cy) * z).astype(F32) / fy).astype(F32)
    grad, _ = gradient(gray_plane(image, gray))
    colour = image.reshape(h * w, ch)[pix].astype(F32)
    feat = np.zeros((len(pix), ch + 2), F32)
    feat[:, :ch] = (colour.astype(np.float64) / 255.0).astype(F32)
    # QUIRK: the interleaved gradient array is indexed with the PIXEL index (v w + u and v w + u + 1), not 2 (v w + u)
    feat[:, ch] = (grad[pix].astype(np.float64) / 500.0 + 0.5).astype(F32)
    feat[:, ch + 1] = (grad[pix + 1].astype(np.float64) / 500.0 + 0.5).astype(F32)
    return dict(pixel=pix.astype(np.int32), xyz=np.stack([x, y, z], axis=1).astype(F32), feat=feat,
                label=None if semantic is None else sem[pix].copy(),
                geotype=np.tile(np.array([gt], F32), (len(pix), 1)), schedule=schedule,
                with_depth=int(np.count_nonzero((np.asarray(depth).reshape(-1) != 0) & ~np.isnan(np.asarray(depth, F32).reshape(-1)))))


def byte_round_trip(f):
    """export_to_pcd<PointXYZRGB> (CvoPointCloud.cpp:1237-1239): min(255, int(f * 255)) on float32."""
    return np.minimum(255, (np.asarray(f, F32) * F32(255)).astype(np.int64)).astype(np.uint8)


def voxel_reference(xyz, s):
    """The cvo_voxel_select contract: of every occupied voxel k = rint(x / s) the lowest index, ascending."""
    k = np.rint(np.asarray(xyz, F32).reshape(-1, 3) / F32(s)).astype(np.int64)
    if k.shape[0] == 0:
        return np.zeros(0, np.int64)
    _, first = np.unique(k, axis=0, return_index=True)
    return np.sort(first)


def recipe(image, gray, depth, calib, semantic, leaf, edge_divisor=4):
    """The multi-frame drivers' per-frame block (main_multi_frame_irls_tum.cpp:279-335): FULL and DSO_EDGES clouds, each
    exported to XYZRGB bytes, voxel-selected with leaf / edge_divisor (edge) and leaf (surface), rebuilt by the
    (XYZRGB, GeometryType) constructor (CvoPointCloud.cpp:598-630: F = 5, features (b, g, r) / 255, 0, 0 from the
    exported bytes - feature k of the first three comes back from byte k) and concatenated edge first.
    Returns a dict: pixel, is_edge, xyz, feat (n, 5), geotype; counts of the stages."""
    out = []
    stats = {}
    for method, s, gt in ((DSO_EDGES, F32(leaf) / F32(edge_divisor), (1.0, 0.0)), (FULL, F32(leaf), (0.0, 1.0))):
        p = points(image, gray, depth, calib, semantic, method)
        kept = voxel_reference(p["xyz"], s)
        f3 = np.zeros((len(kept), 3), F32)
        k = min(3, p["feat"].shape[1])
        f3[:, :k] = p["feat"][kept, :k]
        b = byte_round_trip(f3)
        feat = np.zeros((len(kept), 5), F32)
        feat[:, :3] = (b.astype(np.int32).astype(F32).astype(np.float64) / 255.0).astype(F32)
        out.append((p["pixel"][kept], p["xyz"][kept], feat, np.tile(np.array([gt], F32), (len(kept), 1))))
        stats["edge" if method == DSO_EDGES else "surface"] = dict(candidates=len(p["pixel"]), kept=len(kept), schedule=p["schedule"])
        stats["with_depth"] = p["with_depth"]
    ne = len(out[0][0])
    return dict(pixel=np.concatenate([out[0][0], out[1][0]]).astype(np.int32),
                is_edge=np.concatenate([np.ones(ne, np.uint8), np.zeros(len(out[1][0]), np.uint8)]),
                xyz=np.concatenate([out[0][1], out[1][1]]), feat=np.concatenate([out[0][2], out[1][2]]),
                geotype=np.concatenate([out[0][3], out[1][3]]), stats=stats)
