"""numpy statement of the stereo front end (cvo_stereo_points / cvo_cloud_upload_stereo / _recipe): the reference's
CvoPointCloud(ImageStereo, Calibration, method) (CvoPointCloud.cpp:680-773, StaticStereo.cpp:84-107, is_good_point :39-49)
from a GIVEN disparity map, and the multi-frame KITTI driver's per-frame block (main_multi_frame_irls_kitti.cpp:235-292).
Reuses np_rgbd for the gray plane, the gradient, the DSO selector and the voxel recipe, np_fast for CV_FAST.  Shares no
code with the library.  Frames are plain arrays as in np_rgbd, with

    disparity  (h, w) float32, left disparity in pixels (libelas codes invalid pixels as -10)
    calib      (fx, fy, cx, cy, baseline)
"""
import numpy as np

import np_fast
import np_rgbd

CV_FAST, DSO_EDGES, FULL = 0, 2, 8  # cvo::CvoPointCloud::PointSelectionMethod
F32 = np.float32
TOP, BOTTOM = 100, 30  # is_good_point: 100 <= v <= h - 30: a frame with fewer than 130 rows yields no points


def candidates(image, gray, method, has_classes):
    """select_points_from_image(left, STEREO, method): (pixel indices, geometric type, schedule or None).  DSO_EDGES and FULL
    are exactly the RGB-D candidates; CV_FAST has type (1, 0) (CvoPointCloud.cpp:310-311) and num_want 28000 with classes."""
    if method != CV_FAST:
        return np_rgbd.candidates(image, gray, method)
    plane = np_rgbd.gray_plane(image, gray).astype(np.uint8)
    pix, used, tried, counts = np_fast.select(plane, np_fast.STEREO_SEMANTIC if has_classes else np_fast.STEREO)
    return pix, (F32(1), F32(0)), (tried, counts, used)


def back_project(u, v, disp, calib):
    """pt_depth_from_disparity's arithmetic in float32, every operation rounded on its own (numpy does not contract):
    depth = |baseline| fx / disparity; xyz = (Kinv (u, v, 1)) depth with Eigen 3.3's size-3 cofactor inverse of
    K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]], each row's dot product summed left to right (the zero entries add +-0),
    each component then multiplied by depth; norm = sqrt((x x + y y) + z z)."""
    fx, fy, cx, cy, baseline = (F32(c) for c in calib)
    with np.errstate(all="ignore"):
        depth = (np.abs(baseline) * fx) / disp.astype(F32)
        invdet = F32(1) / (fx * fy)
        k00, k11 = fy * invdet, fx * invdet
        k02, k12, k22 = -(cx * fy) * invdet, -(fx * cy) * invdet, (fx * fy) * invdet
        x = (k00 * u.astype(F32) + k02) * depth
        y = (k11 * v.astype(F32) + k12) * depth
        z = k22 * depth
        norm = np.sqrt((x * x + y * y) + z * z)
    xyz = np.stack([x, y, z], axis=1).astype(F32)
    assert xyz.dtype == F32 and norm.dtype == F32
    return xyz, norm


def keep_mask(u, v, disp, norm, h, w):
    """TraceStatus GOOD and is_good_point.  `disparity <= 0.05` promotes to double: it rejects exactly the floats below
    0.05f, and 0.05f itself (0.0500000007...) is kept.  A NaN disparity fails no test."""
    with np.errstate(all="ignore"):
        oob = (u < 1) | (u > w - 2) | (v < 1) | (v > h - 2)
        outlier = disp.astype(np.float64) <= 0.05
        bad = (u < 2) | (u > w - 2) | (v < TOP) | (v > h - BOTTOM) | (norm >= F32(55))
    return ~oob & ~outlier & ~bad


def points(image, gray, disparity, calib, semantic, method):
    """The constructor.  Returns a dict: pixel (n,), xyz (n, 3), feat (n, channels + 2), label or None, geotype (n, 2),
    schedule, candidates (pixels the predicate saw)."""
    image = np.asarray(image, np.uint8)
    h, w = image.shape[:2]
    ch = 1 if image.ndim == 2 else 3
    pix, gt, sched = candidates(image, gray, method, semantic is not None)
    pix = np.asarray(pix, np.int64)
    u, v = pix % w, pix // w
    disp = np.asarray(disparity, F32).reshape(-1)[pix]
    xyz, norm = back_project(u, v, disp, calib)
    keep = keep_mask(u, v, disp, norm, h, w)
    if semantic is not None:
        sem = np.asarray(semantic, F32).reshape(h * w, -1)
        keep &= np.argmax(sem[pix], axis=1) != 10
    n_cand = len(pix)
    pix, xyz = pix[keep], xyz[keep]
    grad, _ = np_rgbd.gradient(np_rgbd.gray_plane(image, gray))
    feat = np.zeros((len(pix), ch + 2), F32)
    feat[:, :ch] = (image.reshape(h * w, ch)[pix].astype(F32).astype(np.float64) / 255.0).astype(F32)
    # QUIRK (as in the RGB-D constructor): the interleaved gradient array is indexed with the PIXEL index
    feat[:, ch] = (grad[pix].astype(np.float64) / 500.0 + 0.5).astype(F32)
    feat[:, ch + 1] = (grad[pix + 1].astype(np.float64) / 500.0 + 0.5).astype(F32)
    return dict(pixel=pix.astype(np.int32), xyz=xyz, feat=feat, label=None if semantic is None else sem[pix].copy(),
                geotype=np.tile(np.array([gt], F32), (len(pix), 1)), schedule=sched, candidates=n_cand)


def recipe(image, gray, disparity, calib, semantic, leaf, edge_divisor=5):
    """The multi-frame KITTI driver's block: np_rgbd.recipe's steps on the stereo points - DSO_EDGES and FULL clouds, exported to
    XYZRGB bytes, voxel-selected with leaf / edge_divisor (the driver: 5) and leaf, rebuilt as EDGE / SURFACE colour points,
    edge first."""
    out, stats = [], dict(candidates=0, kept=0)
    for method, s, gt in ((DSO_EDGES, F32(leaf) / F32(edge_divisor), (1.0, 0.0)), (FULL, F32(leaf), (0.0, 1.0))):
        p = points(image, gray, disparity, calib, semantic, method)
        kept = np_rgbd.voxel_reference(p["xyz"], s)
        f3 = np.zeros((len(kept), 3), F32)
        k = min(3, p["feat"].shape[1])
        f3[:, :k] = p["feat"][kept, :k]
        feat = np.zeros((len(kept), 5), F32)
        feat[:, :3] = (np_rgbd.byte_round_trip(f3).astype(np.int32).astype(F32).astype(np.float64) / 255.0).astype(F32)
        out.append((p["pixel"][kept], p["xyz"][kept], feat, np.tile(np.array([gt], F32), (len(kept), 1))))
        stats["candidates"] += p["candidates"]
        stats["kept"] += len(p["pixel"])
        if method == DSO_EDGES:
            stats["schedule"] = p["schedule"]
    ne = len(out[0][0])
    return dict(pixel=np.concatenate([out[0][0], out[1][0]]).astype(np.int32),
                is_edge=np.concatenate([np.ones(ne, np.uint8), np.zeros(len(out[1][0]), np.uint8)]),
                xyz=np.concatenate([out[0][1], out[1][1]]), feat=np.concatenate([out[0][2], out[1][2]]),
                geotype=np.concatenate([out[0][3], out[1][3]]), stats=stats)
