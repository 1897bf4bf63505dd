"""numpy statement of the device-frame RGB-D front end (cvo_cloud_from_rgbd_device / _recipe, cvo_rgbd_frame_rows_host): the
rows of np_rgbd.points / np_rgbd.recipe as a RESIDENT cloud holds them - features zero-padded to 5 columns, class scores to
19 - and the exclusion rule over STRIDED scores.  Shares no code with the library.

A frame's class scores may come in any view: `layout` "hwc" (rows, cols, classes) or "chw" (classes, rows, cols), with any
numpy strides (a transposed view, a column slice of a wider array).  The statement reads them through numpy's indexing."""
import numpy as np

import np_rgbd

FEATURES, CLASSES, EXCLUDED_CLASS = 5, 19, 10
F32 = np.float32


def hwc(semantic, layout="hwc"):
    """The scores as an (h, w, classes) view, whatever the layout."""
    if semantic is None:
        return None
    s = np.asarray(semantic)
    return s if layout == "hwc" else np.moveaxis(s, 0, 2)


def first_maximum(scores):
    """(h, w) class index of the FIRST maximum under `row[c] > row[best]` from best = 0 (CvoPointCloud.cpp:501-507): equal
    scores keep the earlier class.  (For rows without NaN this is np.argmax; a NaN's behaviour is not stated here.)"""
    s = np.asarray(scores, F32)
    best = np.zeros(s.shape[:2], np.int64)
    val = s[..., 0].copy()
    for c in range(1, s.shape[2]):
        better = s[..., c] > val
        best[better] = c
        val[better] = s[..., c][better]
    return best


def excluded(semantic, layout="hwc"):
    """(h * w,) bool: the pixel's first-maximum class is 10.  Without scores nothing is excluded."""
    s = hwc(semantic, layout)
    return first_maximum(s).reshape(-1) == EXCLUDED_CLASS


def pad(a, width):
    a = np.asarray(a, F32)
    out = np.zeros((a.shape[0], width), F32)
    out[:, :a.shape[1]] = a
    return out


def points(image, gray, depth, calib, semantic, method, layout="hwc"):
    """np_rgbd.points as the resident cloud holds it: pixel, xyz, feat (n, 5), label (n, 19) or None, geotype."""
    s = hwc(semantic, layout)
    p = np_rgbd.points(image, gray, depth, calib, None if s is None else np.ascontiguousarray(s), method)
    return dict(pixel=p["pixel"], xyz=p["xyz"], feat=pad(p["feat"], FEATURES), label=None if p["label"] is None else pad(p["label"], CLASSES),
                geotype=p["geotype"], schedule=p["schedule"], with_depth=p["with_depth"])


def recipe(image, gray, depth, calib, semantic, leaf, edge_divisor=4, layout="hwc"):
    """np_rgbd.recipe (its rows have 5 features and no labels already)."""
    s = hwc(semantic, layout)
    return np_rgbd.recipe(image, gray, depth, calib, None if s is None else np.ascontiguousarray(s), leaf, edge_divisor)


def labels_of(semantic, pixel, layout="hwc"):
    """(n, 19) zero-padded scores of the given pixels."""
    s = hwc(semantic, layout)
    h, w, c = s.shape
    pixel = np.asarray(pixel, np.int64)
    return pad(s[pixel // w, pixel % w, :], CLASSES)
