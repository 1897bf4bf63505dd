"""Python mirror of the reference's operator interface for the path (cvo::CvoGPU, cvo::CvoPointCloud;
include/UnifiedCvo/cvo/CvoGPU.hpp:49-229, utils/CvoPointCloud.hpp:126-188), over the C-ABI.

This is the harness used by tests/ and bench.py; the C++ veneer with the same names lives in
include/UnifiedCvo/.  All compute happens in libcvo_hip.so on the GPU.
"""
import collections
import ctypes as C
import weakref
import os

import numpy as np

from . import _capi
from .params import CvoParams, read_cvo_params_yaml
from .synth import FEATURE_DIMENSIONS, NUM_CLASSES


class CvoError(RuntimeError):
    pass


def _fptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


class CvoPointCloud:
    """Host container: positions (n,3), features (n,F), labels (n,C), geometric_types (n,2)."""

    def __init__(self, feature_dimensions=0, num_classes=0):
        self.num_points_ = 0
        self.feature_dimensions_ = feature_dimensions
        self.num_classes_ = num_classes
        self.positions_ = np.zeros((0, 3), np.float32)
        self.features_ = np.zeros((0, feature_dimensions), np.float32)
        self.labels_ = np.zeros((0, num_classes), np.float32)
        self.geometric_types_ = np.zeros((0, 2), np.float32)
        self._reserved = False

    # -- constructors mirroring the pcl ones (CvoPointCloud.cpp:569-652) -------------------------
    @classmethod
    def from_xyz(cls, xyz):
        """pcl::PointXYZ constructor: F = 0, geometric_type = (1, 0) (CvoPointCloud.cpp:633-652)."""
        pc = cls(0, 0)
        pc.positions_ = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        pc.num_points_ = pc.positions_.shape[0]
        pc.geometric_types_ = np.tile(np.array([[1.0, 0.0]], np.float32), (pc.num_points_, 1))
        pc._reserved = True
        return pc

    @classmethod
    def from_xyzrgb(cls, xyz, rgb_u8):
        """pcl::PointXYZRGB constructor: features (r,g,b)/255,0,0; type (0,1) (CvoPointCloud.cpp:569-594)."""
        pc = cls(5, 0)
        pc.positions_ = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        pc.num_points_ = pc.positions_.shape[0]
        f = np.zeros((pc.num_points_, 5), np.float32)
        f[:, :3] = (np.asarray(rgb_u8).astype(np.int32).astype(np.float32) / np.float32(255.0))
        pc.features_ = f
        pc.geometric_types_ = np.tile(np.array([[0.0, 1.0]], np.float32), (pc.num_points_, 1))
        pc._reserved = True
        return pc

    @classmethod
    def from_arrays(cls, xyz, features=None, labels=None, geometric_types=None):
        n = np.asarray(xyz).reshape(-1, 3).shape[0]
        F = 0 if features is None else np.asarray(features).shape[1]
        Cn = 0 if labels is None else np.asarray(labels).shape[1]
        pc = cls(F, Cn)
        pc.reserve(n, F, Cn)
        pc.positions_[:] = np.asarray(xyz, np.float32).reshape(-1, 3)
        if F:
            pc.features_[:] = features
        if Cn:
            pc.labels_[:] = labels
        if geometric_types is not None:
            pc.geometric_types_[:] = geometric_types
        return pc

    # -- reserve / add_point (CvoPointCloud.cpp:1384-1420) ----------------------------------------
    def reserve(self, num_points, feature_dims, num_classes):
        self.num_points_ = num_points
        self.feature_dimensions_ = feature_dims
        self.num_classes_ = num_classes
        self.positions_ = np.zeros((num_points, 3), np.float32)
        self.features_ = np.zeros((num_points, feature_dims), np.float32)
        self.labels_ = np.zeros((num_points, num_classes), np.float32)
        self.geometric_types_ = np.zeros((num_points, 2), np.float32)
        self._reserved = True

    def add_point(self, index, xyz, feature, label, geometric_type):
        if index >= self.num_points_:
            return -1
        if (not self._reserved or self.features_.shape[0] < self.num_points_
                or self.features_.shape[1] != self.feature_dimensions_ or len(geometric_type) != 2):
            return -1
        self.positions_[index] = xyz
        if self.feature_dimensions_:
            self.features_[index] = feature
        if self.num_classes_:
            self.labels_[index] = label
        self.geometric_types_[index] = geometric_type
        return 0

    # -- getters (CvoPointCloud.hpp:140-154) ------------------------------------------------------
    def num_points(self):
        return self.num_points_

    size = num_points

    def num_classes(self):
        return self.num_classes_

    def num_features(self):
        return self.feature_dimensions_

    feature_dimensions = num_features

    def positions(self):
        return self.positions_

    def features(self):
        return self.features_

    def labels(self):
        return self.labels_

    semantics = labels

    # label_at / feature_at / geometry_type_at (CvoPointCloud.hpp:141-143, CvoPointCloud.cpp:1282-1286): rows by value
    def label_at(self, index):
        return np.array(self.labels_[index], dtype=np.float32)

    def feature_at(self, index):
        return np.array(self.features_[index], dtype=np.float32)

    def geometry_type_at(self, index):
        return np.array(self.geometric_types_.reshape(-1)[2 * index:2 * index + 2], dtype=np.float32)

    def geometric_types(self):
        return self.geometric_types_.reshape(-1)

    @staticmethod
    def transform(pose, inp, out):
        """static CvoPointCloud::transform (CvoPointCloud.cpp:1366-1382); feature_dimensions_ is not copied."""
        P = np.asarray(pose, np.float32).reshape(4, 4)
        out.num_points_ = inp.num_points_
        out.num_classes_ = inp.num_classes_
        out.features_ = inp.features_.copy()
        out.labels_ = inp.labels_.copy()
        out.positions_ = (inp.positions_ @ P[:3, :3].T + P[:3, 3]).astype(np.float32)
        out.geometric_types_ = inp.geometric_types_.copy()
        out._reserved = True

    def __add__(self, other):
        """operator+ concatenation (CvoPointCloud.cpp:1139-1151)."""
        r = CvoPointCloud(self.feature_dimensions_, self.num_classes_)
        r.num_points_ = self.num_points_ + other.num_points_
        r.positions_ = np.concatenate([self.positions_, other.positions_])
        r.features_ = np.concatenate([self.features_, other.features_]) if self.feature_dimensions_ else self.features_
        r.labels_ = np.concatenate([self.labels_, other.labels_]) if self.num_classes_ else self.labels_
        r.geometric_types_ = np.concatenate([self.geometric_types_, other.geometric_types_])
        r._reserved = True
        return r

    def select(self, indices):
        """A new cloud of the rows `indices`, in that order (what a voxel selection keeps)."""
        idx = np.asarray(indices, np.int64).reshape(-1)
        r = CvoPointCloud(self.feature_dimensions_, self.num_classes_)
        r.num_points_ = int(idx.shape[0])
        r.positions_ = np.ascontiguousarray(self.positions_[idx])
        r.features_ = np.ascontiguousarray(self.features_[idx]) if self.features_.shape[0] == self.num_points_ else self.features_
        r.labels_ = np.ascontiguousarray(self.labels_[idx]) if self.labels_.shape[0] == self.num_points_ else self.labels_
        r.geometric_types_ = np.ascontiguousarray(self.geometric_types_.reshape(-1, 2)[idx])
        r._reserved = True
        return r

    # -- what CvoPointCloud_to_gpu builds per point (CvoGPU_impl.cu:206-263) ----------------------
    def device_arrays(self):
        n = self.num_points_
        xyz = np.ascontiguousarray(self.positions_, np.float32)
        feat = None
        if self.features_.shape[0] == n and self.features_.shape[1] > 0:
            feat = np.zeros((n, FEATURE_DIMENSIONS), np.float32)
            k = min(FEATURE_DIMENSIONS, self.features_.shape[1])
            feat[:, :k] = self.features_[:, :k]
        label = None
        if self.num_classes_ > 0:
            label = np.zeros((n, NUM_CLASSES), np.float32)
            k = min(NUM_CLASSES, self.labels_.shape[1])
            label[:, :k] = self.labels_[:, :k]
        geo = np.ascontiguousarray(self.geometric_types_, np.float32).reshape(n, 2)
        return xyz, feat, label, geo


class RGBDFrame:
    """What cvo::ImageRGBD<DepthType> and cvo::Calibration hold of one RGB-D frame (cvo_rgbd_frame_t): `image` (rows, cols)
    or (rows, cols, 3) uint8 in BGR order, as RawImage holds it AFTER its denoising (CvoGPU.nlm_denoise / nlm_denoise_lab); `depth` (rows, cols) uint16 or float32;
    the intrinsics and the depth scaling factor; optionally the 8-bit `gray` plane the gradient is taken of (overrides the
    BGR -> gray formula) and `semantic` (rows, cols, num_classes) float32."""

    def __init__(self, image, depth, fx, fy, cx, cy, scaling_factor, gray=None, semantic=None):
        self.image = np.ascontiguousarray(image, np.uint8)
        if self.image.ndim == 3 and self.image.shape[2] == 1:
            self.image = np.ascontiguousarray(self.image[..., 0])
        self.rows, self.cols = self.image.shape[:2]
        self.channels = 1 if self.image.ndim == 2 else self.image.shape[2]
        depth = np.asarray(depth)
        self.depth = np.ascontiguousarray(depth, np.uint16 if depth.dtype == np.uint16 else np.float32)
        if self.depth.shape != (self.rows, self.cols):
            raise ValueError(f"depth is {self.depth.shape}, the image {self.rows} x {self.cols}")
        self.fx, self.fy, self.cx, self.cy, self.scaling_factor = (float(v) for v in (fx, fy, cx, cy, scaling_factor))
        self.gray = None if gray is None else np.ascontiguousarray(gray, np.uint8).reshape(self.rows, self.cols)
        self.semantic = None if semantic is None else np.ascontiguousarray(semantic, np.float32).reshape(self.rows, self.cols, -1)
        self.num_classes = 0 if self.semantic is None else self.semantic.shape[2]

    def c_struct(self):
        """cvo_rgbd_frame_t over this frame's arrays (which must outlive it)."""
        ptr = lambda a: None if a is None else a.ctypes.data
        return _capi.cvo_rgbd_frame_t(self.rows, self.cols, self.channels, ptr(self.image), ptr(self.gray), ptr(self.depth),
                                      _capi.CVO_DEPTH_U16 if self.depth.dtype == np.uint16 else _capi.CVO_DEPTH_F32,
                                      self.fx, self.fy, self.cx, self.cy, self.scaling_factor, self.num_classes, ptr(self.semantic))


FULL, DSO_EDGES = _capi.CVO_SELECT_FULL, _capi.CVO_SELECT_DSO_EDGES  # cvo::CvoPointCloud::PointSelectionMethod


def _rgbd_points(call, frame, method):
    """Shared by CvoGPU.rgbd_points and rgbd_points_host: runs `call(frame struct, method, outputs...)` -> (rc, cloud)."""
    n_max = max(frame.rows * frame.cols, 1)
    F, nc = frame.channels + 2, frame.num_classes
    pixel = np.zeros(n_max, np.int32)
    xyz, feat, geo = np.zeros((n_max, 3), np.float32), np.zeros((n_max, F), np.float32), np.zeros((n_max, 2), np.float32)
    label = np.zeros((n_max, nc), np.float32) if nc else None
    n = C.c_int()
    fs = frame.c_struct()
    rc = call(C.byref(fs), int(method), pixel.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n), _fptr(xyz), _fptr(feat), _fptr(label), _fptr(geo))
    if rc != 0:
        return rc, None
    k = n.value
    pc = CvoPointCloud.from_arrays(xyz[:k], feat[:k], None if label is None else label[:k], geo[:k])
    pc.pixel = pixel[:k].copy()
    return rc, pc


def rgbd_points_host(frame, method):
    """cvo_rgbd_points_host: the CPU twin of CvoGPU.rgbd_points, no context."""
    L = _capi.lib()
    rc, pc = _rgbd_points(L.cvo_rgbd_points_host, frame, method)
    if rc != 0:
        e = CvoError(f"error {rc}: cvo_rgbd_points_host refused the frame or the method")
        e.code = rc
        raise e
    return pc


CV_FAST = _capi.CVO_SELECT_CV_FAST
FAST_RGBD, FAST_STEREO, FAST_STEREO_SEMANTIC = _capi.CVO_FAST_RGBD, _capi.CVO_FAST_STEREO, _capi.CVO_FAST_STEREO_SEMANTIC


class StereoFrame:
    """What cvo::ImageStereo and cvo::Calibration hold of one stereo frame (cvo_stereo_frame_t): the LEFT `image` (rows, cols)
    or (rows, cols, 3) uint8 in BGR order, after RawImage's denoising (CvoGPU.nlm_denoise / nlm_denoise_lab); the left `disparity` (rows, cols) float32 in pixels,
    from the caller's matcher (upstream: libelas, invalid = -10) or from CvoGPU.stereo_disparity - the library's own matcher, another
    algorithm than libelas -; the intrinsics and the baseline; optionally the 8-bit `gray`
    plane and `semantic` (rows, cols, num_classes) float32, as in RGBDFrame."""

    def __init__(self, image, disparity, fx, fy, cx, cy, baseline, gray=None, semantic=None):
        self.image = np.ascontiguousarray(image, np.uint8)
        if self.image.ndim == 3 and self.image.shape[2] == 1:
            self.image = np.ascontiguousarray(self.image[..., 0])
        self.rows, self.cols = self.image.shape[:2]
        self.channels = 1 if self.image.ndim == 2 else self.image.shape[2]
        self.disparity = None if disparity is None else np.ascontiguousarray(disparity, np.float32)  # (None: for CvoGPU.upload_stereo_pair only)
        if self.disparity is not None and self.disparity.shape != (self.rows, self.cols):
            raise ValueError(f"disparity is {self.disparity.shape}, the image {self.rows} x {self.cols}")
        self.fx, self.fy, self.cx, self.cy, self.baseline = (float(v) for v in (fx, fy, cx, cy, baseline))
        self.gray = None if gray is None else np.ascontiguousarray(gray, np.uint8).reshape(self.rows, self.cols)
        self.semantic = None if semantic is None else np.ascontiguousarray(semantic, np.float32).reshape(self.rows, self.cols, -1)
        self.num_classes = 0 if self.semantic is None else self.semantic.shape[2]

    def c_struct(self):
        """cvo_stereo_frame_t over this frame's arrays (which must outlive it)."""
        ptr = lambda a: None if a is None else a.ctypes.data
        return _capi.cvo_stereo_frame_t(self.rows, self.cols, self.channels, ptr(self.image), ptr(self.gray), ptr(self.disparity),
                                        self.fx, self.fy, self.cx, self.cy, self.baseline, self.num_classes, ptr(self.semantic))


def _raise(rc, text):
    e = CvoError(f"error {rc}: {text}")
    e.code = rc
    raise e


def _fast_select(call, gray, schedule):
    """Shared by CvoGPU.fast_select and fast_select_host -> (rc, pixel indices, threshold used)."""
    gray = np.ascontiguousarray(gray, np.uint8)
    rows, cols = gray.shape
    pixel = np.zeros(max(rows * cols, 1), np.int32)
    n, used = C.c_int(), C.c_int()
    sched = _capi.cvo_fast_schedule_t(*[int(v) for v in schedule])
    rc = call(rows, cols, gray.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(sched), pixel.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n), C.byref(used))
    return rc, pixel[:n.value].copy(), used.value


def fast_select_host(gray, schedule=FAST_STEREO):
    """cvo_fast_select_host: the CV_FAST selection of an 8-bit gray plane under `schedule` (thresh, num_want, num_min,
    break_thresh) on one CPU thread -> (pixel indices v * cols + u in row-major order, the threshold whose keypoints stand)."""
    rc, pixel, used = _fast_select(_capi.lib().cvo_fast_select_host, gray, schedule)
    if rc != 0:
        _raise(rc, "cvo_fast_select_host refused the plane or the schedule")
    return pixel, used


def stereo_points_host(frame, method=CV_FAST):
    """cvo_stereo_points_host: the CPU twin of CvoGPU.stereo_points, no context."""
    rc, pc = _rgbd_points(_capi.lib().cvo_stereo_points_host, frame, method)
    if rc != 0:
        _raise(rc, "cvo_stereo_points_host refused the frame or the method")
    return pc


class SGMConfig:
    """cvo_sgm_config_t: the stereo matcher's configuration (semi-global matching over a census cost; tests/np_sgm.py states it).
    max_disparity 64 / 128 / 256, 0 <= p1 <= p2 <= 193, uniqueness 0 .. 99 percent, lr_max_diff < 0 turns the left-right check
    off, paths 4 or 8."""

    def __init__(self, max_disparity=128, p1=10, p2=120, uniqueness=5, lr_max_diff=1, paths=8):
        self.max_disparity, self.p1, self.p2 = int(max_disparity), int(p1), int(p2)
        self.uniqueness, self.lr_max_diff, self.paths = int(uniqueness), int(lr_max_diff), int(paths)

    def c_struct(self):
        return _capi.cvo_sgm_config_t(self.max_disparity, self.p1, self.p2, self.uniqueness, self.lr_max_diff, self.paths)


def _stereo_disparity(call, left, right, config):
    """Shared by CvoGPU.stereo_disparity and stereo_disparity_host -> (rc, disparity (rows, cols) float32)."""
    left, right = np.ascontiguousarray(left, np.uint8), np.ascontiguousarray(right, np.uint8)
    if left.ndim != 2 or left.shape != right.shape:
        raise ValueError(f"left {left.shape} and right {right.shape} must be gray planes of one shape")
    cfg = (config or SGMConfig()).c_struct()
    out = np.zeros(left.shape, np.float32)
    bp = C.POINTER(C.c_ubyte)
    rc = call(left.shape[0], left.shape[1], left.ctypes.data_as(bp), right.ctypes.data_as(bp), C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, out


def stereo_disparity_host(left, right, config=None):
    """cvo_stereo_disparity_host: the left disparity of a rectified pair of 8-bit gray planes on one CPU thread, float32,
    invalid = -10.  The library's own matcher, not libelas."""
    rc, out = _stereo_disparity(_capi.lib().cvo_stereo_disparity_host, left, right, config)
    if rc != 0:
        _raise(rc, "cvo_stereo_disparity_host refused the planes or the configuration")
    return out


class DFilterConfig:
    """cvo_dfilter_config_t: the disparity post-filter's configuration (libelas's removeSmallSegments, gapInterpolation and
    adaptiveMean; tests/np_dfilter.py states them).  The defaults are libelas's ROBOTICS setting.  speckle_size <= 1,
    ipol_gap_width 0 and adaptive_mean 0 turn the three passes off."""

    def __init__(self, speckle_sim_threshold=1.0, speckle_size=200, ipol_gap_width=3, adaptive_mean=1):
        self.speckle_sim_threshold, self.speckle_size = float(speckle_sim_threshold), int(speckle_size)
        self.ipol_gap_width, self.adaptive_mean = int(ipol_gap_width), int(adaptive_mean)

    def c_struct(self):
        return _capi.cvo_dfilter_config_t(self.speckle_sim_threshold, self.speckle_size, self.ipol_gap_width, self.adaptive_mean)


def _disparity_filter(call, disparity, config, out=None):
    """Shared by CvoGPU.disparity_filter and disparity_filter_host -> (rc, filtered (rows, cols) float32).  out: the array to
    write, which may be `disparity` itself."""
    d = np.ascontiguousarray(disparity, np.float32)
    if d.ndim != 2:
        raise ValueError(f"disparity {d.shape} must be a (rows, cols) map")
    cfg = (config or DFilterConfig()).c_struct()
    if out is None:
        out = np.zeros(d.shape, np.float32)
    elif out.dtype != np.float32 or out.shape != d.shape or not out.flags.c_contiguous:
        raise ValueError("out must be a contiguous float32 array of the map's shape")
    fp = C.POINTER(C.c_float)
    rc = call(d.shape[0], d.shape[1], d.ctypes.data_as(fp), C.byref(cfg), out.ctypes.data_as(fp))
    return rc, out


def disparity_filter_host(disparity, config=None, out=None):
    """cvo_disparity_filter_host: libelas's three post-passes (speckle, gap, adaptive mean) on a float32 disparity map whose
    invalid pixels are negative, on one CPU thread; invalid pixels leave as -10."""
    rc, out = _disparity_filter(_capi.lib().cvo_disparity_filter_host, disparity, config, out)
    if rc != 0:
        _raise(rc, "cvo_disparity_filter_host refused the map or the configuration")
    return out


def _nlm_config(h, template_window, search_window):
    return _capi.cvo_nlm_config_t(float(h), int(template_window), int(search_window))


def nlm_weights(h=10, template_window=7, search_window=21, channels=1):
    """cvo_nlm_weights: the weight table of the non-local-means denoising, built where the twin and the device route take it
    -> dict(weight: all n_table entries, n_nonzero, mult, shift)."""
    cfg = _nlm_config(h, template_window, search_window)
    nt, nz, mult, shift = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    call = _capi.lib().cvo_nlm_weights
    rc = call(C.byref(cfg), int(channels), None, 0, C.byref(nt), C.byref(nz), C.byref(mult), C.byref(shift))
    if rc != 0:
        _raise(rc, "cvo_nlm_weights refused the configuration")
    weight = np.zeros(nt.value, np.int32)
    rc = call(C.byref(cfg), int(channels), weight.ctypes.data_as(C.POINTER(C.c_int)), nt.value, None, None, None, None)
    if rc != 0:
        _raise(rc, "cvo_nlm_weights refused the configuration")
    return dict(weight=weight, n_nonzero=nz.value, mult=mult.value, shift=shift.value)


def _nlm_image(image, channels=None):
    """An 8-bit image as (rows, cols, channels) contiguous bytes; (rows, cols) is one channel."""
    image = np.ascontiguousarray(image, np.uint8)
    if image.ndim == 2:
        image = image[:, :, None]
    if image.ndim != 3 or (channels is not None and image.shape[2] != channels):
        raise ValueError(f"an image of shape {image.shape} is not rows x cols x {channels or 'channels'}")
    return image


def _nlm_denoise(call, image, cfg, out, *extra):
    """Shared by the four denoising calls -> (rc, denoised image of the input's shape).  out: None, or the array written
    (the input itself for an in-place call)."""
    img = _nlm_image(image, 3 if extra else None)
    rows, cols, ch = img.shape
    dst = np.zeros_like(img) if out is None else out
    if dst.dtype != np.uint8 or not dst.flags.c_contiguous or dst.size != img.size:
        raise ValueError("out must be contiguous bytes of the image's size")
    bp = C.POINTER(C.c_ubyte)
    shape = () if extra else (ch,)
    rc = call(rows, cols, *shape, img.ctypes.data_as(bp), C.byref(cfg), *extra, dst.ctypes.data_as(bp))
    return rc, dst.reshape(np.shape(image)) if out is None else dst


def nlm_denoise_host(image, h=10, template_window=7, search_window=21, out=None):
    """cvo_nlm_denoise_host: cv::fastNlMeansDenoising of an 8-bit image of 1, 2 or 3 interleaved channels on one CPU thread
    (RawImage's call: 10, 7, 21).  out=image denoises in place."""
    rc, dst = _nlm_denoise(_capi.lib().cvo_nlm_denoise_host, image, _nlm_config(h, template_window, search_window), out)
    if rc != 0:
        _raise(rc, "cvo_nlm_denoise_host refused the image or the configuration")
    return dst


def nlm_denoise_lab_host(lab, h=10, h_color=10, template_window=7, search_window=21, out=None):
    """cvo_nlm_denoise_lab_host: the middle of cv::fastNlMeansDenoisingColored on a rows x cols x 3 Lab image - L with h, ab
    as one 2-channel image with h_color - on one CPU thread."""
    rc, dst = _nlm_denoise(_capi.lib().cvo_nlm_denoise_lab_host, lab, _nlm_config(h, template_window, search_window), out, float(h_color))
    if rc != 0:
        _raise(rc, "cvo_nlm_denoise_lab_host refused the image or the configuration")
    return dst


class LidarScan:
    """One raw LiDAR scan (cvo_lidar_scan_t): `xyzi` (n, 4) float32 - x, y, z, intensity in upstream's axes after
    KittiHandler::read_next_lidar (x = -raw.y, y = -raw.z, z = raw.x), in the order the sensor returned them - and optionally
    `semantic` (n,) int32 class ids, -1 = unlabelled, with `num_classes`."""

    def __init__(self, xyzi, semantic=None, num_classes=0):
        self.xyzi = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
        self.n = len(self.xyzi)
        self.semantic = None if semantic is None else np.ascontiguousarray(semantic, np.int32).reshape(self.n)
        self.num_classes = int(num_classes)

    def c_struct(self):
        """cvo_lidar_scan_t over this scan's arrays (which must outlive it)."""
        return _capi.cvo_lidar_scan_t(self.n, self.xyzi.ctypes.data, None if self.semantic is None else self.semantic.ctypes.data, self.num_classes)


class LidarConfig:
    """cvo_lidar_config_t: what upstream compiles into LeGoLoamPointSelection.hpp and the LiDAR constructors.  The HDL-64
    defaults (distance bound 40, `semantic`: 75); keyword arguments override fields, the derived constants follow."""

    def __init__(self, semantic=False, **fields):
        self.c = _capi.cvo_lidar_config_t()
        _capi.lib().cvo_lidar_config_default(C.byref(self.c), int(bool(semantic)))
        self.set(**fields)

    def set(self, **fields):
        for name, value in fields.items():
            if name not in dict(_capi.cvo_lidar_config_t._fields_):
                raise AttributeError(name)
            setattr(self.c, name, value)
        _capi.lib().cvo_lidar_config_derive(C.byref(self.c))
        return self

    def __getattr__(self, name):
        return getattr(self.__dict__["c"], name)


class LidarRand:
    """cvo_lidar_rand_t: the state of glibc's default rand(), which the thinning draws from; one state chained through the
    frames of a run reproduces a process that made no other draw.  Seed 1 is an unseeded process."""

    def __init__(self, seed=1):
        self.c = _capi.cvo_lidar_rand_t()
        self.seed(seed)

    def seed(self, seed):
        _capi.lib().cvo_lidar_rand_seed(C.byref(self.c), int(seed))

    def state(self):
        return list(self.c.r), self.c.front, self.c.rear

    def next(self):
        """cvo_lidar_rand_next: one draw, as rand() would return it, by the stepping function the library's calls use."""
        return int(_capi.lib().cvo_lidar_rand_next(C.byref(self.c)))


def debug_order_route_rule(n, finite=True, order=None, no_sort=False):
    """cvo_debug_order_route_rule: who orders a cloud of n points (0 host, 1 k_kd_order, 2 the multi-block ordering) under the
    text `order` of the ORDER switch (None: unset) - the function the upload paths call, no context needed."""
    return int(_capi.lib().cvo_debug_order_route_rule(int(n), int(bool(finite)), None if order is None else str(order).encode(), int(bool(no_sort))))


def debug_wide_plan(n):
    """cvo_debug_wide_plan -> (W, rows): the leaf capacity of a default context and the (level, lo, hi, left) of every cut of
    a segment of more than W points in the host's plan of the multi-block ordering of n points."""
    W, k = C.c_int(), C.c_int()
    ipp = C.POINTER(C.c_int)
    rc = _capi.lib().cvo_debug_wide_plan(int(n), C.byref(W), None, 0, C.byref(k))
    rows = np.zeros((max(k.value, 1), 4), np.int32)
    if rc == 0:
        rc = _capi.lib().cvo_debug_wide_plan(int(n), C.byref(W), rows.ctypes.data_as(ipp), k.value, C.byref(k))
    if rc != 0:
        _raise(rc, "cvo_debug_wide_plan refused its arguments")
    return W.value, rows[:k.value]


def debug_wide_plan_at(n, leaf):
    """cvo_debug_wide_plan_at -> rows: debug_wide_plan's rows with leaves of at most `leaf` points (1024 .. 16384), the plan of a
    context with WIDE_LEAF=leaf."""
    k = C.c_int()
    ipp = C.POINTER(C.c_int)
    rc = _capi.lib().cvo_debug_wide_plan_at(int(n), int(leaf), None, 0, C.byref(k))
    rows = np.zeros((max(k.value, 1), 4), np.int32)
    if rc == 0:
        rc = _capi.lib().cvo_debug_wide_plan_at(int(n), int(leaf), rows.ctypes.data_as(ipp), k.value, C.byref(k))
    if rc != 0:
        _raise(rc, "cvo_debug_wide_plan_at refused its arguments")
    return rows[:k.value]


def debug_lidar_atan2(y, x):
    """cvo_debug_lidar_atan2: the library's own atan2 in degrees (cvo_lidar_math.h, what the twin and the kernels compile),
    evaluated on the host for arrays y, x of doubles."""
    y, x = np.ascontiguousarray(np.broadcast_arrays(y, x)[0], np.float64), np.ascontiguousarray(np.broadcast_arrays(y, x)[1], np.float64)
    out = np.zeros(y.shape, np.float64)
    dp = C.POINTER(C.c_double)
    rc = _capi.lib().cvo_debug_lidar_atan2(int(y.size), y.ctypes.data_as(dp), x.ctypes.data_as(dp), out.ctypes.data_as(dp))
    if rc != 0:
        _raise(rc, "cvo_debug_lidar_atan2 refused its arguments")
    return out


def _lidar_select(call, scan, config, rand):
    """Shared by CvoGPU.lidar_select and lidar_select_host -> (rc, indices, is_edge)."""
    cap = max(2 * scan.n, 1)
    index, is_edge = np.zeros(cap, np.int32), np.zeros(cap, np.uint8)
    n, s = C.c_int(), scan.c_struct()
    rc = call(C.byref(s), C.byref(config.c), C.byref(rand.c), index.ctypes.data_as(C.POINTER(C.c_int)), is_edge.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(n))
    return rc, index[:n.value].copy(), is_edge[:n.value].astype(bool)


def lidar_select_host(scan, config, rand):
    """cvo_lidar_select_host: the CPU twin of CvoGPU.lidar_select, no context -> (indices, is_edge)."""
    rc, index, is_edge = _lidar_select(_capi.lib().cvo_lidar_select_host, scan, config, rand)
    if rc != 0:
        _raise(rc, "cvo_lidar_select_host refused the scan or the config")
    return index, is_edge


class DeviceCloud:
    """A cloud resident in HBM (cvo_cloud*)."""

    def __init__(self, gpu, pc):
        self.gpu = gpu
        self.n = pc.num_points()
        xyz, feat, label, geo = pc.device_arrays()
        self._keep = (xyz, feat, label, geo)
        h = C.c_void_p()
        rc = gpu.L.cvo_cloud_upload(gpu.ctx, self.n, _fptr(xyz), _fptr(feat), _fptr(label), _fptr(geo), C.byref(h))
        gpu._check(rc)
        self.handle = h

    def free(self):
        if self.handle:
            self.gpu.L.cvo_cloud_free(self.handle)
            self.handle = None

    def debug_order(self):
        """The cloud's spatial (k-d) ordering: original index of the point at every sorted position."""
        out = np.zeros(max(self.n, 1), np.int32)
        self.gpu._check(self.gpu.L.cvo_debug_cloud_order(self.handle, out.ctypes.data_as(C.POINTER(C.c_int))))
        return out[:self.n]

    def debug_order_route(self):
        """cvo_debug_cloud_order_route: what ordered this cloud - 0 the host, 1 k_kd_order, 2 the multi-block ordering of
        ORDER=wide."""
        return int(self.gpu.L.cvo_debug_cloud_order_route(self.handle))

    def debug_wide_pivots(self):
        """cvo_debug_cloud_wide_pivots -> (pivot, rem), uint32 each: the select's result for every cut of the cloud's plan, in
        plan order, as the device computed it.  Needs a context with WIDE_RECORD=1 and a cloud ordered by the multi-block
        ordering; raises otherwise."""
        n = C.c_int()
        up = C.POINTER(C.c_uint)
        self.gpu._check(self.gpu.L.cvo_debug_cloud_wide_pivots(self.handle, 0, None, None, C.byref(n)))
        pivot, rem = np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.uint32)
        self.gpu._check(self.gpu.L.cvo_debug_cloud_wide_pivots(self.handle, n.value, pivot.ctypes.data_as(up), rem.ctypes.data_as(up), C.byref(n)))
        return pivot[:n.value], rem[:n.value]

    def debug_tiles(self):
        """cvo_debug_cloud_tiles: the records k_overlap culls by, float32[ceil(n / 64), 8] - centre x, y, z, radius, box half
        extents x, y, z, 0 of every 64 consecutive sorted positions (debug_order() says which points those are)."""
        out = np.zeros(((self.n + 63) // 64 or 1, 8), np.float32)
        nt = C.c_int()
        self.gpu._check(self.gpu.L.cvo_debug_cloud_tiles(self.gpu.ctx, self.handle, _fptr(out), C.byref(nt)))
        return out[:nt.value]

    def download(self):
        """cvo_cloud_download: the cloud's rows in ORIGINAL order as a CvoPointCloud, bit for bit what was uploaded.  An
        attribute the cloud does not hold is left out (features / labels: no columns; geometric types: zeros); `.present`
        of the result holds the CVO_CLOUD_HAS_* bits (1 features, 2 labels, 4 geometric types)."""
        n = self.n
        xyz, feat, label = np.zeros((n, 3), np.float32), np.zeros((n, FEATURE_DIMENSIONS), np.float32), np.zeros((n, NUM_CLASSES), np.float32)
        geo = np.zeros((n, 2), np.float32)
        present = C.c_int()
        self.gpu._check(self.gpu.L.cvo_cloud_download(self.gpu.ctx, self.handle, _fptr(xyz), _fptr(feat), _fptr(label), _fptr(geo),
                                                      C.byref(present)))
        has = present.value
        pc = CvoPointCloud.from_arrays(xyz, feat if has & 1 else None, label if has & 2 else None, geo)
        pc.present = has
        return pc

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceCloudAoS(DeviceCloud):
    """A cloud uploaded from the reference's 192-byte AoS records (pcl::PointCloud<CvoPoint>::points, the wire format
    of pcl_PointCloud_to_gpu, CvoGPU_impl.cu:287-362) through cvo_cloud_upload_aos192."""

    def __init__(self, gpu, records):
        rec = np.ascontiguousarray(records)
        assert rec.dtype.itemsize == 192, "CvoPoint is 192 bytes (PointSegmentedDistribution.hpp:17-99)"
        self.gpu = gpu
        self.n = int(rec.shape[0])
        self._keep = rec
        h = C.c_void_p()
        gpu._check(gpu.L.cvo_cloud_upload_aos192(gpu.ctx, self.n, rec.ctypes.data_as(C.c_void_p), C.byref(h)))
        self.handle = h


# what SemanticMap.query / raycast / render return: one numpy array per output of the C call
MapQuery = collections.namedtuple("MapQuery", "found state semantics probs vars feat centre")
MapRays = collections.namedtuple("MapRays", "status key centre t steps state semantics")
MapView = collections.namedtuple("MapView", "depth semantics feat label")


class MapConfig:
    """cvo_map_config_t: the semantic voxel map's configuration; the defaults are those of upstream's driver
    main_local_mapping.cpp.  sf2 and ell are the sparse kernel's (SemanticMap.set_kernel); the counting kernel ignores them, and
    var_thresh and ds_resolution are accepted and change nothing, as upstream."""

    FIELDS = ("resolution", "block_depth", "num_classes", "sf2", "ell", "prior", "var_thresh", "free_thresh", "occupied_thresh",
              "ds_resolution", "free_resolution", "max_range")

    def __init__(self, resolution=0.05, block_depth=1, num_classes=0, sf2=1.0, ell=1.0, prior=0.0, var_thresh=1.0, free_thresh=0.65,
                 occupied_thresh=0.9, ds_resolution=-1.0, free_resolution=1.0, max_range=-1.0):
        self.resolution, self.block_depth, self.num_classes = float(resolution), int(block_depth), int(num_classes)
        self.sf2, self.ell, self.prior, self.var_thresh = float(sf2), float(ell), float(prior), float(var_thresh)
        self.free_thresh, self.occupied_thresh = float(free_thresh), float(occupied_thresh)
        self.ds_resolution, self.free_resolution, self.max_range = float(ds_resolution), float(free_resolution), float(max_range)

    def c_struct(self):
        return _capi.cvo_map_config_t(*[getattr(self, f) for f in self.FIELDS])


def _map_rows(pc_or_rows, num_classes):
    """(xyz, feat or None, label or None) float32 rows of a CvoPointCloud or of a tuple (xyz[, feat[, label]])."""
    if isinstance(pc_or_rows, CvoPointCloud):
        pc = pc_or_rows
        rows = (pc.positions_, pc.features_ if pc.feature_dimensions_ == 5 else None, pc.labels_ if pc.num_classes_ else None)
    else:
        rows = tuple(pc_or_rows) if isinstance(pc_or_rows, (tuple, list)) else (pc_or_rows,)
        rows = rows + (None,) * (3 - len(rows))
    xyz = np.ascontiguousarray(rows[0], np.float32).reshape(-1, 3)
    feat = None if rows[1] is None else np.ascontiguousarray(rows[1], np.float32).reshape(-1, 5)
    label = None if rows[2] is None or num_classes == 0 else np.ascontiguousarray(rows[2], np.float32).reshape(xyz.shape[0], -1)
    if feat is not None and feat.shape[0] != xyz.shape[0]:
        raise ValueError("feature rows and points differ in number")
    if label is not None and label.shape[1] != num_classes:
        raise ValueError(f"label rows have {label.shape[1]} classes, the map {num_classes}")
    return xyz, feat, label


class SemanticMap:
    """cvo_map: a semantic voxel map (upstream's SemanticBKIOctoMap, block_depth 1, under its counting sensor model -
    tests/np_bki.py states it - or, after set_kernel("sparse"), its sparse kernel - tests/np_bki_sparse.py).
    CvoGPU.map_open makes one on a context; SemanticMap(None, config) is the CPU twin's."""

    def __init__(self, gpu, config=None, initial_voxels=0):
        self.gpu, self.config = gpu, config or MapConfig()
        self.L = gpu.L if gpu is not None else _capi.lib()
        cfg, h = self.config.c_struct(), C.c_void_p()
        if gpu is not None:
            gpu._check(self.L.cvo_map_open(gpu.ctx, C.byref(cfg), int(initial_voxels), C.byref(h)))
            gpu._maps.append(weakref.ref(self))
        else:
            rc = self.L.cvo_map_open_host(C.byref(cfg), C.byref(h))
            if rc != 0:
                _raise(rc, "cvo_map_open_host refused the configuration")
        self.handle = h

    def _check(self, rc, text):
        if self.gpu is not None:
            return self.gpu._check(rc)
        if rc != 0:
            _raise(rc, text)
        return rc

    def insert(self, pc_or_rows, origin=None, pose=None):
        """cvo_map_insert(_host): the hits, already in the map frame, seen from `origin`; or cvo_map_insert_posed: the rows
        moved by `pose` (3x4 or 4x4), its translation the origin."""
        xyz, feat, label = _map_rows(pc_or_rows, self.config.num_classes)
        if (origin is None) == (pose is None):
            raise ValueError("give the origin or the pose")
        if pose is not None:
            if self.gpu is None:
                raise ValueError("a host map takes rows in the map frame")
            T = np.ascontiguousarray(np.asarray(pose, np.float32)[:3, :4])
            return self._check(self.L.cvo_map_insert_posed(self.handle, xyz.shape[0], _fptr(xyz), _fptr(feat), _fptr(label), _fptr(T)), "")
        o = np.ascontiguousarray(origin, np.float32).reshape(3)
        call = self.L.cvo_map_insert if self.gpu is not None else self.L.cvo_map_insert_host
        return self._check(call(self.handle, xyz.shape[0], _fptr(xyz), _fptr(feat), _fptr(label), _fptr(o)), "cvo_map_insert_host refused the hits")

    KERNELS = {"csm": 0, "sparse": 1}  # CVO_MAP_KERNEL_*

    def set_kernel(self, kernel):
        """cvo_map_set_kernel: "csm", the counting sensor model (the default), or "sparse", covSparse over a block and its
        face neighbours (tests/np_bki_sparse.py states it); applies to every insert that follows."""
        code = self.KERNELS.get(kernel, kernel)
        if not isinstance(code, int):
            raise ValueError(f"the kernel is 'csm' or 'sparse', got {kernel!r}")
        return self._check(self.L.cvo_map_set_kernel(self.handle, code), "cvo_map_set_kernel refused the kernel")

    def insert_cloud(self, cloud, pose=None, origin=None):
        """cvo_map_insert_cloud: the rows of a resident cloud (DeviceCloud), in original order, as the hits of one insert,
        without a host copy - moved by `pose` (3x4 or 4x4, cast to float32 as insert casts; None: the stored rows), seen
        from `origin` (None: the pose's translation).  The map insert(cloud.download() rows, pose= / origin=) leaves."""
        if pose is None and origin is None:
            raise ValueError("give the origin or the pose")
        if self.gpu is None:
            raise ValueError("a host map takes rows, not a resident cloud")
        T = o = None
        if pose is not None:
            P = np.asarray(pose, np.float32)
            if P.shape not in ((3, 4), (4, 4)):
                raise ValueError(f"the pose is 3x4 or 4x4, got {P.shape}")
            T = np.ascontiguousarray(P[:3, :4])
        if origin is not None:
            o = np.ascontiguousarray(origin, np.float32).reshape(3)
        return self._check(self.L.cvo_map_insert_cloud(self.handle, cloud.handle, _fptr(T), _fptr(o)), "")

    def resident_cloud(self):
        """cvo_map_cloud_resident: the OCCUPIED voxels in ascending key order as a DeviceCloud, built on the device from the
        rows where the read-out kernel leaves them; interchangeable with cloud(resident=True)[3]."""
        if self.gpu is None:
            raise ValueError("a host map has no resident cloud")
        h, n = C.c_void_p(), C.c_longlong()
        self._check(self.L.cvo_map_cloud_resident(self.handle, C.byref(h), C.byref(n)), "")
        return self.gpu._adopt(h, n.value)

    STOP_BITS = {"free": 1, "occupied": 2, "unknown": 4, "absent": 8}  # CVO_MAP_STOP_*

    @classmethod
    def stop_mask(cls, stop):
        """The stop mask of raycast / render: an int 0 .. 15, or names out of "free", "occupied", "unknown", "absent"."""
        if isinstance(stop, (int, np.integer)) and not isinstance(stop, bool):
            mask = int(stop)
        else:
            names = (stop,) if isinstance(stop, str) else tuple(stop)
            unknown = [s for s in names if s not in cls.STOP_BITS]
            if unknown:
                raise ValueError(f"a stop is one of {sorted(cls.STOP_BITS)}, got {unknown[0]!r}")
            mask = 0
            for s in names:
                mask |= cls.STOP_BITS[s]
        if not 0 <= mask <= 15:
            raise ValueError(f"the stop mask lies in 0 .. 15, got {mask}")
        return mask

    def _classes(self):
        return max(self.config.num_classes, 1) + 1

    def query(self, points_or_cloud, pose=None):
        """cvo_map_query(_host) / cvo_map_query_cloud: what is at these points - upstream's search(x, y, z) with the node's
        getters, batched.  points (n, 3) in the map frame, or a resident cloud (DeviceCloud) whose rows, in original order, are
        moved by `pose` (3x4 or 4x4; None: as stored) on the device.  -> MapQuery(found, state, semantics, probs, vars, feat,
        centre); found: 0 no stored voxel (the default node answers), 1 stored, 2 outside the map's key range or not finite."""
        is_cloud = isinstance(points_or_cloud, DeviceCloud)
        T = None
        if pose is not None:
            if not is_cloud:
                raise ValueError("a pose moves a resident cloud; points are given in the map frame")
            P = np.asarray(pose, np.float32)
            if P.shape not in ((3, 4), (4, 4)):
                raise ValueError(f"the pose is 3x4 or 4x4, got {P.shape}")
            T = np.ascontiguousarray(P[:3, :4])
        if is_cloud:
            if self.gpu is None:
                raise ValueError("a host map takes points, not a resident cloud")
            n, xyz = int(points_or_cloud.n), None
        else:
            xyz = np.asarray(points_or_cloud, np.float32)
            if xyz.ndim != 2 or xyz.shape[1] != 3:
                raise ValueError(f"the points are (n, 3), got {xyz.shape}")
            xyz = np.ascontiguousarray(xyz)
            n = xyz.shape[0]
        nc = self._classes()
        r = MapQuery(np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros((n, nc), np.float32),
                     np.zeros((n, nc), np.float32), np.zeros((n, 5), np.float32), np.zeros((n, 3), np.float32))
        out = _capi.cvo_map_query_out_t(*[a.ctypes.data for a in r])
        if is_cloud:
            self._check(self.L.cvo_map_query_cloud(self.handle, points_or_cloud.handle, _fptr(T), C.byref(out)), "")
        else:
            call = self.L.cvo_map_query if self.gpu is not None else self.L.cvo_map_query_host
            self._check(call(self.handle, n, _fptr(xyz), C.byref(out)), "cvo_map_query_host refused the points")
        return r

    def raycast(self, origin, end, stop=("occupied",), max_steps=1 << 20):
        """cvo_map_raycast(_host): the library's own walk (not upstream's RayCaster) over the voxels each segment
        origin[i] -> end[i] passes through, face by face, to the first voxel whose state is in `stop` (names or a mask; 0 walks
        to the end).  origin may be one point for all rays.  -> MapRays(status, key, centre, t, steps, state, semantics);
        status: 0 reached the end, 1 stopped, 2 more than max_steps voxels, 3 an endpoint outside the map."""
        mask = self.stop_mask(stop)
        e = np.asarray(end, np.float32)
        if e.ndim != 2 or e.shape[1] != 3:
            raise ValueError(f"the ends are (n, 3), got {e.shape}")
        o = np.asarray(origin, np.float32)
        if o.shape == (3,):
            o = np.broadcast_to(o, e.shape)
        if o.shape != e.shape:
            raise ValueError(f"origins {o.shape} and ends {e.shape} differ in shape")
        if not 1 <= int(max_steps) <= 1 << 20:
            raise ValueError(f"max_steps lies in 1 .. 2^20, got {max_steps}")
        o, e, n = np.ascontiguousarray(o), np.ascontiguousarray(e), e.shape[0]
        r = MapRays(np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32),
                    np.zeros(n, np.uint8), np.zeros(n, np.int32))
        out = _capi.cvo_map_ray_out_t(*[a.ctypes.data for a in r])
        call = self.L.cvo_map_raycast if self.gpu is not None else self.L.cvo_map_raycast_host
        self._check(call(self.handle, n, _fptr(o), _fptr(e), mask, int(max_steps), C.byref(out)), "cvo_map_raycast_host refused the rays")
        return r

    def render(self, pose, fx, fy, cx, cy, rows, cols, z_far, stop=("occupied",), planes=("depth", "semantics", "feat", "label")):
        """cvo_map_render(_host): the map seen by a pinhole camera at `pose` (3x4 or 4x4, camera to map), one ray of raycast
        per pixel out to camera z = z_far, made on the device.  -> MapView(depth, semantics, feat, label): rows x cols z-depth (0:
        no stop), class (-1: no stop), x 5 features, x num_classes class distribution (cvo_rgbd_frame_t::semantic's layout);
        a plane not named in `planes` is None and is not computed."""
        mask = self.stop_mask(stop)
        P = np.asarray(pose, np.float32)
        if P.shape not in ((3, 4), (4, 4)):
            raise ValueError(f"the pose is 3x4 or 4x4, got {P.shape}")
        rows, cols = int(rows), int(cols)
        if rows < 1 or cols < 1:
            raise ValueError("rows and cols are at least 1")
        if rows * cols > 1 << 24:
            raise ValueError("more than 2^24 pixels")
        bad = [p for p in planes if p not in MapView._fields]
        if bad:
            raise ValueError(f"a plane is one of {MapView._fields}, got {bad[0]!r}")
        T = np.ascontiguousarray(P[:3, :4])
        shapes = dict(depth=((rows, cols), np.float32), semantics=((rows, cols), np.int32), feat=((rows, cols, 5), np.float32),
                      label=((rows, cols, self.config.num_classes), np.float32))
        r = MapView(*[np.zeros(*shapes[p]) if p in planes else None for p in MapView._fields])
        out = _capi.cvo_map_render_out_t(*[None if a is None or a.size == 0 else a.ctypes.data for a in r])
        call = self.L.cvo_map_render if self.gpu is not None else self.L.cvo_map_render_host
        self._check(call(self.handle, _fptr(T), float(fx), float(fy), float(cx), float(cy), rows, cols, float(z_far), mask, C.byref(out)),
                    "cvo_map_render_host refused the view")
        return r

    def size(self):
        """cvo_map_size -> (voxels stored, of them OCCUPIED)."""
        v, o = C.c_longlong(), C.c_longlong()
        self._check(self.L.cvo_map_size(self.handle, C.byref(v), C.byref(o)), "cvo_map_size failed")
        return v.value, o.value

    def cloud(self, resident=False):
        """cvo_map_cloud(_host): the OCCUPIED voxels in ascending key order -> (xyz (n, 3), feat (n, 5), label (n, C)); with
        resident=True also the DeviceCloud cvo_cloud_upload makes of those rows, as a fourth element."""
        cap, C_ = self.size()[1], self.config.num_classes  # (one counting pass; the voxels are collected and sorted once, below)
        xyz, feat, label = np.zeros((cap, 3), np.float32), np.zeros((cap, 5), np.float32), np.zeros((cap, C_), np.float32)
        n = C.c_longlong()
        lab = _fptr(label) if C_ else None
        if self.gpu is None:
            if resident:
                raise ValueError("a host map has no resident cloud")
            self._check(self.L.cvo_map_cloud_host(self.handle, cap, _fptr(xyz), _fptr(feat), lab, C.byref(n)), "cvo_map_cloud_host failed")
            return xyz[:n.value], feat[:n.value], label[:n.value]
        h = C.c_void_p()
        self._check(self.L.cvo_map_cloud(self.handle, cap, _fptr(xyz), _fptr(feat), lab, C.byref(n), C.byref(h) if resident else None), "")
        out = (xyz[:n.value], feat[:n.value], label[:n.value])
        if not resident:
            return out
        dc = DeviceCloud.__new__(DeviceCloud)
        dc.gpu, dc.n, dc._keep, dc.handle = self.gpu, int(n.value), None, h
        return out + (dc,)

    def debug_stats(self, readback=False):
        """cvo_debug_map_stats of the last insert -> dict(on_device, training, members, longest_run, capacity, growths,
        longest_probe, voxels, classes); readback=True adds the stored voxels sorted by key: keys (v,), ms (v, classes), fs (v, 5)."""
        on, counts = C.c_int(), (C.c_ulonglong * 8)()
        self._check(self.L.cvo_debug_map_stats(self.handle, C.byref(on), counts, None, None, None), "cvo_debug_map_stats failed")
        names = ("training", "members", "longest_run", "capacity", "growths", "longest_probe", "voxels", "classes")
        out = dict(on_device=on.value, **{k: int(v) for k, v in zip(names, counts)})
        if readback:
            cap, nc = max(out["capacity"], 1), out["classes"]
            keys, ms, fs = np.full(cap, np.uint64(2**64 - 1), np.uint64), np.zeros((cap, nc), np.float32), np.zeros((cap, 5), np.float32)
            self._check(self.L.cvo_debug_map_stats(self.handle, None, None, keys.ctypes.data_as(C.POINTER(C.c_ulonglong)), _fptr(ms), _fptr(fs)),
                        "cvo_debug_map_stats failed")
            live = np.flatnonzero(keys != np.uint64(2**64 - 1))
            live = live[np.argsort(keys[live], kind="stable")]
            out.update(keys=keys[live], ms=ms[live], fs=fs[live])
        return out

    def close(self):
        if getattr(self, "handle", None):
            if self.gpu is None:
                self.L.cvo_map_close_host(self.handle)
            elif self.gpu.ctx:
                self.L.cvo_map_close(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def map_open_host(config=None):
    """cvo_map_open_host: a semantic voxel map of the CPU twin (one thread, no context)."""
    return SemanticMap(None, config)


def map_insert_host(smap, pc_or_rows, origin):
    """cvo_map_insert_host on a map of map_open_host."""
    return smap.insert(pc_or_rows, origin=origin)


def map_cloud_host(smap):
    """cvo_map_cloud_host on a map of map_open_host."""
    return smap.cloud()


def map_close_host(smap):
    smap.close()


# numpy view of pcl::PointSegmentedDistribution<5, 19> (PointSegmentedDistribution.hpp:17-99): byte offsets as laid out
# by PCL_ADD_POINT4D / PCL_ADD_RGB and the member order, verified with a layout-identical struct
CVO_POINT_DTYPE = np.dtype({
    "names": ["xyz", "pad_w", "rgba", "features", "label", "label_distribution", "geometric_type", "normal", "covariance",
              "cov_eigenvalues"],
    "formats": [(np.float32, 3), np.float32, np.uint32, (np.float32, 5), np.int32, (np.float32, 19), (np.float32, 2),
                (np.float32, 3), (np.float32, 9), (np.float32, 3)],
    "offsets": [0, 12, 16, 20, 40, 44, 120, 128, 140, 176],
    "itemsize": 192,
})


def cvo_points_from_pointcloud(pc):
    """What CvoPointCloud_to_gpu builds per point (CvoGPU_impl.cu:206-263) as an array of CvoPoint records: xyz,
    features (+ r, g, b bytes = min(255, f * 255)), label_distribution (+ label = argmax), geometric_type."""
    xyz, feat, label, geo = pc.device_arrays()
    n = xyz.shape[0]
    rec = np.zeros(n, CVO_POINT_DTYPE)
    rec["xyz"] = xyz
    rec["pad_w"] = 1.0
    if feat is not None:
        rec["features"] = feat
        rgb = np.minimum(255.0, feat[:, :3] * 255.0).astype(np.uint32)
        rec["rgba"] = (rgb[:, 0] << 16) | (rgb[:, 1] << 8) | rgb[:, 2]
    if label is not None:
        rec["label_distribution"] = label
        rec["label"] = np.argmax(label, axis=1)
    if geo is not None:
        rec["geometric_type"] = geo
    return rec


def _device_array(name, a, width, dtype, device):
    """(address or None, records or None, row stride in bytes) of one argument of CvoGPU.upload_device; width None: the 1-D
    index array `rows` (then: address, n, 4)."""
    if a is None:
        return None, None, 0
    if not hasattr(a, "data_ptr"):  # (address, records, stride in bytes) / (address, n)
        t = tuple(a)
        if len(t) != (2 if width is None else 3):
            raise ValueError(f"{name}: give a tensor or (address, {'n' if width is None else 'records, stride in bytes'})")
        return int(t[0]) or None, int(t[1]), (4 if width is None else int(t[2]))
    if not str(a.dtype).endswith(dtype):
        raise TypeError(f"{name}: dtype {a.dtype}, {dtype} is required")
    dev = a.device
    if getattr(dev, "type", "cuda") == "cpu":
        raise ValueError(f"{name} is a host tensor")
    if getattr(dev, "index", None) not in (None, device):
        raise ValueError(f"{name} is on device {dev.index}, the context on {device}")
    shape, stride = tuple(a.shape), tuple(a.stride())
    if width is None:
        if len(shape) != 1 or (shape[0] > 1 and stride[0] != 1):
            raise ValueError(f"{name} must be a contiguous 1-D tensor")
        return int(a.data_ptr()) or None, int(shape[0]), 4
    if len(shape) != 2 or shape[1] != width:
        raise ValueError(f"{name} is {shape}, (records, {width}) is required")
    if stride[1] != 1:
        raise ValueError(f"{name}: rows must be contiguous (inner stride {stride[1]})")
    return int(a.data_ptr()) or None, int(shape[0]), (4 * int(stride[0]) if shape[0] > 1 else 4 * width)


def _sync_producers(objs):
    """Waits for the current stream of every tensor's device, where the tensor's module offers <module>.cuda.current_stream
    (torch does): the library reads the arrays on its own stream."""
    import sys
    seen = set()
    for o in objs:
        mod = sys.modules.get(type(o).__module__.split(".")[0])
        cur = getattr(getattr(mod, "cuda", None), "current_stream", None)
        key = (id(mod), str(o.device))
        if cur is not None and key not in seen:
            seen.add(key)
            cur(o.device).synchronize()


def _is_tensor(a):
    return hasattr(a, "data_ptr")


def _plane_checks(name, a, dtypes, device):
    """dtype, device and density of a tensor handed over as a dense plane -> its dtype's name."""
    kind = [d for d in dtypes if str(a.dtype).endswith(d)]
    if not kind:
        raise TypeError(f"{name}: dtype {a.dtype}, {' or '.join(dtypes)} is required")
    dev = a.device
    if getattr(dev, "type", "cuda") == "cpu":
        raise ValueError(f"{name} is a host tensor")
    if getattr(dev, "index", None) not in (None, device):
        raise ValueError(f"{name} is on device {dev.index}, the context on {device}")
    shape, stride, want = tuple(a.shape), tuple(a.stride()), 1
    for k in range(len(shape) - 1, -1, -1):
        if shape[k] > 1 and stride[k] != want:
            raise ValueError(f"{name} must be dense: strides {stride} for shape {shape}; pass {name}.contiguous()")
        want *= shape[k]
    return kind[0]


class DeviceRGBDFrame:
    """One RGB-D frame whose planes are ALREADY in device memory (cvo_rgbd_device_frame_t): what RGBDFrame holds, never copied.
    Every plane is either a torch-like object (data_ptr(), stride(), shape, dtype, device) or a tuple of a device address and
    what a tensor would have said:

        image     (rows, cols) or (rows, cols, 3) uint8, BGR, dense            | (address, rows, cols, channels)
        depth     (rows, cols) uint16 (or int16 holding those bits) / float32  | (address, "u16" or "f32")
        gray      None or (rows, cols) uint8, dense                            | (address,)
        semantic  None or float32 scores, layout "hwc" (rows, cols, classes) or "chw" (classes, rows, cols), ANY strides that
                  are multiples of 4 bytes - a permuted view, a column slice of a wider tensor -
                                                                             | (address, classes, row, pixel, class stride in bytes)

    image / gray / depth must be contiguous (`.contiguous()`); the semantic strides are taken from the tensor.  device: the
    context's device index, checked against every tensor."""

    def __init__(self, image, depth, fx, fy, cx, cy, scaling_factor, gray=None, semantic=None, layout="hwc", device=0):
        if layout not in ("hwc", "chw"):
            raise ValueError(f"layout {layout!r}: 'hwc' (rows, cols, classes) or 'chw' (classes, rows, cols)")
        self.device = int(device)
        self.tensors = [a for a in (image, depth, gray, semantic) if _is_tensor(a)]
        if _is_tensor(image):
            _plane_checks("image", image, ("uint8",), device)
            shape = tuple(image.shape)
            if len(shape) == 3 and shape[2] == 1:
                shape = shape[:2]
            if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3):
                raise ValueError(f"image is {tuple(image.shape)}, (rows, cols) or (rows, cols, 3) is required")
            self.rows, self.cols, self.channels = int(shape[0]), int(shape[1]), (1 if len(shape) == 2 else 3)
            self.image = int(image.data_ptr())
        else:
            t = tuple(image)
            if len(t) != 4:
                raise ValueError("image: give a tensor or (address, rows, cols, channels)")
            self.image, self.rows, self.cols, self.channels = (int(v) for v in t)
        if _is_tensor(depth):
            kind = _plane_checks("depth", depth, ("uint16", "int16", "float32"), device)
            if tuple(depth.shape) != (self.rows, self.cols):
                raise ValueError(f"depth is {tuple(depth.shape)}, the image {self.rows} x {self.cols}")
            self.depth, self.depth_type = int(depth.data_ptr()), (_capi.CVO_DEPTH_F32 if kind == "float32" else _capi.CVO_DEPTH_U16)
        else:
            t = tuple(depth)
            if len(t) != 2 or t[1] not in ("u16", "f32"):
                raise ValueError('depth: give a tensor or (address, "u16" | "f32")')
            self.depth, self.depth_type = int(t[0]), (_capi.CVO_DEPTH_F32 if t[1] == "f32" else _capi.CVO_DEPTH_U16)
        self.gray = None
        if gray is not None:
            if _is_tensor(gray):
                _plane_checks("gray", gray, ("uint8",), device)
                if tuple(gray.shape) != (self.rows, self.cols):
                    raise ValueError(f"gray is {tuple(gray.shape)}, the image {self.rows} x {self.cols}")
                self.gray = int(gray.data_ptr())
            else:
                self.gray = int(gray[0] if isinstance(gray, (tuple, list)) else gray)
        self.num_classes, self.semantic, self.semantic_strides = 0, None, (0, 0, 0)
        if semantic is not None:
            if _is_tensor(semantic):
                if not str(semantic.dtype).endswith("float32"):
                    raise TypeError(f"semantic: dtype {semantic.dtype}, float32 is required")
                dev = semantic.device
                if getattr(dev, "type", "cuda") == "cpu":
                    raise ValueError("semantic is a host tensor")
                if getattr(dev, "index", None) not in (None, device):
                    raise ValueError(f"semantic is on device {dev.index}, the context on {device}")
                shape, stride = tuple(semantic.shape), tuple(4 * int(s) for s in semantic.stride())
                if len(shape) != 3 or (shape[:2] if layout == "hwc" else shape[1:]) != (self.rows, self.cols):
                    raise ValueError(f"semantic is {shape} with layout {layout!r}, the image {self.rows} x {self.cols}")
                r, p, c = (0, 1, 2) if layout == "hwc" else (1, 2, 0)
                self.num_classes, self.semantic = int(shape[c]), int(semantic.data_ptr())
                self.semantic_strides = (stride[r], stride[p], stride[c])
            else:
                t = tuple(semantic)
                if len(t) != 5:
                    raise ValueError("semantic: give a tensor or (address, classes, row stride, pixel stride, class stride) in bytes")
                self.semantic, self.num_classes = int(t[0]), int(t[1])
                self.semantic_strides = tuple(int(v) for v in t[2:])
        self.fx, self.fy, self.cx, self.cy, self.scaling_factor = (float(v) for v in (fx, fy, cx, cy, scaling_factor))

    def c_struct(self):
        """cvo_rgbd_device_frame_t over this frame's planes (which must stay allocated until the call returns)."""
        return _capi.cvo_rgbd_device_frame_t(self.rows, self.cols, self.channels, self.image or None, self.gray, self.depth or None, self.depth_type,
                                             self.fx, self.fy, self.cx, self.cy, self.scaling_factor, self.num_classes, self.semantic,
                                             *self.semantic_strides)


def rgbd_frame_rows_host(frame, pixel, method=None, recipe=False, is_edge=None, semantic=None, layout="hwc"):
    """cvo_rgbd_frame_rows_host: the CPU twin of the rows CvoGPU.upload_rgbd_points_device / upload_rgbd_device build, no
    context.  frame: an RGBDFrame (host arrays); semantic (optional, replaces frame.semantic): a float32 numpy array or view
    with ANY strides, layout "hwc" or "chw".  pixel: indices v * cols + u.  recipe False: the constructor's rows of `method`
    (DSO_EDGES / FULL); True: the recipe's rows, is_edge per pixel.  -> dict(xyz (n, 3), feat (n, 5), label (n, 19) or None
    without classes, geotype (n, 2), excluded (n,) bool)."""
    L = _capi.lib()
    if layout not in ("hwc", "chw"):
        raise ValueError(f"layout {layout!r}: 'hwc' or 'chw'")
    sem = frame.semantic if semantic is None else semantic
    nc, sem_ptr, strides = 0, None, (0, 0, 0)
    if sem is not None:
        if sem.dtype != np.float32 or sem.ndim != 3:
            raise ValueError("semantic: a 3-D float32 array is required")
        r, p, c = (0, 1, 2) if layout == "hwc" else (1, 2, 0)
        if (sem.shape[r], sem.shape[p]) != (frame.rows, frame.cols):
            raise ValueError(f"semantic is {sem.shape} with layout {layout!r}, the image {frame.rows} x {frame.cols}")
        nc, sem_ptr, strides = sem.shape[c], sem.ctypes.data, (sem.strides[r], sem.strides[p], sem.strides[c])
    pixel = np.ascontiguousarray(pixel, np.int32).reshape(-1)
    n = pixel.shape[0]
    if recipe:
        if is_edge is None or np.asarray(is_edge).reshape(-1).shape[0] != n:
            raise ValueError("recipe rows need is_edge, one flag per pixel")
        edge = np.ascontiguousarray(np.asarray(is_edge).reshape(-1) != 0, np.uint8)
    else:
        if method is None:
            raise ValueError("give the method (DSO_EDGES or FULL), or recipe=True")
        edge = None
    ptr = lambda a: None if a is None else a.ctypes.data
    fs = _capi.cvo_rgbd_device_frame_t(frame.rows, frame.cols, frame.channels, ptr(frame.image), ptr(frame.gray), ptr(frame.depth),
                                       _capi.CVO_DEPTH_U16 if frame.depth.dtype == np.uint16 else _capi.CVO_DEPTH_F32,
                                       frame.fx, frame.fy, frame.cx, frame.cy, frame.scaling_factor, int(nc), sem_ptr, *[int(s) for s in strides])
    m = max(n, 1)
    xyz, feat, geo = np.zeros((m, 3), np.float32), np.zeros((m, FEATURE_DIMENSIONS), np.float32), np.zeros((m, 2), np.float32)
    label, excl = (np.zeros((m, NUM_CLASSES), np.float32) if nc else None), np.zeros(m, np.uint8)
    rc = L.cvo_rgbd_frame_rows_host(C.byref(fs), int(bool(recipe)), int(method if method is not None else DSO_EDGES), n,
                                    pixel.ctypes.data_as(C.POINTER(C.c_int)), None if edge is None else edge.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                    _fptr(xyz), _fptr(feat), _fptr(label), _fptr(geo), excl.ctypes.data_as(C.POINTER(C.c_ubyte)))
    if rc != 0:
        e = CvoError(f"error {rc}: cvo_rgbd_frame_rows_host refused the frame, the method or a pixel")
        e.code = rc
        raise e
    return dict(xyz=xyz[:n], feat=feat[:n], label=None if label is None else label[:n], geotype=geo[:n], excluded=excl[:n].astype(bool))


def _mat_to_c(T):
    a = np.ascontiguousarray(np.asarray(T, np.float32).reshape(4, 4).T).reshape(16)
    return a


def _mats_to_c(Ts, k, name):
    """k 4x4 matrices (row, col) -> 16 k floats, column-major each, as the C-ABI takes its transforms."""
    a = np.asarray(Ts, np.float32)
    if a.size != 16 * k or (k and a.shape[-2:] != (4, 4)):
        raise ValueError(f"{name}: one 4x4 matrix per frame")
    if k == 0:
        return np.zeros(16, np.float32)  # (never read)
    return np.ascontiguousarray(a.reshape(k, 4, 4).transpose(0, 2, 1)).reshape(16 * k)


def _kernel_to_c(kernel):
    a = np.asarray(kernel, np.float32)
    if a.shape != (3, 3):
        raise ValueError("kernel: a 3x3 matrix")
    return np.ascontiguousarray(a.T).reshape(9)


def _min_count(min_count):
    if int(min_count) != min_count or min_count < 0:
        raise ValueError("min_count: an integer >= 0")


def _mat4(T, name):
    a = np.asarray(T, np.float32)
    if a.shape != (4, 4):
        raise ValueError(f"{name}: a 4x4 matrix")
    return _mat_to_c(a)


class DepthFilter:
    """cvo_depth_filter_t: a keyframe's depths refined from later frames on the device (the last loops of
    main_depth_filtering.cpp; tests/np_depthfilter.py states the arithmetic).  CvoGPU.depth_filter_open makes one."""

    def __init__(self, gpu, keyframe):
        self.handle = None
        self.gpu, self.n = gpu, keyframe.n
        h = C.c_void_p()
        gpu._check(gpu.L.cvo_depth_filter_open(gpu.ctx, keyframe.handle, C.byref(h)))
        self.handle = h

    def _open(self):
        if not self.handle:
            raise ValueError("the depth filter is closed")

    def add(self, frame, T, kernel, T_depth):
        """cvo_depth_filter_add: one resident frame.  T and kernel (3x3, row / col) are compute_association_gpu_non_isotropic's
        with the keyframe as source; T_depth (4x4): its third row gives an associated point's depth in the keyframe's frame."""
        self._open()
        if not isinstance(frame, DeviceCloud):
            raise ValueError("add: the frame is a DeviceCloud (CvoGPU.upload makes one)")
        Tm, Td, kcm = _mat4(T, "T"), _mat4(T_depth, "T_depth"), _kernel_to_c(kernel)
        p = self.gpu.params.to_ctypes()
        self.gpu._check(self.gpu.L.cvo_depth_filter_add(self.handle, C.byref(p), frame.handle, _fptr(Tm), _fptr(Td), _fptr(kcm)))
        return self

    def state(self):
        """cvo_depth_filter_state -> (depth_sum float32[n], weight_sum float32[n], count int32[n]), original row order."""
        self._open()
        n = self.n
        ds, ws, cnt = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int32)
        self.gpu._check(self.gpu.L.cvo_depth_filter_state(self.handle, _fptr(ds), _fptr(ws), cnt.ctypes.data_as(C.POINTER(C.c_int))))
        return ds[:n], ws[:n], cnt[:n]

    def finish(self, min_count=3, return_kept=False):
        """cvo_depth_filter_finish: the refined keyframe as a DeviceCloud (rows with more than min_count observations, moved
        along their rays); return_kept: (cloud, kept original indices, refined depths, rows dropped as non-finite).  The state
        stays: more frames may follow."""
        self._open()
        _min_count(min_count)
        n = self.n
        kept, depth = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32)
        nk, nf, h = C.c_int(), C.c_int(), C.c_void_p()
        self.gpu._check(self.gpu.L.cvo_depth_filter_finish(self.handle, int(min_count), C.byref(h), kept.ctypes.data_as(C.POINTER(C.c_int)),
                                                           _fptr(depth), C.byref(nk), C.byref(nf)))
        out = self.gpu._adopt(h, nk.value)
        return (out, kept[:nk.value].copy(), depth[:nk.value].copy(), nf.value) if return_kept else out

    def debug_rows(self):
        """cvo_debug_depth_filter_rows: dict(empty, list, dense_slot, run, full, max_nnz, K, wide) - how the rows of the last
        add's matrix were stored and how many k_assoc_dense gave a whole block; valid until the context evaluates something else."""
        self._open()
        v = [C.c_int() for _ in range(8)]
        self.gpu._check(self.gpu.L.cvo_debug_depth_filter_rows(self.handle, *[C.byref(x) for x in v]))
        return dict(zip(("empty", "list", "dense_slot", "run", "full", "max_nnz", "K", "wide"), (x.value for x in v)))

    def close(self):
        if self.handle:
            self.gpu.L.cvo_depth_filter_close(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _raise_depth(rc, who):
    if rc != 0:
        raise CvoError(f"error {rc}: {who}")


def depth_filter_accumulate_host(row_ptr, col, val, target_xyz, T_depth, state=None):
    """cvo_depth_filter_accumulate_host: one frame's association (CSR over the keyframe's rows, columns ascending) folded into
    `state` = (depth_sum, weight_sum, count) - None: zeros - which is returned, updated in place.  No context."""
    rp = np.ascontiguousarray(row_ptr, np.int32).reshape(-1)
    if rp.size < 1:
        raise ValueError("row_ptr: n_rows + 1 entries")
    n = rp.size - 1
    c, v = np.ascontiguousarray(col, np.int32).reshape(-1), np.ascontiguousarray(val, np.float32).reshape(-1)
    if c.size != v.size or c.size < int(rp[-1]):
        raise ValueError("col / val: row_ptr[-1] entries each")
    y = np.ascontiguousarray(target_xyz, np.float32)
    if y.ndim != 2 or y.shape[1] != 3:
        raise ValueError("target_xyz: (m, 3)")
    Td = _mat4(T_depth, "T_depth")
    if state is None:
        state = (np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32))
    ds, ws, cnt = state
    for a, t in ((ds, np.float32), (ws, np.float32), (cnt, np.int32)):
        if not (isinstance(a, np.ndarray) and a.dtype == t and a.shape == (n,) and a.flags.c_contiguous):
            raise ValueError("state: (float32[n], float32[n], int32[n]), contiguous")
    ipp = C.POINTER(C.c_int)
    _raise_depth(_capi.lib().cvo_depth_filter_accumulate_host(n, rp.ctypes.data_as(ipp), c.ctypes.data_as(ipp), _fptr(v), y.shape[0], _fptr(y),
                                                              _fptr(Td), _fptr(ds), _fptr(ws), cnt.ctypes.data_as(ipp)),
                 "cvo_depth_filter_accumulate_host refused the association")
    return state


def depth_filter_finish_host(xyz, state, min_count=3):
    """cvo_depth_filter_finish_host -> (moved xyz of the kept rows (k, 3), kept original indices, refined depths, rows dropped as
    non-finite).  No context."""
    x = np.ascontiguousarray(xyz, np.float32)
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError("xyz: (n, 3)")
    n = x.shape[0]
    _min_count(min_count)
    ds, ws, cnt = (np.ascontiguousarray(state[0], np.float32), np.ascontiguousarray(state[1], np.float32), np.ascontiguousarray(state[2], np.int32))
    if ds.shape != (n,) or ws.shape != (n,) or cnt.shape != (n,):
        raise ValueError("state: three arrays of n entries")
    out, kept, depth = np.zeros((max(n, 1), 3), np.float32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32)
    nk, nf = C.c_int(), C.c_int()
    ipp = C.POINTER(C.c_int)
    _raise_depth(_capi.lib().cvo_depth_filter_finish_host(n, _fptr(x), _fptr(ds), _fptr(ws), cnt.ctypes.data_as(ipp), int(min_count), _fptr(out),
                                                          kept.ctypes.data_as(ipp), _fptr(depth), C.byref(nk), C.byref(nf)),
                 "cvo_depth_filter_finish_host refused its arguments")
    k = nk.value
    return out[:k].copy(), kept[:k].copy(), depth[:k].copy(), nf.value


class AlignResult:
    def __init__(self, ret, transform, info, trace=None):
        self.ret = ret
        self.transform = transform  # 4x4 float32 (row, col)
        self.iterations = info.iterations
        self.final_ell = info.final_ell
        self.final_num_neighbors = info.final_num_neighbors
        self.seconds = info.seconds
        self.trace = trace


class BatchQueue:
    """cvo_batch_open / _submit / _poll / _close: a stream of frame pairs through a fixed number of in-flight slots."""

    def __init__(self, gpu, slots, max_source_points, max_target_points, min_source_points=0, max_iterations=0):
        self.handle = None  # (set before anything can raise: close() / __del__ then have something to look at)
        self.gpu = gpu
        self.slots = slots
        o = _capi.cvo_align_opts_t()
        o.max_iterations = max_iterations
        p = gpu.params.to_ctypes()
        h = C.c_void_p()
        gpu._check(gpu.L.cvo_batch_open(gpu.ctx, C.byref(p), slots, max_source_points, max_target_points, min_source_points,
                                        C.byref(o), C.byref(h)))
        self.handle = h
        self._keep = {}
        gpu._queues.append(weakref.ref(self))  # (weak: a queue dropped without close() must still be collected)

    def submit(self, source, target, init, max_iterations=0):
        src, tgt = self.gpu._dev(source), self.gpu._dev(target)
        t = C.c_longlong()
        Tm = _mat_to_c(init)
        self.gpu._check(self.gpu.L.cvo_batch_submit(self.handle, src.handle, tgt.handle, _fptr(Tm), max_iterations, C.byref(t)))
        self._keep[t.value] = (src, tgt)  # the clouds must outlive the solve
        return t.value

    def poll(self, wait=1, capacity=None):
        """Finished pairs in submission order as AlignResult objects whose `.ticket` is the submission's ticket; wait:
        0 = just make progress, 1 = until one is ready, 2 = until everything submitted has finished."""
        cap = capacity or max(self.pending(), 1)
        buf = (_capi.cvo_batch_result_t * cap)()
        n = C.c_int()
        self.gpu._check(self.gpu.L.cvo_batch_poll(self.handle, wait, cap, buf, C.byref(n)))
        out = []
        for i in range(n.value):
            r = buf[i]
            T = np.array(list(r.transform), np.float32).reshape(4, 4).T.copy()
            res = AlignResult(r.info.ret, T, r.info)
            res.ticket = int(r.ticket)
            self._keep.pop(res.ticket, None)
            out.append(res)
        return out

    def pending(self):
        return int(self.gpu.L.cvo_batch_pending(self.handle))

    def stats(self):
        a, b, c = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        self.gpu._check(self.gpu.L.cvo_batch_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return {"chunks": a.value, "full_chunks": b.value, "refills": c.value}

    def close(self):
        if self.handle:
            self.gpu.L.cvo_batch_close(self.handle)
            self.handle = None
            self._keep = {}
            self.gpu._queues[:] = [w for w in self.gpu._queues if w() is not None and w() is not self]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CvoGPU:
    """cvo::CvoGPU(yaml) over the HIP backend."""

    def __init__(self, param_file=None, params=None, device=0, library=None):
        self.L = _capi.lib(library)  # (library: another build of the same C-ABI, e.g. an experiment build of build.build_variant)
        if params is not None:
            self.params = params
        elif param_file is not None:
            self.params = read_cvo_params_yaml(param_file)
        else:
            self.params = CvoParams()
        ctx = C.c_void_p()
        rc = self.L.cvo_ctx_create(device, C.byref(ctx))
        if rc != 0:
            raise CvoError(f"cvo_ctx_create(device={device}) failed with {rc}: is a HIP GPU visible?")
        self.ctx = ctx
        self.device = int(device)
        self._queues = []  # weak references to the live BatchQueue objects (closed before the context goes)
        self._maps = []    # ... and to the live SemanticMap objects

    def close(self):
        for w in list(getattr(self, "_queues", [])):
            q = w()
            if q is not None:
                q.close()
        for w in list(getattr(self, "_maps", [])):
            m = w()
            if m is not None:
                m.close()
        if getattr(self, "ctx", None):
            self.L.cvo_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc <= _capi.CVO_E_INVALID:
            raise CvoError(f"error {rc}: {self.L.cvo_last_error(self.ctx).decode()}")
        return rc

    def get_params(self):
        return self.params

    def set_option(self, name, value):
        """cvo_ctx_set_option: a tuning / diagnostic switch of this context (the CVO_<NAME> environment variables are read
        once, when the context is created); value None clears it."""
        v = None if value is None else str(value).encode()
        self._check(self.L.cvo_ctx_set_option(self.ctx, name.encode(), v))

    def write_params(self, p):
        """CvoGPU::write_params (CvoGPU.cu:73-77): the device copy is refreshed per call here."""
        self.params = p

    def upload(self, pc):
        return DeviceCloud(self, pc)

    def map_open(self, config=None, initial_voxels=0):
        """cvo_map_open: a semantic voxel map on this context (MapConfig; initial_voxels sizes the first table)."""
        return SemanticMap(self, config, initial_voxels)

    def _voxel_size(self, voxel_size):
        return float(self.params.multiframe_downsample_voxel_size if voxel_size is None else voxel_size)

    def voxel_select(self, xyz, voxel_size=None):
        """cvo_voxel_select: indices (int32, ascending) of the points a voxel grid of side `voxel_size` keeps - of every
        occupied voxel the point with the lowest index.  voxel_size None: params.multiframe_downsample_voxel_size."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        n = xyz.shape[0]
        kept = np.zeros(max(n, 1), np.int32)
        nk = C.c_int()
        self._check(self.L.cvo_voxel_select(self.ctx, n, _fptr(xyz), self._voxel_size(voxel_size),
                                            kept.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nk)))
        return kept[:nk.value].copy()

    def upload_voxel(self, pc, voxel_size=None):
        """cvo_cloud_upload_voxel: the resident cloud of the points voxel_select keeps (attributes follow their point);
        `.kept` holds their indices in `pc`.  Indistinguishable from upload(pc.select(kept))."""
        xyz, feat, label, geo = pc.device_arrays()
        n = xyz.shape[0]
        kept = np.zeros(max(n, 1), np.int32)
        nk = C.c_int()
        h = C.c_void_p()
        self._check(self.L.cvo_cloud_upload_voxel(self.ctx, n, _fptr(xyz), _fptr(feat), _fptr(label), _fptr(geo),
                                                  self._voxel_size(voxel_size), C.byref(h),
                                                  kept.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nk)))
        d = DeviceCloud.__new__(DeviceCloud)
        d.gpu, d.n, d._keep, d.handle = self, nk.value, None, h
        d.kept = kept[:nk.value].copy()
        return d

    def debug_voxel_stats(self):
        """cvo_debug_voxel_stats of the last selection on the device: a dict of capacity, occupied, probes_total,
        probe_longest, entered (all 0 after a selection on the host)."""
        v = [C.c_ulonglong() for _ in range(5)]
        self._check(self.L.cvo_debug_voxel_stats(self.ctx, *[C.byref(x) for x in v]))
        return dict(zip(("capacity", "occupied", "probes_total", "probe_longest", "entered"), [x.value for x in v]))

    def rgbd_points(self, frame, method):
        """cvo_rgbd_points: CvoPointCloud(ImageRGBD, Calibration, method) for method FULL / DSO_EDGES - a CvoPointCloud with
        F = channels + 2 and `.pixel`, the index v * cols + u of every point, in the reference's order."""
        rc, pc = _rgbd_points(lambda *a: self.L.cvo_rgbd_points(self.ctx, *a), frame, method)
        self._check(rc)
        return pc

    def upload_rgbd(self, frame, leaf=None, edge_divisor=4):
        """cvo_cloud_upload_rgbd: the multi-frame drivers' per-frame block as one call - the resident cloud of the voxel-selected
        edge points (grid leaf / edge_divisor, type (1, 0)) followed by the voxel-selected surface points (grid leaf, type
        (0, 1)); `.pixel` and `.is_edge` per point.  leaf None: params.multiframe_downsample_voxel_size."""
        cap = max(2 * frame.rows * frame.cols, 1)
        pixel, is_edge = np.zeros(cap, np.int32), np.zeros(cap, np.uint8)
        n = C.c_int()
        h = C.c_void_p()
        fs = frame.c_struct()
        self._check(self.L.cvo_cloud_upload_rgbd(self.ctx, C.byref(fs), self._voxel_size(leaf), float(edge_divisor), C.byref(h),
                                                 pixel.ctypes.data_as(C.POINTER(C.c_int)), is_edge.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                 C.byref(n)))
        d = DeviceCloud.__new__(DeviceCloud)
        d.gpu, d.n, d._keep, d.handle = self, n.value, None, h
        d.pixel, d.is_edge = pixel[:n.value].copy(), is_edge[:n.value].astype(bool)
        return d

    def _device_frame(self, frame):
        if not isinstance(frame, DeviceRGBDFrame):
            raise ValueError("a DeviceRGBDFrame is required (RGBDFrame holds host arrays: rgbd_points / upload_rgbd)")
        if frame.device != self.device:
            raise ValueError(f"the frame was described for device {frame.device}, the context is on {self.device}")
        _sync_producers(frame.tensors)
        return frame.c_struct()

    def upload_rgbd_points_device(self, frame, method, want_pixel=False):
        """cvo_cloud_from_rgbd_device: CvoPointCloud(ImageRGBD, Calibration, method), method FULL / DSO_EDGES, of a
        DeviceRGBDFrame as a resident cloud - the cloud upload(rgbd_points(f, method)) makes of the frame's host copy f, with no
        plane and no row crossing to the host.  want_pixel: `.pixel`, the index v * cols + u of every point (a copy down and a
        synchronisation more).  For tensors of a module that offers <module>.cuda.current_stream that stream is synchronised
        first; with raw addresses the caller has done so."""
        fs = self._device_frame(frame)
        pixel = np.zeros(max(frame.rows * frame.cols, 1), np.int32) if want_pixel else None
        n, h = C.c_int(), C.c_void_p()
        self._check(self.L.cvo_cloud_from_rgbd_device(self.ctx, C.byref(fs), int(method), C.byref(h), C.byref(n),
                                                      None if pixel is None else pixel.ctypes.data_as(C.POINTER(C.c_int))))
        d = self._adopt(h, n.value)
        if want_pixel:
            d.pixel = pixel[:n.value].copy()
        return d

    def upload_rgbd_device(self, frame, leaf=None, edge_divisor=4, want_pixel=False):
        """cvo_cloud_from_rgbd_device_recipe: upload_rgbd's cloud of a DeviceRGBDFrame; `.n_edge` edge points come first.
        want_pixel: `.pixel` and `.is_edge` per point, as upload_rgbd sets them."""
        fs = self._device_frame(frame)
        pixel = np.zeros(max(2 * frame.rows * frame.cols, 1), np.int32) if want_pixel else None
        n, ne, h = C.c_int(), C.c_int(), C.c_void_p()
        self._check(self.L.cvo_cloud_from_rgbd_device_recipe(self.ctx, C.byref(fs), self._voxel_size(leaf), float(edge_divisor), C.byref(h),
                                                             C.byref(n), C.byref(ne), None if pixel is None else pixel.ctypes.data_as(C.POINTER(C.c_int))))
        d = self._adopt(h, n.value)
        d.n_edge = ne.value
        if want_pixel:
            d.pixel, d.is_edge = pixel[:n.value].copy(), np.arange(n.value) < ne.value
        return d

    def debug_rgbd_stats(self):
        """cvo_debug_rgbd_stats of the last rgbd_points / upload_rgbd: potentials tried and the count at each, the standing
        selection, the points of both sets, the pixels with a depth, whether the kernels ran."""
        nt, pots, cnts, dev = C.c_int(), (C.c_int * 8)(), (C.c_int * 8)(), C.c_int()
        v = [C.c_ulonglong() for _ in range(4)]
        self._check(self.L.cvo_debug_rgbd_stats(self.ctx, C.byref(nt), pots, cnts, *[C.byref(x) for x in v], C.byref(dev)))
        out = dict(zip(("edge_selected", "edge_points", "surface_points", "with_depth"), [x.value for x in v]))
        out.update(potentials=list(pots[:nt.value]), counts=list(cnts[:nt.value]), on_device=bool(dev.value))
        return out

    def debug_rgbd_readback(self):
        """cvo_debug_rgbd_readback: the stages of the last selection that ran on the device (rgbd_points / stereo_points with
        DSO_EDGES, upload_rgbd, upload_stereo_recipe) -> dict(g2 (rows, cols) float32; ths, sm: all (cols // 32)(rows // 32)
        + 100 entries; selected: {potential: pixel indices in the compaction's order} for the potentials 2 .. 7)."""
        rows, cols, counts = C.c_int(), C.c_int(), (C.c_int * 6)()
        self._check(self.L.cvo_debug_rgbd_readback(self.ctx, C.byref(rows), C.byref(cols), counts, None, None, None, None))
        h, w, counts = rows.value, cols.value, list(counts)
        n_ths = (w // 32) * (h // 32) + 100
        g2, ths, sm = np.zeros((h, w), np.float32), np.zeros(n_ths, np.float32), np.zeros(n_ths, np.float32)
        sel = np.zeros(max(sum(counts), 1), np.int32)
        self._check(self.L.cvo_debug_rgbd_readback(self.ctx, None, None, None, _fptr(g2), _fptr(ths), _fptr(sm), sel.ctypes.data_as(C.POINTER(C.c_int))))
        at = np.concatenate([[0], np.cumsum(counts)])
        return dict(g2=g2, ths=ths, sm=sm, selected={2 + k: sel[at[k]:at[k + 1]].copy() for k in range(6)})

    def fast_select(self, gray, schedule=FAST_STEREO):
        """cvo_fast_select: as fast_select_host, by the context's route (switch STEREO_HOST)."""
        rc, pixel, used = _fast_select(lambda *a: self.L.cvo_fast_select(self.ctx, *a), gray, schedule)
        self._check(rc)
        return pixel, used

    def stereo_points(self, frame, method=CV_FAST):
        """cvo_stereo_points: CvoPointCloud(ImageStereo, Calibration, method) for method CV_FAST / DSO_EDGES / FULL from the frame's
        disparity - a CvoPointCloud with F = channels + 2 and `.pixel`, in the reference's order."""
        rc, pc = _rgbd_points(lambda *a: self.L.cvo_stereo_points(self.ctx, *a), frame, method)
        self._check(rc)
        return pc

    def _resident(self, h, n, pixel, is_edge=None):
        d = DeviceCloud.__new__(DeviceCloud)
        d.gpu, d.n, d._keep, d.handle = self, n, None, h
        d.pixel = pixel[:n].copy()
        if is_edge is not None:
            d.is_edge = is_edge[:n].astype(bool)
        return d

    def upload_stereo(self, frame, method=CV_FAST):
        """cvo_cloud_upload_stereo: the pairwise stereo driver's cloud - stereo_points' rows, resident (mono frames: the 3
        features zero-padded to 5); `.pixel` per point."""
        pixel = np.zeros(max(frame.rows * frame.cols, 1), np.int32)
        n, h, fs = C.c_int(), C.c_void_p(), frame.c_struct()
        self._check(self.L.cvo_cloud_upload_stereo(self.ctx, C.byref(fs), int(method), C.byref(h), pixel.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n)))
        return self._resident(h, n.value, pixel)

    def stereo_disparity(self, left, right, config=None, dfilter=None):
        """cvo_stereo_disparity: as stereo_disparity_host, by the context's route (switch SGM_HOST).  dfilter (a DFilterConfig):
        cvo_stereo_disparity_filtered - the matcher, then disparity_filter of its map, which stays on the device in between."""
        if dfilter is None:
            call = lambda *a: self.L.cvo_stereo_disparity(self.ctx, *a)  # noqa: E731
        else:
            df = dfilter.c_struct()
            call = lambda *a: self.L.cvo_stereo_disparity_filtered(self.ctx, *a[:-1], C.byref(df), a[-1])  # noqa: E731
        rc, out = _stereo_disparity(call, left, right, config)
        self._check(rc)
        return out

    def disparity_filter(self, disparity, config=None, out=None):
        """cvo_disparity_filter: as disparity_filter_host, by the context's route (switch DFILTER_HOST)."""
        rc, out = _disparity_filter(lambda *a: self.L.cvo_disparity_filter(self.ctx, *a), disparity, config, out)
        self._check(rc)
        return out

    def debug_dfilter_stats(self, readback=False):
        """cvo_debug_dfilter_stats of the last disparity_filter / filtered stereo_disparity / upload_stereo_pair -> dict(on_device,
        rows, cols, tile_w, tile_h, segments, removed, filled); readback: also the maps the device kept of the stages that ran -
        after_speckle, after_gap, mean_tmp (a stage that did not run: None)."""
        names = ("on_device", "rows", "cols", "tile_w", "tile_h")
        v = {k: C.c_int() for k in names}
        counts = (C.c_ulonglong * 3)()
        self._check(self.L.cvo_debug_dfilter_stats(self.ctx, *[C.byref(v[k]) for k in names], counts, None, None, None))
        out = {k: x.value for k, x in v.items()}
        out["on_device"] = bool(out["on_device"])
        out["segments"], out["removed"], out["filled"] = (int(c) for c in counts)
        if readback:
            fp = C.POINTER(C.c_float)
            for i, name in enumerate(("after_speckle", "after_gap", "mean_tmp")):
                m = np.zeros((out["rows"], out["cols"]), np.float32)
                ptrs = [None, None, None]
                ptrs[i] = m.ctypes.data_as(fp)
                rc = self.L.cvo_debug_dfilter_stats(self.ctx, None, None, None, None, None, None, *ptrs)
                out[name] = m if rc == 0 else None
        return out

    def upload_stereo_pair(self, frame, right_gray, config=None, method=CV_FAST, dfilter=None):
        """cvo_cloud_upload_stereo_pair: stereo_disparity of (the frame's gray plane, right_gray), then upload_stereo with that
        map; frame.disparity may be None and is not read.  dfilter (a DFilterConfig): cvo_cloud_upload_stereo_pair_filtered."""
        right = np.ascontiguousarray(right_gray, np.uint8)
        if right.shape != (frame.rows, frame.cols):
            raise ValueError(f"right_gray is {right.shape}, the frame {frame.rows} x {frame.cols}")
        pixel = np.zeros(max(frame.rows * frame.cols, 1), np.int32)
        n, h, fs, cfg = C.c_int(), C.c_void_p(), frame.c_struct(), (config or SGMConfig()).c_struct()
        rp, pp = right.ctypes.data_as(C.POINTER(C.c_ubyte)), pixel.ctypes.data_as(C.POINTER(C.c_int))
        if dfilter is None:
            self._check(self.L.cvo_cloud_upload_stereo_pair(self.ctx, C.byref(fs), rp, C.byref(cfg), int(method), C.byref(h), pp, C.byref(n)))
        else:
            df = dfilter.c_struct()
            self._check(self.L.cvo_cloud_upload_stereo_pair_filtered(self.ctx, C.byref(fs), rp, C.byref(cfg), C.byref(df), int(method), C.byref(h), pp,
                                                                     C.byref(n)))
        return self._resident(h, n.value, pixel)

    def debug_sgm_stats(self):
        """cvo_debug_sgm_stats of the last stereo_disparity / upload_stereo_pair."""
        names = ("on_device", "max_disparity", "paths", "rows", "cols", "tile_w", "tile_h")
        v = {k: C.c_int() for k in names}
        lines = (C.c_int * 8)()
        self._check(self.L.cvo_debug_sgm_stats(self.ctx, C.byref(v["on_device"]), C.byref(v["max_disparity"]), C.byref(v["paths"]), lines,
                                               C.byref(v["rows"]), C.byref(v["cols"]), C.byref(v["tile_w"]), C.byref(v["tile_h"])))
        out = {k: x.value for k, x in v.items()}
        out["on_device"], out["lines"] = bool(out["on_device"]), list(lines)
        return out

    def debug_sgm_readback(self):
        """cvo_debug_sgm_readback: the census planes and S of the last stereo_disparity that ran on the device ->
        dict(census_left, census_right (rows, cols) uint64, S (rows, cols, max_disparity) uint16)."""
        st = self.debug_sgm_stats()
        shape = (st["rows"], st["cols"])
        cl, cr, S = np.zeros(shape, np.uint64), np.zeros(shape, np.uint64), np.zeros(shape + (st["max_disparity"],), np.uint16)
        self._check(self.L.cvo_debug_sgm_readback(self.ctx, cl.ctypes.data_as(C.POINTER(C.c_ulonglong)), cr.ctypes.data_as(C.POINTER(C.c_ulonglong)),
                                                  S.ctypes.data_as(C.POINTER(C.c_ushort))))
        return dict(census_left=cl, census_right=cr, S=S)

    def upload_stereo_recipe(self, frame, leaf=None, edge_divisor=5):
        """cvo_cloud_upload_stereo_recipe: the multi-frame KITTI driver's per-frame block - upload_rgbd's recipe on the stereo
        points (edge grid leaf / edge_divisor, the driver's divisor is 5); `.pixel` and `.is_edge` per point."""
        cap = max(2 * frame.rows * frame.cols, 1)
        pixel, is_edge = np.zeros(cap, np.int32), np.zeros(cap, np.uint8)
        n, h, fs = C.c_int(), C.c_void_p(), frame.c_struct()
        self._check(self.L.cvo_cloud_upload_stereo_recipe(self.ctx, C.byref(fs), self._voxel_size(leaf), float(edge_divisor), C.byref(h),
                                                          pixel.ctypes.data_as(C.POINTER(C.c_int)), is_edge.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                                          C.byref(n)))
        return self._resident(h, n.value, pixel, is_edge)

    def debug_stereo_stats(self):
        """cvo_debug_stereo_stats of the last fast_select / stereo_points / upload_stereo / upload_stereo_recipe: thresholds (or
        potentials) tried and the count at each, the FAST threshold used, the 257 counts per FAST score -1 .. 255, candidates,
        kept, whether the kernels ran."""
        cap = 1024
        nt, used, dev = C.c_int(), C.c_int(), C.c_int()
        tried, cnts, hist = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_uint * 257)()
        cand, kept = C.c_ulonglong(), C.c_ulonglong()
        self._check(self.L.cvo_debug_stereo_stats(self.ctx, cap, C.byref(nt), tried, cnts, C.byref(used), hist, C.byref(cand), C.byref(kept), C.byref(dev)))
        k = min(nt.value, cap)
        return dict(tried=list(tried[:k]), counts=list(cnts[:k]), threshold_used=used.value, histogram=np.array(hist[:], np.int64),
                    candidates=cand.value, kept=kept.value, on_device=bool(dev.value))

    def lidar_select(self, scan, config, rand):
        """cvo_lidar_select: the LOAM point selection of CvoPointCloud(PointCloud<PointXYZI>::Ptr, n, beams) - edge_detection's
        indices, then LeGO-LOAM's - by the context's route (switch LIDAR_HOST) -> (indices, is_edge).  `rand` advances by the
        draws upstream would make."""
        rc, index, is_edge = _lidar_select(lambda *a: self.L.cvo_lidar_select(self.ctx, *a), scan, config, rand)
        self._check(rc)
        return index, is_edge

    def upload_lidar(self, scan, config, rand):
        """cvo_cloud_upload_lidar: the constructor's cloud - the selected points with F = 1 (intensity), type (1, 0) and, with
        semantics, one-hot labels - resident; `.pixel` is the point index per row."""
        index = np.zeros(max(2 * scan.n, 1), np.int32)
        n, h, s = C.c_int(), C.c_void_p(), scan.c_struct()
        self._check(self.L.cvo_cloud_upload_lidar(self.ctx, C.byref(s), C.byref(config.c), C.byref(rand.c), C.byref(h),
                                                  index.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n)))
        return self._resident(h, n.value, index)

    def debug_lidar_stats(self):
        """cvo_debug_lidar_stats of the last lidar_select / upload_lidar."""
        counts, dev = (C.c_ulonglong * 9)(), C.c_int()
        self._check(self.L.cvo_debug_lidar_stats(self.ctx, counts, C.byref(dev)))
        names = ("projected", "ground", "valid", "invalid", "segmented", "edges", "draws", "thinned", "edge_detected")
        out = dict(zip(names, (int(v) for v in counts)))
        out["on_device"] = bool(dev.value)
        return out

    def nlm_denoise(self, image, h=10, template_window=7, search_window=21, out=None):
        """cvo_nlm_denoise: as nlm_denoise_host, by the context's route (switch NLM_HOST)."""
        rc, dst = _nlm_denoise(lambda *a: self.L.cvo_nlm_denoise(self.ctx, *a), image, _nlm_config(h, template_window, search_window), out)
        self._check(rc)
        return dst

    def nlm_denoise_lab(self, lab, h=10, h_color=10, template_window=7, search_window=21, out=None):
        """cvo_nlm_denoise_lab: as nlm_denoise_lab_host, by the context's route: one upload, two launches, one download."""
        rc, dst = _nlm_denoise(lambda *a: self.L.cvo_nlm_denoise_lab(self.ctx, *a), lab, _nlm_config(h, template_window, search_window), out,
                               float(h_color))
        self._check(rc)
        return dst

    def debug_nlm_stats(self):
        """cvo_debug_nlm_stats of the last nlm_denoise / nlm_denoise_lab."""
        names = ("on_device", "mult", "shift", "n_nonzero", "tile_w", "tile_h", "table_in_lds")
        v = [C.c_int() for _ in names]
        self._check(self.L.cvo_debug_nlm_stats(self.ctx, *[C.byref(x) for x in v]))
        out = dict(zip(names, (x.value for x in v)))
        out["on_device"], out["table_in_lds"] = bool(out["on_device"]), bool(out["table_in_lds"])
        return out

    def upload_many(self, clouds, threads=None):
        """Uploads a list of clouds with cvo_cloud_upload_many: a pool of host threads inside the library, each cloud
        ordered / allocated / copied by one of them on its own stream (one ctypes call, the GIL is released for all of it)."""
        clouds = list(clouds)
        k = len(clouds)
        if k == 0:
            return []
        if threads is None:
            try:
                threads = len(os.sched_getaffinity(0))
            except AttributeError:
                threads = os.cpu_count() or 1
        threads = max(1, min(int(threads), k, 32))
        arrs = [pc.device_arrays() for pc in clouds]
        fpp = C.POINTER(C.c_float)
        n = (C.c_int * k)(*[a[0].shape[0] for a in arrs])

        def col(i):
            if all(a[i] is None for a in arrs):
                return None
            return (fpp * k)(*[_fptr(a[i]) if a[i] is not None else C.cast(None, fpp) for a in arrs])

        xyz = (fpp * k)(*[_fptr(a[0]) for a in arrs])
        out = (C.c_void_p * k)()
        self._check(self.L.cvo_cloud_upload_many(self.ctx, k, n, xyz, col(1), col(2), col(3), threads, out))
        res = []
        for i in range(k):
            d = DeviceCloud.__new__(DeviceCloud)
            d.gpu, d.n, d._keep, d.handle = self, int(n[i]), None, C.c_void_p(out[i])
            res.append(d)
        return res

    def _device_rows(self, xyz, feat=None, label=None, geotype=None, rows=None, n_records=None):
        """cvo_device_rows_t of one cloud (+ the objects to synchronise), refusing what the wrapper can see is wrong."""
        dev = self.device
        arrs = [_device_array("xyz", xyz, 3, "float32", dev), _device_array("feat", feat, FEATURE_DIMENSIONS, "float32", dev),
                _device_array("label", label, NUM_CLASSES, "float32", dev), _device_array("geotype", geotype, 2, "float32", dev)]
        idx = _device_array("rows", rows, None, "int32", dev)
        if xyz is None:
            raise ValueError("xyz is required")
        have = arrs[0][1]
        if n_records is None:
            n_records = have
        n_records = int(n_records)
        for name, (_, k, _) in zip(("xyz", "feat", "label", "geotype"), arrs):
            if k is not None and k < n_records:
                raise ValueError(f"{name} holds {k} records, n_records is {n_records}")
        n = have if rows is None else idx[1]
        if rows is None and n_records < n:
            raise ValueError(f"n_records ({n_records}) < n ({n}) without rows")
        d = _capi.cvo_device_rows_t(n, n_records, arrs[0][0], arrs[0][2], arrs[1][0], arrs[1][2], arrs[2][0], arrs[2][2],
                                    arrs[3][0], arrs[3][2], idx[0])
        return d, [a for a in (xyz, feat, label, geotype, rows) if hasattr(a, "data_ptr")]

    def upload_device(self, xyz, feat=None, label=None, geotype=None, rows=None, n_records=None):
        """cvo_cloud_from_device: a resident cloud from rows that are already in this context's device memory - no host copy.
        Every array is either an object with data_ptr() / stride() / shape / dtype / device (a torch tensor: (records, 3 | 5 |
        19 | 2) float32, inner stride 1, any row stride - a column slice of a wider tensor is fine) or a tuple (device address,
        records, row stride in bytes).  rows: optional int32 indices (a contiguous 1-D tensor, or (address, n)): point i is
        record rows[i].  n_records: how many records the arrays hold (default: xyz's).  For tensors of a module that offers
        <module>.cuda.current_stream, that stream is synchronised first; with raw addresses the caller has done so."""
        d, objs = self._device_rows(xyz, feat, label, geotype, rows, n_records)
        _sync_producers(objs)
        h = C.c_void_p()
        self._check(self.L.cvo_cloud_from_device(self.ctx, C.byref(d), C.byref(h)))
        return self._adopt(h, d.n)

    def upload_device_many(self, clouds):
        """cvo_cloud_from_device_many: a list of clouds - each a dict of upload_device's arguments, or a tuple of them in order -
        with one ingest launch, one read-back and one ordering launch."""
        specs = [self._device_rows(**c) if isinstance(c, dict) else self._device_rows(*c) for c in clouds]
        k = len(specs)
        if k == 0:
            return []
        _sync_producers([o for _, objs in specs for o in objs])
        arr = (_capi.cvo_device_rows_t * k)(*[d for d, _ in specs])
        out = (C.c_void_p * k)()
        self._check(self.L.cvo_cloud_from_device_many(self.ctx, k, arr, out))
        return [self._adopt(C.c_void_p(out[i]), arr[i].n) for i in range(k)]

    def upload_device_aos192(self, address, n):
        """cvo_cloud_from_device_aos192: n 192-byte CvoPoint records (CVO_POINT_DTYPE) at a device address."""
        h = C.c_void_p()
        self._check(self.L.cvo_cloud_from_device_aos192(self.ctx, int(n), C.c_void_p(int(address)), C.byref(h)))
        return self._adopt(h, int(n))

    def _adopt(self, handle, n):
        d = DeviceCloud.__new__(DeviceCloud)
        d.gpu, d.n, d._keep, d.handle = self, int(n), None, handle
        return d

    def merge_clouds(self, clouds, poses=None, voxel_size=0.0, return_kept=False):
        """cvo_cloud_merge: ONE resident cloud of the rows of `clouds` (DeviceCloud, in original order, cloud after cloud),
        each moved by its pose - poses: (len(clouds), 12) or (len(clouds), 3, 4) doubles, what multiframe_align_raw returns;
        None: nothing is moved - and, voxel_size > 0, thinned to the lowest global row of every voxel of that side.  Nothing
        comes down to the host.  The cloud upload_voxel (voxel_size 0: upload) makes of the same moved, concatenated rows.
        return_kept: (cloud, global indices of its points) instead of the cloud."""
        clouds = list(clouds)
        k = len(clouds)
        handles = (C.c_void_p * max(k, 1))(*[None if c is None else c.handle for c in clouds])
        P = None
        if poses is not None:
            P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1))
            if P.shape[0] != 12 * k:
                raise ValueError("poses: 12 entries per cloud")
        total = sum(c.n for c in clouds if c is not None)
        kept = np.zeros(max(total, 1), np.int32) if return_kept else None
        nk = C.c_int()
        h = C.c_void_p()
        self._check(self.L.cvo_cloud_merge(self.ctx, k, handles, None if P is None else P.ctypes.data_as(C.POINTER(C.c_double)),
                                           float(voxel_size), C.byref(h),
                                           None if kept is None else kept.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nk)))
        out = self._adopt(h, nk.value)
        return (out, kept[:nk.value].copy()) if return_kept else out

    def download(self, cloud):
        """DeviceCloud.download of a resident cloud."""
        return cloud.download()

    # -- keyframe depth filtering (main_depth_filtering.cpp:208-298) ----
    def depth_filter_open(self, keyframe):
        """cvo_depth_filter_open: a DepthFilter over a resident keyframe (DeviceCloud).  The filter copies what it needs: the
        keyframe may be freed afterwards."""
        if not isinstance(keyframe, DeviceCloud):
            raise ValueError("depth_filter_open: the keyframe is a DeviceCloud (CvoGPU.upload makes one)")
        return DepthFilter(self, keyframe)

    def depth_filter(self, keyframe, frames, Ts, T_depths, kernel, min_count=3, return_kept=False):
        """cvo_depth_filter: open, add every frame (Ts[k]: the association's transform, T_depths[k]: the one whose third row
        gives the depth in the keyframe's frame; 4x4 each), finish, close - one call.  The refined keyframe as a DeviceCloud;
        return_kept: (cloud, kept original indices, refined depths, rows dropped as non-finite)."""
        if not isinstance(keyframe, DeviceCloud):
            raise ValueError("depth_filter: the keyframe is a DeviceCloud (CvoGPU.upload makes one)")
        frames = list(frames)
        k = len(frames)
        if any(not isinstance(f, DeviceCloud) for f in frames):
            raise ValueError("depth_filter: every frame is a DeviceCloud")
        Tm, Td = _mats_to_c(Ts, k, "Ts"), _mats_to_c(T_depths, k, "T_depths")
        kcm = _kernel_to_c(kernel)
        _min_count(min_count)
        handles = (C.c_void_p * max(k, 1))(*[f.handle for f in frames])
        kept, depth = np.zeros(max(keyframe.n, 1), np.int32), np.zeros(max(keyframe.n, 1), np.float32)
        nk, nf, h = C.c_int(), C.c_int(), C.c_void_p()
        p = self.params.to_ctypes()
        self._check(self.L.cvo_depth_filter(self.ctx, C.byref(p), keyframe.handle, k, handles, _fptr(Tm), _fptr(Td), _fptr(kcm),
                                            int(min_count), C.byref(h), kept.ctypes.data_as(C.POINTER(C.c_int)), _fptr(depth),
                                            C.byref(nk), C.byref(nf)))
        out = self._adopt(h, nk.value)
        return (out, kept[:nk.value].copy(), depth[:nk.value].copy(), nf.value) if return_kept else out

    def debug_device_buffer(self, data, into=None):
        """cvo_debug_device_buffer: the bytes of a numpy array in device memory -> the device address; into: an address this
        call returned before, overwritten instead (the array must not be larger than that buffer)."""
        a = np.ascontiguousarray(data)
        d = C.c_void_p(into)
        self._check(self.L.cvo_debug_device_buffer(self.ctx, max(a.nbytes, 1), a.ctypes.data_as(C.c_void_p) if a.nbytes else None, C.byref(d)))
        return d.value

    def debug_device_release(self, address):
        self._check(self.L.cvo_debug_device_release(self.ctx, C.c_void_p(address)))

    def upload_aos192(self, records):
        """pcl_PointCloud_to_gpu: uploads an array of 192-byte CvoPoint records (dtype CVO_POINT_DTYPE)."""
        return DeviceCloudAoS(self, records)

    def _dev(self, pc):
        return pc if isinstance(pc, DeviceCloud) else DeviceCloud(self, pc)

    def _opts(self, max_iterations=0, ell0=None, K0=None, trace_capacity=0, trace_dense=0, trace_every=0,
              n_pairs=1, iters_per_launch=0, use_graph=0, kernel_clock=False):
        o = _capi.cvo_align_opts_t()
        o.max_iterations = max_iterations
        keep = []
        if ell0 is not None or K0 is not None:
            o.override_state = 1
            o.ell0 = self.params.ell_init if ell0 is None else ell0
            o.K0 = self.params.nearest_neighbors_max if K0 is None else K0
        if trace_capacity > 0:
            tr = (_capi.cvo_trace_t * (trace_capacity * n_pairs))()
            nt = (C.c_int * n_pairs)()
            o.trace = tr
            o.trace_capacity = trace_capacity
            o.trace_dense = trace_dense
            o.trace_every = trace_every
            o.n_trace = nt
            keep = [tr, nt]
        o.iters_per_launch = iters_per_launch
        o.use_graph = use_graph
        o.kernel_clock = 1 if kernel_clock else 0
        return o, keep

    def align(self, source, target, T_target_frame_to_source_frame, **kw):
        """CvoGPU::align (CvoGPU.cu:1605-1632).  Returns AlignResult (ret = 0 / -1)."""
        if source.num_points() == 0 or target.num_points() == 0 if not isinstance(source, DeviceCloud) else False:
            info = _capi.cvo_align_info_t()
            return AlignResult(0, None, info)  # transform untouched
        src, tgt = self._dev(source), self._dev(target)
        p = self.params.to_ctypes()
        init = _mat_to_c(T_target_frame_to_source_frame)
        out = np.zeros(16, np.float32)
        info = _capi.cvo_align_info_t()
        opts, keep = self._opts(**kw)
        rc = self.L.cvo_align_ex(self.ctx, C.byref(p), src.handle, tgt.handle, _fptr(init), _fptr(out),
                                 C.byref(info), C.byref(opts))
        self._check(rc)
        trace = None
        if keep:
            trace = [keep[0][i] for i in range(keep[1][0])]
        self._keepalive = keep
        return AlignResult(rc, out.reshape(4, 4).T.copy(), info, trace)

    def align_batch(self, sources, targets, inits, **kw):
        """n independent pairs solved concurrently on this context's GPU (cvo_align_batch)."""
        n = len(sources)
        src = [self._dev(s) for s in sources]
        tgt = [self._dev(t) for t in targets]
        sh = (C.c_void_p * n)(*[s.handle for s in src])
        th = (C.c_void_p * n)(*[t.handle for t in tgt])
        init = np.concatenate([_mat_to_c(T) for T in inits]).astype(np.float32)
        out = np.zeros(16 * n, np.float32)
        infos = (_capi.cvo_align_info_t * n)()
        p = self.params.to_ctypes()
        opts, keep = self._opts(n_pairs=n, **kw)
        rc = self.L.cvo_align_batch(self.ctx, C.byref(p), n, sh, th, _fptr(init), _fptr(out), infos, C.byref(opts))
        self._check(rc)
        res = []
        cap = opts.trace_capacity
        for i in range(n):
            trace = None
            if keep:
                trace = [keep[0][i * cap + t] for t in range(keep[1][i])]
            res.append(AlignResult(infos[i].ret, out[16 * i:16 * i + 16].reshape(4, 4).T.copy(), infos[i], trace))
        self._keepalive = keep
        return res

    def open_queue(self, slots, max_source_points, max_target_points, min_source_points=0, max_iterations=0):
        """A batch queue (cvo_batch_open): `slots` pairs in flight, finished pairs hand their slot to the next submitted
        one at a chunk boundary, results in submission order."""
        return BatchQueue(self, slots, max_source_points, max_target_points, min_source_points, max_iterations)

    def align_stream(self, sources, targets, inits, slots=64, max_iterations=0, limits=None):
        """All pairs through a batch queue of `slots` in-flight slots; returns their AlignResults in submission order
        (limits: per-pair iteration limits)."""
        src = [self._dev(s) for s in sources]
        tgt = [self._dev(t) for t in targets]
        if not src:  # (the C++ veneer returns an empty result likewise)
            return []
        q = self.open_queue(slots, max(s.n for s in src), max(t.n for t in tgt), min(s.n for s in src), max_iterations)
        try:
            for k, (s, t, T) in enumerate(zip(src, tgt, inits)):
                q.submit(s, t, T, limits[k] if limits else 0)
            out = []
            while q.pending():
                out.extend(q.poll(wait=2))
            return out
        finally:
            q.close()

    def align_association(self, n_source, pair=0, capacity=None):
        """The Association `align()` exports under is_exporting_association (CvoGPU.cu:1552-1556): CSR of the kernel
        matrix of the last executed iteration of pair `pair` of the last align call, + (stride_written, stride_read)."""
        row_ptr = np.zeros(n_source + 1, np.int32)
        nnz, kw, kr = C.c_size_t(), C.c_int(), C.c_int()
        ipt = C.POINTER(C.c_int)
        rc = self.L.cvo_align_association(self.ctx, pair, row_ptr.ctypes.data_as(ipt), None, None, 0, C.byref(nnz),
                                          C.byref(kw), C.byref(kr))
        if rc != _capi.CVO_E_NOMEM:
            self._check(rc)
        cap = nnz.value if capacity is None else capacity
        col, val = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.float32)
        self._check(self.L.cvo_align_association(self.ctx, pair, row_ptr.ctypes.data_as(ipt), col.ctypes.data_as(ipt),
                                                 _fptr(val), cap, C.byref(nnz), C.byref(kw), C.byref(kr)))
        return row_ptr, col[:nnz.value], val[:nnz.value], kw.value, kr.value

    def poses_to_device(self, dst_ptr, n):
        self._check(self.L.cvo_batch_poses_to_device(self.ctx, C.c_void_p(dst_ptr), n))

    def inner_product_gpu(self, source, target, T, ell):
        src, tgt = self._dev(source), self._dev(target)
        p = self.params.to_ctypes()
        out = C.c_float()
        Tm = _mat_to_c(T)
        self._check(self.L.cvo_inner_product(self.ctx, C.byref(p), src.handle, tgt.handle, _fptr(Tm), ell,
                                             C.byref(out)))
        return out.value

    def function_angle(self, source, target, T, ell, is_approximate=True):
        src, tgt = self._dev(source), self._dev(target)
        p = self.params.to_ctypes()
        out = C.c_float()
        Tm = _mat_to_c(T)
        self._check(self.L.cvo_function_angle(self.ctx, C.byref(p), src.handle, tgt.handle, _fptr(Tm), ell,
                                              1 if is_approximate else 0, C.byref(out)))
        return out.value

    def _score_batch(self, fn, sources, targets, Ts, ells, *extra):
        n = len(sources)
        if len(targets) != n or len(Ts) != n:
            raise CvoError(f"{n} sources, {len(targets)} targets, {len(Ts)} transforms: one of each per job")
        ell = np.asarray(ells, np.float32)
        ell = np.full(n, ell, np.float32) if ell.ndim == 0 else np.ascontiguousarray(ell)
        if ell.shape != (n,):
            raise CvoError(f"ells: a scalar or {n} values, got shape {ell.shape}")
        up = {}  # CvoPointCloud -> DeviceCloud, keyed by object identity: a cloud of several jobs goes up once

        def dev(pc):
            if isinstance(pc, DeviceCloud):
                return pc
            if id(pc) not in up:
                up[id(pc)] = (pc, DeviceCloud(self, pc))
            return up[id(pc)][1]

        src = [dev(s) for s in sources]
        tgt = [dev(t) for t in targets]
        sh = (C.c_void_p * max(n, 1))(*[s.handle for s in src])
        th = (C.c_void_p * max(n, 1))(*[t.handle for t in tgt])
        Tm = np.concatenate([_mat_to_c(T) for T in Ts]).astype(np.float32) if n else np.zeros(16, np.float32)
        out = np.zeros(max(n, 1), np.float32)
        p = self.params.to_ctypes()
        self._check(fn(self.ctx, C.byref(p), n, sh, th, _fptr(Tm), _fptr(ell if n else np.zeros(1, np.float32)), *extra,
                       _fptr(out)))
        return out[:n]

    def inner_product_batch(self, sources, targets, Ts, ells):
        """inner_product_gpu for many (source, target, T, ell) jobs in one call (cvo_inner_product_batch): np.float32[n],
        every value bit-identical to inner_product_gpu's.  ells: one per job or a scalar."""
        return self._score_batch(self.L.cvo_inner_product_batch, sources, targets, Ts, ells)

    def function_angle_batch(self, sources, targets, Ts, ells, is_approximate=True):
        """function_angle for many jobs in one call (cvo_function_angle_batch): np.float32[n], bit-identical to
        function_angle's.  The exact form evaluates <X, X> / <Y, Y> once per distinct cloud and ell."""
        return self._score_batch(self.L.cvo_function_angle_batch, sources, targets, Ts, ells, 1 if is_approximate else 0)

    def debug_last_score_batch(self):
        """(overlap evaluations, chain evaluations, launches) of the last score call, single or batched: e.g. (1, 0, 1)
        for an inner_product_gpu no row voids, (3, 0, 1) for an exact function_angle of two distinct clouds."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._check(self.L.cvo_debug_last_score_batch(self.ctx, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def compute_association_gpu(self, source, target, T, lengthscale):
        """Association::pairs as CSR (row_ptr, col, val) (CvoGPU.cu:1876-1911)."""
        src, tgt = self._dev(source), self._dev(target)
        n = src.n
        p = self.params.to_ctypes()
        cap = n * min(self.params.nearest_neighbors_max, tgt.n)
        row_ptr = np.zeros(n + 1, np.int32)
        col = np.zeros(max(cap, 1), np.int32)
        val = np.zeros(max(cap, 1), np.float32)
        nnz = C.c_size_t()
        Tm = _mat_to_c(T)
        self._check(self.L.cvo_association(self.ctx, C.byref(p), src.handle, tgt.handle, _fptr(Tm), lengthscale,
                                           row_ptr.ctypes.data_as(C.POINTER(C.c_int)),
                                           col.ctypes.data_as(C.POINTER(C.c_int)), _fptr(val), cap, C.byref(nnz)))
        return row_ptr, col[:nnz.value], val[:nnz.value]

    def compute_association_gpu_non_isotropic(self, source, target, T, kernel):
        """Association under the Mahalanobis kernel d^T kernel^-1 d, as CSR (CvoGPU.cu:1913-1995)."""
        src, tgt = self._dev(source), self._dev(target)
        n = src.n
        p = self.params.to_ctypes()
        cap = n * min(self.params.nearest_neighbors_max, tgt.n)
        row_ptr = np.zeros(n + 1, np.int32)
        col = np.zeros(max(cap, 1), np.int32)
        val = np.zeros(max(cap, 1), np.float32)
        nnz = C.c_size_t()
        Tm = _mat_to_c(T)
        kcm = np.ascontiguousarray(np.asarray(kernel, np.float32).reshape(3, 3).T).reshape(9)
        self._check(self.L.cvo_association_non_isotropic(self.ctx, C.byref(p), src.handle, tgt.handle, _fptr(Tm), _fptr(kcm),
                                                         row_ptr.ctypes.data_as(C.POINTER(C.c_int)),
                                                         col.ctypes.data_as(C.POINTER(C.c_int)), _fptr(val), cap,
                                                         C.byref(nnz)))
        return row_ptr, col[:nnz.value], val[:nnz.value]

    # -- multi-frame edge kernel (BinaryStateGPU::update_inner_product, IRLS_State_GPU.cu:43-79) ----
    def transformed(self, cloud, pose_3x4):
        """CvoFrameGPU::transform_pointcloud: a new resident cloud moved by a 3x4 row-major pose."""
        src = self._dev(cloud)
        pose = np.ascontiguousarray(np.asarray(pose_3x4, np.float64).reshape(12).astype(np.float32))
        h = C.c_void_p()
        self._check(self.L.cvo_cloud_transformed(self.ctx, src.handle, _fptr(pose), C.byref(h)))
        out = DeviceCloud.__new__(DeviceCloud)
        out.gpu, out.n, out._keep, out.handle = self, src.n, None, h
        return out

    def edge_kernel_matrix(self, frame1, frame2, ell, num_neighbors):
        """fill_in_A_mat_gpu on two transformed frames -> (mat, ind, nonzeros, nonzero_sum) in the reference's host
        layout ([n1 x K] row-major, 0 / -1 padded)."""
        f1, f2 = self._dev(frame1), self._dev(frame2)
        K = int(num_neighbors)
        mat = np.zeros((f1.n, K), np.float32)
        ind = np.zeros((f1.n, K), np.int32)
        nz = np.zeros(f1.n, np.uint32)
        total = C.c_uint()
        p = self.params.to_ctypes()
        self._check(self.L.cvo_edge_kernel_matrix(self.ctx, C.byref(p), f1.handle, f2.handle, float(ell), K, _fptr(mat),
                                                  ind.ctypes.data_as(C.POINTER(C.c_int)),
                                                  nz.ctypes.data_as(C.POINTER(C.c_uint)), C.byref(total)))
        return mat, ind, nz, total.value

    # -- multi-frame align (CvoGPU::align over frames and edges, CvoGPU.cu:1637-1683) ----------------
    def align_multiframe(self, frames, hold_const, edges, trace=False):
        """cvo_multiframe_align on CvoFrameGPU objects: edges = (frame1, frame2) pairs, as frames or as indices into
        `frames`; hold_const: one flag per frame (None = none held).  Updates every frame's pose_vec (and its transformed
        cloud); returns
        (info, trace rows) - info a dict of cvo_multiframe_info_t, the rows dicts of cvo_multiframe_trace_t ([] unless
        trace)."""
        frames = list(frames)
        F = len(frames)
        pos = {id(f): i for i, f in enumerate(frames)}
        flat = []
        for a, b in edges:
            for f in (a, b):
                flat.append(int(f) if isinstance(f, (int, np.integer)) else pos[id(f)])
        E = len(flat) // 2
        handles = (C.c_void_p * max(F, 1))(*[f._init.handle for f in frames])
        poses = np.ascontiguousarray(np.concatenate([np.asarray(f.pose_vec, np.float64).reshape(12) for f in frames])
                                     if F else np.zeros(12), np.float64)
        hold = None if hold_const is None else np.ascontiguousarray([1 if h else 0 for h in hold_const], np.int32)
        if hold is not None and hold.shape[0] != F:
            raise ValueError("hold_const: one flag per frame")
        ed = np.ascontiguousarray(flat if E else [0, 0], np.int32)
        info = _capi.cvo_multiframe_info_t()
        cap = max(self.params.multiframe_max_iters + 2, 1) if trace else 0
        rows = (_capi.cvo_multiframe_trace_t * max(cap, 1))()
        n_trace = C.c_int()
        p = self.params.to_ctypes()
        ip = C.POINTER(C.c_int)
        self._check(self.L.cvo_multiframe_align(
            self.ctx, C.byref(p), F, handles, poses.ctypes.data_as(C.POINTER(C.c_double)),
            None if hold is None else hold.ctypes.data_as(ip), E, ed.ctypes.data_as(ip), C.byref(info), rows, cap,
            C.byref(n_trace)))
        for i, f in enumerate(frames):
            f.pose_vec[:] = poses[12 * i:12 * i + 12]
            f.transform_pointcloud()  # the transformed copy follows the new pose (as CvoGPU::align does in C++)
        names = [n for n, _ in _capi.cvo_multiframe_trace_t._fields_]
        out = [{n: getattr(rows[i], n) for n in names} for i in range(n_trace.value)]
        return {n: getattr(info, n) for n, _ in _capi.cvo_multiframe_info_t._fields_}, out

    def multiframe_align_raw(self, clouds, poses, hold_const, edges, trace_capacity=0):
        """cvo_multiframe_align as it is: clouds (DeviceCloud or None), poses (F x 12, copied), hold_const (None or F
        ints), edges (flat ints).  Returns (rc, poses, info, trace rows, n_trace); rc is not checked (argument tests)."""
        F = len(clouds)
        handles = (C.c_void_p * max(F, 1))(*[None if c is None else c.handle for c in clouds])
        P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1) if F else np.zeros(12), np.float64).copy()
        hold = None if hold_const is None else np.ascontiguousarray(hold_const, np.int32)
        ed = np.ascontiguousarray(list(edges) if len(edges) else [0, 0], np.int32)
        info = _capi.cvo_multiframe_info_t()
        rows = (_capi.cvo_multiframe_trace_t * max(trace_capacity, 1))()
        n_trace = C.c_int(-7)
        p = self.params.to_ctypes()
        ip = C.POINTER(C.c_int)
        rc = self.L.cvo_multiframe_align(self.ctx, C.byref(p), F, handles, P.ctypes.data_as(C.POINTER(C.c_double)),
                                         None if hold is None else hold.ctypes.data_as(ip), len(edges) // 2,
                                         ed.ctypes.data_as(ip), C.byref(info), rows, trace_capacity, C.byref(n_trace))
        return rc, P, info, rows, n_trace.value

    def debug_irls_normal(self, frame1, frame2, pose1, pose2):
        """cvo_debug_irls_normal: k_irls_normal over the kernel matrix of the last evaluation (edge_kernel_matrix) with
        the UNtransformed clouds frame1 / frame2 at 3x4 poses -> (cost, g[12], H 12x12 symmetric)."""
        f1, f2 = self._dev(frame1), self._dev(frame2)
        a = np.ascontiguousarray(np.asarray(pose1, np.float64).reshape(12))
        b = np.ascontiguousarray(np.asarray(pose2, np.float64).reshape(12))
        out = np.zeros(91, np.float64)
        dp = C.POINTER(C.c_double)
        self._check(self.L.cvo_debug_irls_normal(self.ctx, f1.handle, f2.handle, a.ctypes.data_as(dp),
                                                 b.ctypes.data_as(dp), out.ctypes.data_as(dp)))
        H = np.zeros((12, 12))
        H[np.triu_indices(12)] = out[13:]
        H = H + np.triu(H, 1).T
        return out[0], out[1:13].copy(), H

    def debug_irls_eval(self, clouds, poses, edge_frames, slot_off, ent_r, ent_c, ent_w, normal=True):
        """cvo_debug_irls_eval: k_irls_eval + k_irls_finish on a caller-made table.  clouds: resident untransformed
        clouds; poses: F x 12; edge_frames: E x 2; slot_off: E + 1 offsets into ent_r / ent_c (int32) / ent_w (float32),
        c < 0 an empty slot.  Returns E x 91 doubles (cost, g[12], upper H[78]) or, cost-only, E doubles.  Raises on
        any index out of range (checked on the host before a launch)."""
        devs = [self._dev(c) for c in clouds]
        F = len(devs)
        handles = (C.c_void_p * max(F, 1))(*[d.handle for d in devs])
        X = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1) if F else np.zeros(12))
        ef = np.ascontiguousarray(np.asarray(edge_frames, np.int32).reshape(-1))
        E = ef.shape[0] // 2
        so = np.ascontiguousarray(slot_off, np.int32)
        r, c = np.ascontiguousarray(ent_r, np.int32), np.ascontiguousarray(ent_c, np.int32)
        w = np.ascontiguousarray(ent_w, np.float32)
        if X.shape[0] != 12 * max(F, 1) or so.shape[0] != E + 1 or not (r.shape == c.shape == w.shape) or \
                (E and r.shape[0] < so[-1]):
            raise ValueError("debug_irls_eval: array sizes do not match")
        out = np.zeros((E, 91) if normal else (E,), np.float64)
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        pad = np.zeros(1, np.int32)
        self._check(self.L.cvo_debug_irls_eval(
            self.ctx, F, handles, X.ctypes.data_as(dp), E, (ef if E else pad).ctypes.data_as(ip), so.ctypes.data_as(ip),
            (r if r.size else pad).ctypes.data_as(ip), (c if c.size else pad).ctypes.data_as(ip),
            _fptr(w if w.size else np.zeros(1, np.float32)), 1 if normal else 0,
            (out if E else np.zeros(1)).ctypes.data_as(dp)))
        return out

    def debug_irls_gather(self, n_rows, K):
        """cvo_debug_irls_gather: the entry list k_irls_gather makes of the last evaluation (edge_kernel_matrix with
        this K) -> (r, c, w), each [n_rows x K] by sorted position; slots past a row's count are (-1, -1, 0)."""
        r = np.zeros((n_rows, K), np.int32)
        c = np.zeros((n_rows, K), np.int32)
        w = np.zeros((n_rows, K), np.float32)
        ip = C.POINTER(C.c_int)
        self._check(self.L.cvo_debug_irls_gather(self.ctx, K, r.ctypes.data_as(ip), c.ctypes.data_as(ip), _fptr(w)))
        return r, c, w

    # -- test / profiling hooks --------------------------------------------------------------------
    def debug_last_ell(self, n_rows, K):
        mat = np.zeros((n_rows, K), np.float32)
        ind = np.zeros((n_rows, K), np.int32)
        nz = np.zeros(n_rows, np.uint32)
        self._check(self.L.cvo_debug_last_ell(self.ctx, K, _fptr(mat), ind.ctypes.data_as(C.POINTER(C.c_int)),
                                              nz.ctypes.data_as(C.POINTER(C.c_uint))))
        return mat, ind, nz

    def debug_time_scan(self, reps=20):
        ms = C.c_float()
        self._check(self.L.cvo_debug_time_scan(self.ctx, reps, C.byref(ms)))
        return ms.value

    def debug_time_kernels(self, reps=20):
        a, c = C.c_float(), C.c_float()
        self._check(self.L.cvo_debug_time_kernels(self.ctx, reps, C.byref(a), C.byref(c)))
        return a.value, c.value

    def debug_kernel_clock(self):
        """(k_assoc ms, k_coeff ms, intervals): average duration per pair and launch inside the last align call's
        optimiser loop, from the device clock (needs CVO_KERNEL_CLOCK=1 in the environment at context creation)."""
        a, c, n = C.c_float(), C.c_float(), C.c_ulonglong()
        self._check(self.L.cvo_debug_kernel_clock(self.ctx, C.byref(a), C.byref(c), C.byref(n)))
        return a.value, c.value, n.value

    def debug_last_geometry(self):
        """(sub-batches of the last call, pairs per sub-batch): the k_scan launches a profiler sees."""
        g, p = C.c_int(), C.c_int()
        self._check(self.L.cvo_debug_last_geometry(self.ctx, C.byref(g), C.byref(p)))
        return g.value, p.value

    def debug_scan_stats(self):
        """(tiles executed by k_scan during the last align call, rows per tile, targets per tile)."""
        t, r, c = C.c_ulonglong(), C.c_int(), C.c_int()
        self._check(self.L.cvo_debug_scan_stats(self.ctx, C.byref(t), C.byref(r), C.byref(c)))
        return t.value, r.value, c.value

    def debug_list_builds(self):
        b, it, ce = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        self._check(self.L.cvo_debug_list_builds(self.ctx, C.byref(b), C.byref(it), C.byref(ce)))
        return b.value, it.value, ce.value

    def debug_row_classes(self, pair=0):
        """(overflow rows, rows scanned literally, dense regime) of pair `pair` as its last list build left them."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._check(self.L.cvo_debug_row_classes(self.ctx, pair, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, bool(c.value)

    def debug_speculation(self, pair=0):
        """(iterations adopted from the speculative update, iterations run) of pair `pair` of the last align call."""
        a, it = C.c_int(), C.c_int()
        self._check(self.L.cvo_debug_speculation(self.ctx, pair, C.byref(a), C.byref(it)))
        return a.value, it.value

    def advice(self):
        """Performance-relevant observations about the process set-up (cvo_ctx_advice): "" when there is nothing to say,
        e.g. a text about GPU_MAX_HW_QUEUES when HIP was initialised with fewer than 8 hardware queues."""
        return self.L.cvo_ctx_advice(self.ctx).decode()

    def debug_scalar_math(self, op, items):
        """Runs one of the device's scalar routines (k_scalar_math ops 0-6, 8-11) on `items` (n x <=16 doubles); returns
        n x 16 doubles.  op 7 (indicator windows): items = [window, threshold, x_0, ...], returns the n decisions.
        ops 8-11 (hoisted division / exp against the plain forms): eight operands per item, out[:, 2l] plain,
        out[:, 2l+1] hoisted."""
        dp = C.POINTER(C.c_double)
        if op == 7:
            a = np.ascontiguousarray(items, np.float64).reshape(-1)
            n = a.shape[0] - 2
            out = np.zeros(n, np.float64)
        else:
            it = np.atleast_2d(np.asarray(items, np.float64))
            n = it.shape[0]
            a = np.zeros((n, 16), np.float64)
            a[:, :it.shape[1]] = it
            out = np.zeros((n, 16), np.float64)
        self._check(self.L.cvo_debug_scalar_math(self.ctx, op, n, a.ctypes.data_as(dp), out.ctypes.data_as(dp)))
        return out

    def debug_prim(self, op, n, m, k64, a, b):
        """Runs one shared device primitive (cvo_debug_prim of include/cvo_hip_debug.h, which lists the ops and the layouts) on
        copies of the arrays k64 (uint64), a and b (uint32); returns the three as the device left them."""
        k64, a, b = np.array(k64, np.uint64).reshape(-1), np.array(a, np.uint32).reshape(-1), np.array(b, np.uint32).reshape(-1)
        ptr = lambda x, t: x.ctypes.data_as(C.POINTER(t)) if x.size else None
        self._check(self.L.cvo_debug_prim(self.ctx, op, n, m, ptr(k64, C.c_ulonglong), k64.size, ptr(a, C.c_uint), a.size,
                                          ptr(b, C.c_uint), b.size))
        return k64, a, b

    def debug_device_memory(self):
        """(free, total) bytes of this context's device."""
        f, t = C.c_size_t(), C.c_size_t()
        self._check(self.L.cvo_debug_device_memory(self.ctx, C.byref(f), C.byref(t)))
        return f.value, t.value

    def debug_verified_rows(self):
        v = C.c_ulonglong()
        self._check(self.L.cvo_debug_verified_rows(self.ctx, C.byref(v)))
        return v.value

    def debug_last_candidates(self):
        v = C.c_ulonglong()
        self._check(self.L.cvo_debug_last_candidates(self.ctx, C.byref(v)))
        return v.value


class CvoFrameGPU:
    """cvo::CvoFrameGPU (CvoFrameGPU.hpp:14-36): a point cloud under a 3x4 row-major pose; transform_pointcloud()
    refreshes the transformed copy resident on the device."""

    def __init__(self, gpu, pts, poses):
        self.gpu = gpu
        self.points = pts
        self.pose_vec = np.asarray(poses, np.float64).reshape(12).copy()
        self._init = gpu.upload(pts)
        self._transformed = None
        self.transform_pointcloud()

    def transform_pointcloud(self):
        if self._transformed is not None:
            self._transformed.free()
        self._transformed = self.gpu.transformed(self._init, self.pose_vec)

    def points_transformed_gpu(self):
        return self._transformed


class BinaryStateGPU:
    """cvo::BinaryStateGPU (IRLS_State_GPU.hpp:21-89) without the Ceres half: update_inner_product() recomputes the
    edge's kernel matrix from the two frames' current transformed clouds, with the reference's neighbour-count
    adaptation (IRLS_State_GPU.cu:45-47)."""

    def __init__(self, frame1, frame2, num_neighbor, init_ell):
        self.frame1, self.frame2 = frame1, frame2
        self.init_num_neighbors = int(num_neighbor)
        self.num_neighbors = int(num_neighbor)
        self.ell = float(init_ell)
        self.iter = 0
        self.mat = self.ind = self.nonzeros = None
        self.nonzero_sum = 0

    def update_inner_product(self):
        last = int(self.nonzeros.max()) if self.nonzeros is not None and self.nonzeros.size else 0
        if last > 0:
            self.num_neighbors = min(self.init_num_neighbors, int(last * 1.1))
        gpu = self.frame1.gpu
        self.mat, self.ind, self.nonzeros, self.nonzero_sum = gpu.edge_kernel_matrix(
            self.frame1.points_transformed_gpu(), self.frame2.points_transformed_gpu(), self.ell, self.num_neighbors)
        self.iter += 1
        return self.nonzero_sum
