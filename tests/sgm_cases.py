"""Inputs of the stereo matcher's tests (test_sgm_cpu.py, test_gpu_sgm.py, test_cpp_sgm.py) and a cache of the statement's
stages (np_sgm.stages), computed once per (case, shape, configuration) and shared, read-only."""
import numpy as np

import np_sgm

_cache = {}

# (rows, cols, D, d0, seed): the shift cases whose properties test_sgm_cpu.py asserts on the statement; the last three sit
# on the seams of the kernels' 64 lanes over d
SHIFT_CASES = ((24, 100, 64, 17, 0), (40, 160, 64, 40, 1), (24, 150, 128, 63, 2), (24, 150, 128, 64, 3), (16, 300, 256, 129, 4))


def noise(rows, cols, seed=0):
    """independent uint8 planes -> (left, right)"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (rows, cols), dtype=np.uint8), rng.integers(0, 256, (rows, cols), dtype=np.uint8)


def shift(rows, cols, d0, seed=0):
    """right is noise; left[:, d0:] = right[:, :cols - d0], the left d0 columns noise: the true disparity is d0 from column d0 on"""
    rng = np.random.default_rng(seed)
    right = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    left = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    if d0 < cols:
        left[:, d0:] = right[:, :cols - d0]
    return left, right


def two_planes(rows, cols, seed=0, d_top=10, d_bottom=30):
    """right: 2 x 2 box-filtered noise; the rows above the middle shifted by d_top, those below by d_bottom -> (left, right, truth)"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (rows + 1, cols + 1)).astype(np.int32)
    right = ((raw[:-1, :-1] + raw[:-1, 1:] + raw[1:, :-1] + raw[1:, 1:] + 2) >> 2).astype(np.uint8)
    left = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    truth = np.empty((rows, cols), np.int32)
    half = rows // 2
    for r0, r1, d in ((0, half, d_top), (half, rows, d_bottom)):
        if d < cols:
            left[r0:r1, d:] = right[r0:r1, :cols - d]
        truth[r0:r1] = d
    return left, right, truth


def constant_right(rows, cols, seed=0):
    """left noise, right constant: both census planes of the right are 0, every cost of a pixel ties over u - d >= 0"""
    return noise(rows, cols, seed)[0], np.full((rows, cols), 90, np.uint8)


def planes(kind, rows, cols, seed=0, d0=0):
    if kind == "noise":
        return noise(rows, cols, seed)
    if kind == "shift":
        return shift(rows, cols, d0, seed)
    if kind == "two_planes":
        return two_planes(rows, cols, seed)[:2]
    if kind == "constant_right":
        return constant_right(rows, cols, seed)
    raise ValueError(kind)


def statement(kind, rows, cols, seed=0, d0=0, **config):
    """np_sgm.stages of a case, cached"""
    key = (kind, rows, cols, seed, d0, tuple(sorted(config.items())))
    if key not in _cache:
        st = np_sgm.stages(*planes(kind, rows, cols, seed, d0), **config)
        for v in st.values():
            v.setflags(write=False)
        _cache[key] = st
    return _cache[key]


def refusals():
    """(what, rows, cols, config overrides, code name) - of test_sgm_cpu.py and test_gpu_sgm.py"""
    return [("rows", 0, 5, {}, "INVALID"), ("cols", 5, 0, {}, "INVALID"), ("D 0", 5, 5, dict(max_disparity=0), "INVALID"),
            ("D 96", 5, 5, dict(max_disparity=96), "INVALID"), ("D 512", 5, 5, dict(max_disparity=512), "INVALID"),
            ("p1 < 0", 5, 5, dict(p1=-1), "INVALID"), ("p1 > p2", 5, 5, dict(p1=121), "INVALID"), ("p2 194", 5, 5, dict(p2=194), "INVALID"),
            ("uniqueness -1", 5, 5, dict(uniqueness=-1), "INVALID"), ("uniqueness 100", 5, 5, dict(uniqueness=100), "INVALID"),
            ("paths 5", 5, 5, dict(paths=5), "INVALID"), ("paths 0", 5, 5, dict(paths=0), "INVALID"),
            ("pixels", 4097, 4096, {}, "UNSUPPORTED"), ("workspace", 4096, 2048, dict(max_disparity=256), "UNSUPPORTED")]
