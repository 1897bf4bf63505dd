"""Inputs of the denoising tests (test_nlm_cpu.py, test_gpu_nlm.py, test_cpp_nlm.py) and a cache of the statement's outputs
(np_nlm.denoise), computed once per (case, shape, channels, h, windows) and shared."""
import numpy as np

import np_nlm

KINDS = ("steps", "constant", "white", "checker", "random")
_cache = {}


def image(kind, rows, cols, channels=1, seed=0):
    """(rows, cols) for one channel, else (rows, cols, channels), uint8.
    steps: clip(base + N(0, 8)) over a two-level base per axis (0 / 120 left / right, + 60 on the lower half);
    constant: 200 everywhere; white: 255 everywhere - at sw = 21 est reaches its maximum, 441 mult 255;
    checker: 0 / 255 by pixel parity - every non-centre weight is 0, output = input; random: uniform bytes."""
    rng = np.random.default_rng([seed, rows, cols, channels, KINDS.index(kind)])
    shape = (rows, cols, channels)
    if kind == "steps":
        base = np.zeros(shape)
        base[:, cols // 2:] = 120
        base[rows // 2:] += 60
        base += 15 * np.arange(channels)
        img = np.clip(base + rng.normal(0, 8, shape), 0, 255)
    elif kind == "constant":
        img = np.full(shape, 200)
    elif kind == "white":
        img = np.full(shape, 255)
    elif kind == "checker":
        y, x = np.mgrid[0:rows, 0:cols]
        img = np.repeat((((y + x) & 1) * 255)[..., None], channels, 2)
    else:
        img = rng.integers(0, 256, shape)
    img = np.ascontiguousarray(img.astype(np.uint8))
    return img[..., 0].copy() if channels == 1 else img


def statement(kind, rows, cols, channels=1, h=10, windows=(7, 21), seed=0):
    key = (kind, rows, cols, channels, float(h), tuple(windows), seed)
    if key not in _cache:
        out = np_nlm.denoise(image(kind, rows, cols, channels, seed), h, *windows)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def statement_lab(kind, rows, cols, h=10, h_color=10, windows=(7, 21), seed=0):
    key = ("lab", kind, rows, cols, float(h), float(h_color), tuple(windows), seed)
    if key not in _cache:
        out = np_nlm.denoise_lab(image(kind, rows, cols, 3, seed), h, h_color, *windows)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def refusals():
    """(what, rows, cols, channels, h, template_window, search_window, h_color, code name) - of test_nlm_cpu.py and test_gpu_nlm.py"""
    return [("rows", 0, 5, 1, 10, 7, 21, 10, "INVALID"), ("cols", 5, 0, 1, 10, 7, 21, 10, "INVALID"), ("channels 0", 5, 5, 0, 10, 7, 21, 10, "INVALID"),
            ("channels 4", 5, 5, 4, 10, 7, 21, 10, "INVALID"), ("h 0", 5, 5, 1, 0, 7, 21, 10, "INVALID"), ("h < 0", 5, 5, 1, -1, 7, 21, 10, "INVALID"),
            ("h nan", 5, 5, 1, float("nan"), 7, 21, 10, "INVALID"), ("h inf", 5, 5, 1, float("inf"), 7, 21, 10, "INVALID"),
            ("template 0", 5, 5, 1, 10, 0, 21, 10, "INVALID"), ("search 0", 5, 5, 1, 10, 7, 0, 10, "INVALID"),
            ("h_color 0", 5, 5, 3, 10, 7, 21, 0, "INVALID"), ("h_color nan", 5, 5, 3, 10, 7, 21, float("nan"), "INVALID"),
            ("th 4", 5, 5, 1, 10, 8, 20, 10, "UNSUPPORTED"), ("th 4 odd", 5, 5, 1, 10, 9, 21, 10, "UNSUPPORTED"),
            ("sh 11", 5, 5, 1, 10, 7, 22, 10, "UNSUPPORTED"), ("pixels", 4097, 4096, 1, 10, 7, 21, 10, "UNSUPPORTED")]
