"""The surface of "device-frame RGB-D front end" without a GPU: the entry points are declared in the boundary header, bound with
matching argument counts and exported by the library; the ctypes mirror of cvo_rgbd_device_frame_t matches the C struct; the
kernels are part of the kernel set and share ONE copy of the row and exclusion arithmetic with the host routes and the twin;
NULL arguments are refused without a device; the Python wrapper refuses what it can see is wrong before it touches the library."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases
from unified_cvo_amd import CvoGPU, DeviceRGBDFrame, RGBDFrame, _capi, rgbd_frame_rows_host

NEW = {"cvo_cloud_from_rgbd_device": 6, "cvo_cloud_from_rgbd_device_recipe": 8, "cvo_rgbd_frame_rows_host": 11}
SHARED = ("rgbd_excluded", "rgbd_gradient_at", "rgbd_features", "rgbd_recipe_row")
CC = shutil.which("gcc") or shutil.which("cc") or shutil.which("g++")


def _read(*path):
    return open(os.path.join(cases.ROOT, *path)).read()


def test_entry_points_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _read("include", "cvo_hip.h"), flags=re.S)
    L = _capi.lib()
    for sym, n in NEW.items():
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), sym
        assert sym in _capi.EXPORTED, sym
        assert len(getattr(L, sym).argtypes) == n, sym
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % sym, text, flags=re.S).group(1)
        assert len(decl.split(",")) == n, (sym, decl)   # the binding has as many arguments as the declaration
    assert "cvo_rgbd_device_frame_t" in text
    whole = _read("include", "cvo_hip.h")
    assert "RGBD_HOST and its crossover do not apply" in whole and "DENSE (no strides)" in whole   # the header says so


def test_library_exports_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    for sym in NEW:
        assert sym in exported, sym


@pytest.mark.skipif(CC is None, reason="no host C compiler")
def test_ctypes_record_matches_the_header(tmp_path):
    fields = [n for n, _ in _capi.cvo_rgbd_device_frame_t._fields_]
    assert fields == ["rows", "cols", "channels", "image", "gray", "depth", "depth_type", "fx", "fy", "cx", "cy", "scaling_factor",
                      "num_classes", "semantic", "semantic_row_stride", "semantic_pixel_stride", "semantic_class_stride"]
    src = tmp_path / "frame_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cvo_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(cvo_rgbd_device_frame_t));\n'
                   + "".join(f'  printf(" %zu", offsetof(cvo_rgbd_device_frame_t, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "frame_layout"
    subprocess.check_call([CC, "-Wall", "-Werror", "-I", os.path.join(cases.ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(_capi.cvo_rgbd_device_frame_t)] + [getattr(_capi.cvo_rgbd_device_frame_t, f).offset for f in fields]
    assert got == want


def test_kernels_are_part_of_the_kernel_set():
    assert '#include "cvo_k_rgbd_rows.h"' in _read("unified_cvo_amd", "csrc", "cvo_kernels.h")
    kernels = _read("unified_cvo_amd", "csrc", "cvo_k_rgbd_rows.h")
    assert re.search(r"__global__ __launch_bounds__\(\w+\) void k_rgbd_rows\(", kernels)
    for pred in ("struct RgbdKeepScores", "struct RgbdHasDepth"):
        assert pred in kernels, pred
    # ONE copy of the arithmetic: defined __host__ __device__ in the kernel header, called by the kernels there and by the host section
    host = _read("unified_cvo_amd", "csrc", "cvo_rgbd.hip")
    for f in SHARED:
        assert re.search(r"__host__ __device__ inline \w+ %s\(" % f, kernels), f
        assert len(re.findall(r"\b%s\(" % f, kernels)) >= 2, f          # the definition and a call
        if f != "rgbd_gradient_at":                                     # (the host reaches the gradient through rgbd_features)
            assert re.search(r"\b%s\(" % f, host), f
    for other in ("cvo_rgbd.hip", "cvo_stereo.hip", "cvo_k_rgbd.h"):
        assert not re.search(r"/ 255\.0|/ 500\.0", _read("unified_cvo_amd", "csrc", other)), other   # no second copy of the divisions
    assert "fma" not in kernels.replace("multiply-add", "")
    from unified_cvo_amd import build
    assert "-ffp-contract=off" in build.HIPCC_FLAGS


def test_null_arguments_are_refused_without_a_device():
    L = _capi.lib()
    assert L.cvo_cloud_from_rgbd_device(None, None, 2, None, None, None) == _capi.CVO_E_INVALID
    assert L.cvo_cloud_from_rgbd_device_recipe(None, None, 0.1, 4.0, None, None, None, None) == _capi.CVO_E_INVALID
    assert L.cvo_rgbd_frame_rows_host(None, 0, 8, 0, None, None, None, None, None, None, None) == _capi.CVO_E_INVALID
    img, dep = np.zeros((4, 8, 3), np.uint8), np.ones((4, 8), np.uint16)
    fs = _capi.cvo_rgbd_device_frame_t(4, 8, 3, img.ctypes.data, None, dep.ctypes.data, 0, 5.0, 5.0, 4.0, 2.0, 5000.0, 0, None, 0, 0, 0)
    assert L.cvo_rgbd_frame_rows_host(C.byref(fs), 0, 8, -1, None, None, None, None, None, None, None) == _capi.CVO_E_INVALID
    assert L.cvo_rgbd_frame_rows_host(C.byref(fs), 0, 8, 1, None, None, None, None, None, None, None) == _capi.CVO_E_INVALID   # n > 0 without pixels
    assert L.cvo_rgbd_frame_rows_host(C.byref(fs), 0, 0, 0, None, None, None, None, None, None, None) == _capi.CVO_E_UNSUPPORTED  # CV_FAST
    assert L.cvo_rgbd_frame_rows_host(C.byref(fs), 0, 8, 0, None, None, None, None, None, None, None) == _capi.CVO_OK
    sem = np.zeros((4, 8, 19), np.float32)
    for strides in ((0, 76, 4), (608, 0, 4), (608, 76, 0), (608, 76, 6), (606, 76, 4)):
        fs = _capi.cvo_rgbd_device_frame_t(4, 8, 3, img.ctypes.data, None, dep.ctypes.data, 0, 5.0, 5.0, 4.0, 2.0, 5000.0, 19, sem.ctypes.data, *strides)
        assert L.cvo_rgbd_frame_rows_host(C.byref(fs), 0, 8, 0, None, None, None, None, None, None, None) == _capi.CVO_E_INVALID, strides
    fs = _capi.cvo_rgbd_device_frame_t(4, 8, 3, img.ctypes.data, None, dep.ctypes.data, 0, 5.0, 5.0, 4.0, 2.0, 5000.0, 20, sem.ctypes.data, 640, 80, 4)
    assert L.cvo_rgbd_frame_rows_host(C.byref(fs), 0, 8, 0, None, None, None, None, None, None, None) == _capi.CVO_E_UNSUPPORTED


class FakeDevice:
    def __init__(self, type_, index):
        self.type, self.index = type_, index


class FakeTensor:
    """What DeviceRGBDFrame reads of a tensor.  refused=True: data_ptr() raises - a refusal must come before the address is taken."""

    def __init__(self, shape, stride=None, dtype="fake.uint8", device=("cuda", 0), refused=False):
        self.shape, self.dtype, self.device, self.refused = tuple(shape), dtype, FakeDevice(*device), refused
        self._stride = tuple(stride) if stride else tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape)))

    def stride(self):
        return self._stride

    def data_ptr(self):
        if self.refused:
            raise AssertionError("the wrapper took the address of a tensor it had to refuse")
        return 4096


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} for arguments it had to refuse")


IMAGE, DEPTH = FakeTensor((48, 64, 3)), FakeTensor((48, 64), dtype="fake.float32")
CAL = (50.0, 50.0, 32.0, 24.0, 1.0)


def test_frame_takes_strides_from_the_tensor():
    f = DeviceRGBDFrame(IMAGE, DEPTH, *CAL, semantic=FakeTensor((19, 48, 64), dtype="fake.float32"), layout="chw")
    assert (f.rows, f.cols, f.channels, f.num_classes) == (48, 64, 3, 19)
    assert f.semantic_strides == (4 * 64, 4, 4 * 48 * 64) and f.depth_type == _capi.CVO_DEPTH_F32
    f = DeviceRGBDFrame(IMAGE, DEPTH, *CAL, semantic=FakeTensor((48, 64, 19), stride=(64 * 32, 32, 1), dtype="fake.float32"))
    assert f.semantic_strides == (4 * 64 * 32, 4 * 32, 4)   # a column slice of a wider tensor
    f = DeviceRGBDFrame((4096, 48, 64, 1), (8192, "u16"), *CAL, gray=(12288,), semantic=(16384, 19, 4864, 76, 4))
    s = f.c_struct()
    assert (s.rows, s.cols, s.channels, s.depth_type, s.num_classes, s.semantic_pixel_stride) == (48, 64, 1, _capi.CVO_DEPTH_U16, 19, 76)
    assert (s.image, s.depth, s.gray, s.semantic) == (4096, 8192, 12288, 16384)


def test_frame_refuses_before_the_library():
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        DeviceRGBDFrame(FakeTensor((48, 64, 3), stride=(64 * 4, 4, 1), refused=True), DEPTH, *CAL)
    with pytest.raises(ValueError, match=r"depth\.contiguous\(\)"):
        DeviceRGBDFrame(IMAGE, FakeTensor((48, 64), stride=(128, 2), dtype="fake.float32", refused=True), *CAL)
    with pytest.raises(ValueError, match=r"gray\.contiguous\(\)"):
        DeviceRGBDFrame(IMAGE, DEPTH, *CAL, gray=FakeTensor((48, 64), stride=(1, 48), refused=True))
    with pytest.raises(TypeError, match="uint8"):
        DeviceRGBDFrame(FakeTensor((48, 64, 3), dtype="fake.float32", refused=True), DEPTH, *CAL)
    with pytest.raises(TypeError, match="float32"):
        DeviceRGBDFrame(IMAGE, FakeTensor((48, 64), dtype="fake.float64", refused=True), *CAL)
    with pytest.raises(TypeError, match="float32"):
        DeviceRGBDFrame(IMAGE, DEPTH, *CAL, semantic=FakeTensor((48, 64, 19), dtype="fake.float16", refused=True))
    with pytest.raises(ValueError, match="layout"):
        DeviceRGBDFrame(IMAGE, DEPTH, *CAL, semantic=FakeTensor((48, 64, 19), dtype="fake.float32", refused=True), layout="whc")
    with pytest.raises(ValueError, match="layout 'chw'"):
        DeviceRGBDFrame(IMAGE, DEPTH, *CAL, semantic=FakeTensor((48, 64, 19), dtype="fake.float32", refused=True), layout="chw")
    with pytest.raises(ValueError, match="host tensor"):
        DeviceRGBDFrame(FakeTensor((48, 64, 3), device=("cpu", None), refused=True), DEPTH, *CAL)
    with pytest.raises(ValueError, match="device 1"):
        DeviceRGBDFrame(IMAGE, DEPTH, *CAL, semantic=FakeTensor((48, 64, 19), dtype="fake.float32", device=("cuda", 1), refused=True))
    with pytest.raises(ValueError, match="depth is"):
        DeviceRGBDFrame(IMAGE, FakeTensor((48, 63), dtype="fake.float32", refused=True), *CAL)
    with pytest.raises(ValueError, match="rows, cols, channels"):
        DeviceRGBDFrame((4096, 48, 64), (8192, "u16"), *CAL)


def test_wrapper_refuses_before_the_library():
    g = CvoGPU.__new__(CvoGPU)
    g.L, g.ctx, g.device, g.params = NoLibrary(), None, 0, cases.load_params("geometric_gpu")
    host = RGBDFrame(np.zeros((4, 8, 3), np.uint8), np.ones((4, 8), np.uint16), 5, 5, 4, 2, 5000)
    for call in (lambda f: g.upload_rgbd_points_device(f, 8), lambda f: g.upload_rgbd_device(f, 0.1)):
        with pytest.raises(ValueError, match="DeviceRGBDFrame"):
            call(host)
        with pytest.raises(ValueError, match="device 1"):
            call(DeviceRGBDFrame((4096, 4, 8, 3), (8192, "u16"), 5, 5, 4, 2, 5000, device=1))
    with pytest.raises(ValueError, match="layout"):
        rgbd_frame_rows_host(host, [0], 8, semantic=np.zeros((4, 8, 19), np.float32), layout="cwh")
    with pytest.raises(ValueError, match="float32"):
        rgbd_frame_rows_host(host, [0], 8, semantic=np.zeros((4, 8, 19), np.float64))
    with pytest.raises(ValueError, match="layout 'chw'"):
        rgbd_frame_rows_host(host, [0], 8, semantic=np.zeros((4, 8, 19), np.float32), layout="chw")
    with pytest.raises(ValueError, match="method"):
        rgbd_frame_rows_host(host, [0])
