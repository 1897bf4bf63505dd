"""The surface of "clouds from rows already on the device" without a GPU: the new entry points are declared, bound and
exported; the test hooks stay in the debug header; the ctypes record matches the C one; and CvoGPU.upload_device refuses
what it can see is wrong before it touches the library."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import cases
from unified_cvo_amd import CvoGPU, _capi

NEW = ("cvo_cloud_from_device", "cvo_cloud_from_device_many", "cvo_cloud_from_device_aos192")
HOOKS = ("cvo_debug_device_buffer", "cvo_debug_device_release")
CC = shutil.which("gcc") or shutil.which("cc") or shutil.which("g++")


def _header(name):
    return open(os.path.join(cases.ROOT, "include", name)).read()


def test_entry_points_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _header("cvo_hip.h"), flags=re.S)
    for sym in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), sym
        assert sym in _capi.EXPORTED, sym
    assert "cvo_device_rows_t" in text


def test_library_exports_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    for sym in NEW + HOOKS:
        assert sym in exported, sym


def test_hooks_are_only_in_the_debug_header():
    boundary, debug = _header("cvo_hip.h"), _header("cvo_hip_debug.h")
    for sym in HOOKS:
        assert sym not in boundary and re.search(r"\bint\s+%s\s*\(" % sym, debug), sym
        assert sym in _capi.EXPORTED


@pytest.mark.skipif(CC is None, reason="no host C compiler")
def test_ctypes_record_matches_the_header(tmp_path):
    fields = [n for n, _ in _capi.cvo_device_rows_t._fields_]
    assert fields == ["n", "n_records", "xyz", "xyz_stride", "feat", "feat_stride", "label", "label_stride", "geotype",
                      "geotype_stride", "rows"]
    src = tmp_path / "rows_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cvo_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(cvo_device_rows_t));\n'
                   + "".join(f'  printf(" %zu", offsetof(cvo_device_rows_t, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "rows_layout"
    subprocess.check_call([CC, "-Wall", "-Werror", "-I", os.path.join(cases.ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(_capi.cvo_device_rows_t)] + [getattr(_capi.cvo_device_rows_t, f).offset for f in fields]
    assert got == want


class FakeDevice:
    def __init__(self, type_, index):
        self.type, self.index = type_, index


class FakeTensor:
    """What CvoGPU.upload_device reads of a tensor.  data_ptr() raises: a refusal must come before the address is taken."""

    def __init__(self, shape, stride=None, dtype="fake.float32", device=("cuda", 0)):
        self.shape, self.dtype, self.device = tuple(shape), dtype, FakeDevice(*device)
        self._stride = tuple(stride) if stride else tuple(
            int(__import__("math").prod(shape[i + 1:])) for i in range(len(shape)))

    def stride(self):
        return self._stride

    def data_ptr(self):
        raise AssertionError("the wrapper took the address of a tensor it had to refuse")


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} for arguments it had to refuse")


@pytest.fixture
def wrapper():
    """A CvoGPU without a context or a library: any call into either fails the test."""
    g = CvoGPU.__new__(CvoGPU)
    g.L, g.ctx, g.device = NoLibrary(), None, 0
    return g


def test_wrapper_refuses_float64(wrapper):
    with pytest.raises(TypeError, match="float32"):
        wrapper.upload_device(FakeTensor((10, 3), dtype="fake.float64"))
    with pytest.raises(TypeError, match="int32"):
        wrapper.upload_device((4096, 10, 12), rows=FakeTensor((10,), dtype="fake.int64"))


def test_wrapper_refuses_another_device(wrapper):
    with pytest.raises(ValueError, match="device 1"):
        wrapper.upload_device(FakeTensor((10, 3), device=("cuda", 1)))
    with pytest.raises(ValueError, match="host tensor"):
        wrapper.upload_device(FakeTensor((10, 3), device=("cpu", None)))


def test_wrapper_refuses_a_non_unit_inner_stride(wrapper):
    with pytest.raises(ValueError, match="inner stride 2"):
        wrapper.upload_device((4096, 10, 12), label=FakeTensor((10, 19), stride=(64, 2)))
    with pytest.raises(ValueError, match=r"\(records, 19\)"):
        wrapper.upload_device((4096, 10, 12), label=FakeTensor((10, 20)))


def test_wrapper_refuses_too_few_records(wrapper):
    with pytest.raises(ValueError, match="without rows"):
        wrapper.upload_device((4096, 10, 12), n_records=5)
    with pytest.raises(ValueError, match="holds 8 records"):
        wrapper.upload_device((4096, 10, 12), feat=(8192, 8, 20))
