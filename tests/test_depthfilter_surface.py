"""The surface of "keyframe depth filtering on the device" without a GPU: the entry points are declared in the boundary header,
bound and exported by the library; the one test hook lives in the debug header; the kernels are part of the kernel set and
share their arithmetic with the CPU twin; the Python wrappers refuse wrong arguments before they touch the library."""
import os
import re
import subprocess

import numpy as np
import pytest

import cases
from unified_cvo_amd import CvoError, CvoGPU, DepthFilter, DeviceCloud, _capi, depth_filter_accumulate_host, depth_filter_finish_host

NEW = ("cvo_depth_filter_open", "cvo_depth_filter_add", "cvo_depth_filter_size", "cvo_depth_filter_state", "cvo_depth_filter_finish",
       "cvo_depth_filter", "cvo_depth_filter_accumulate_host", "cvo_depth_filter_finish_host")


def _read(*path):
    return open(os.path.join(cases.ROOT, *path)).read()


def test_entry_points_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _read("include", "cvo_hip.h"), flags=re.S)
    for sym in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), sym
        assert sym in _capi.EXPORTED, sym
    assert re.search(r"\bvoid\s+cvo_depth_filter_close\s*\(", text) and "cvo_depth_filter_close" in _capi.EXPORTED
    assert "cvo_debug_" not in text
    dbg = re.sub(r"/\*.*?\*/", "", _read("include", "cvo_hip_debug.h"), flags=re.S)
    assert re.search(r"\bint\s+cvo_debug_depth_filter_rows\s*\(", dbg) and "cvo_debug_depth_filter_rows" in _capi.EXPORTED


def test_library_exports_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    for sym in NEW + ("cvo_depth_filter_close", "cvo_debug_depth_filter_rows"):
        assert sym in exported, sym


def test_bindings_have_argument_types():
    L = _capi.lib()
    want = dict(cvo_depth_filter_open=3, cvo_depth_filter_add=6, cvo_depth_filter_size=1, cvo_depth_filter_state=4, cvo_depth_filter_finish=7,
                cvo_depth_filter_close=1, cvo_depth_filter=14, cvo_depth_filter_accumulate_host=10, cvo_depth_filter_finish_host=11,
                cvo_debug_depth_filter_rows=9)
    text = re.sub(r"/\*.*?\*/", "", _read("include", "cvo_hip.h") + _read("include", "cvo_hip_debug.h"), flags=re.S)
    for sym, n in want.items():
        assert len(getattr(L, sym).argtypes) == n, sym
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % sym, text, flags=re.S).group(1)
        assert len(decl.split(",")) == n, (sym, decl)   # the binding has as many arguments as the declaration


def test_kernels_are_part_of_the_kernel_set():
    assert '#include "cvo_k_depth.h"' in _read("unified_cvo_amd", "csrc", "cvo_kernels.h")
    assert '#include "cvo_depth.hip"' in _read("unified_cvo_amd", "csrc", "cvo_hip.hip")
    text = _read("unified_cvo_amd", "csrc", "cvo_k_depth.h")
    for k in ("k_depth_accumulate", "k_depth_finish"):
        assert re.search(r"__global__ __launch_bounds__\(\w+\) void %s\(" % k, text), k
    assert '#include "cvo_depth_math.h"' in text
    # the twin and the kernels call the ONE copy of the arithmetic, and nothing in it fuses
    host = _read("unified_cvo_amd", "csrc", "cvo_depth.hip")
    for f in ("depth_zj", "depth_fold", "depth_finish_row"):
        assert f + "(" in host and f + "(" in text, f
    assert "fma" not in _read("unified_cvo_amd", "csrc", "cvo_depth_math.h").replace("multiply-add", "")


def test_null_arguments_are_refused_without_a_device():
    L = _capi.lib()
    assert L.cvo_depth_filter_open(None, None, None) == _capi.CVO_E_INVALID
    assert L.cvo_depth_filter_add(None, None, None, None, None, None) == _capi.CVO_E_INVALID
    assert L.cvo_depth_filter_state(None, None, None, None) == _capi.CVO_E_INVALID
    assert L.cvo_depth_filter_finish(None, 3, None, None, None, None, None) == _capi.CVO_E_INVALID
    assert L.cvo_depth_filter(None, None, None, 0, None, None, None, None, 3, None, None, None, None, None) == _capi.CVO_E_INVALID
    assert L.cvo_depth_filter_size(None) == 0
    L.cvo_depth_filter_close(None)
    assert L.cvo_depth_filter_accumulate_host(-1, None, None, None, 0, None, None, None, None, None) == _capi.CVO_E_INVALID
    assert L.cvo_depth_filter_finish_host(-1, None, None, None, None, 3, None, None, None, None, None) == _capi.CVO_E_INVALID
    assert L.cvo_depth_filter_finish_host(0, None, None, None, None, -1, None, None, None, None, None) == _capi.CVO_E_INVALID


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} for arguments it had to refuse")


def _fake_gpu():
    g = CvoGPU.__new__(CvoGPU)
    g.L, g.ctx, g.params = NoLibrary(), None, cases.load_params("geometric_gpu")
    return g


def _fake_cloud(n=3):
    c = DeviceCloud.__new__(DeviceCloud)
    c.gpu, c.n, c._keep, c.handle = None, n, None, None
    return c


def _fake_filter():
    f = DepthFilter.__new__(DepthFilter)
    f.gpu, f.n, f.handle = _fake_gpu(), 3, 1
    return f


def test_wrappers_refuse_before_the_library():
    g = _fake_gpu()
    with pytest.raises(ValueError, match="DeviceCloud"):
        g.depth_filter_open(np.zeros((3, 3)))
    with pytest.raises(ValueError, match="DeviceCloud"):
        g.depth_filter(np.zeros((3, 3)), [], [], [], np.eye(3))
    with pytest.raises(ValueError, match="every frame"):
        g.depth_filter(_fake_cloud(), [np.zeros((3, 3))], [np.eye(4)], [np.eye(4)], np.eye(3))
    with pytest.raises(ValueError, match="one 4x4 matrix per frame"):
        g.depth_filter(_fake_cloud(), [_fake_cloud()], [np.eye(4), np.eye(4)], [np.eye(4)], np.eye(3))
    with pytest.raises(ValueError, match="one 4x4 matrix per frame"):
        g.depth_filter(_fake_cloud(), [_fake_cloud()], [np.eye(4)], [np.eye(3)], np.eye(3))
    with pytest.raises(ValueError, match="3x3"):
        g.depth_filter(_fake_cloud(), [_fake_cloud()], [np.eye(4)], [np.eye(4)], np.eye(4))
    with pytest.raises(ValueError, match="min_count"):
        g.depth_filter(_fake_cloud(), [_fake_cloud()], [np.eye(4)], [np.eye(4)], np.eye(3), min_count=-1)
    f = _fake_filter()
    with pytest.raises(ValueError, match="DeviceCloud"):
        f.add(np.zeros((3, 3)), np.eye(4), np.eye(3), np.eye(4))
    with pytest.raises(ValueError, match="T_depth"):
        f.add(_fake_cloud(), np.eye(4), np.eye(3), np.eye(3))
    with pytest.raises(ValueError, match="T: a 4x4"):
        f.add(_fake_cloud(), np.zeros(12), np.eye(3), np.eye(4))
    with pytest.raises(ValueError, match="3x3"):
        f.add(_fake_cloud(), np.eye(4), np.eye(4), np.eye(4))
    with pytest.raises(ValueError, match="min_count"):
        f.finish(min_count=2.5)
    f.handle = None
    for call in (lambda: f.state(), lambda: f.finish(), lambda: f.add(_fake_cloud(), np.eye(4), np.eye(3), np.eye(4))):
        with pytest.raises(ValueError, match="closed"):
            call()
    f.close()   # (closing twice is harmless)


def test_host_twin_wrappers_refuse_wrong_shapes():
    rp, col, val = np.array([0, 1, 2]), np.array([0, 1]), np.array([0.5, 0.25], np.float32)
    y = np.ones((2, 3), np.float32)
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        depth_filter_accumulate_host(rp, col, val, np.ones(6), np.eye(4))
    with pytest.raises(ValueError, match="T_depth"):
        depth_filter_accumulate_host(rp, col, val, y, np.eye(3))
    with pytest.raises(ValueError, match="row_ptr\\[-1\\] entries"):
        depth_filter_accumulate_host(rp, col[:1], val[:1], y, np.eye(4))
    with pytest.raises(ValueError, match="state"):
        depth_filter_accumulate_host(rp, col, val, y, np.eye(4), (np.zeros(2), np.zeros(2, np.float32), np.zeros(2, np.int32)))
    with pytest.raises(CvoError):   # a column outside the frame: the library's own refusal
        depth_filter_accumulate_host(rp, np.array([0, 2]), val, y, np.eye(4))
    state = depth_filter_accumulate_host(rp, col, val, y, np.eye(4))
    assert state[2].tolist() == [1, 1] and state[0].tolist() == [0.5, 0.25]
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        depth_filter_finish_host(np.ones(6), state)
    with pytest.raises(ValueError, match="three arrays of n"):
        depth_filter_finish_host(np.ones((3, 3)), state)
    with pytest.raises(ValueError, match="min_count"):
        depth_filter_finish_host(np.ones((2, 3)), state, min_count=-3)
    xyz, kept, depth, nf = depth_filter_finish_host(np.ones((2, 3)), state, min_count=0)
    assert kept.tolist() == [0, 1] and nf == 0 and np.allclose(depth, 1.0)
