"""The surface of "insert resident clouds into the semantic map, read it out on the device" without a GPU: both entry points
are declared in the boundary header, bound and exported by the library; no test hook is in the boundary header; the Python
wrapper refuses a call without pose and origin, a pose of the wrong shape and a host map before it touches the library."""
import os
import re
import subprocess

import numpy as np
import pytest

import cases
from unified_cvo_amd import MapConfig, SemanticMap, _capi

NEW = ("cvo_map_insert_cloud", "cvo_map_cloud_resident")


def _header(name):
    return open(os.path.join(cases.ROOT, "include", name)).read()


def test_entry_points_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _header("cvo_hip.h"), flags=re.S)
    for sym in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), sym
        assert sym in _capi.EXPORTED, sym


def test_library_exports_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    for sym in NEW:
        assert sym in exported, sym


def test_bindings_have_argument_types():
    L = _capi.lib()
    assert len(L.cvo_map_insert_cloud.argtypes) == 4 and len(L.cvo_map_cloud_resident.argtypes) == 3


def test_no_debug_hook_in_the_boundary_header():
    text = re.sub(r"/\*.*?\*/", "", _header("cvo_hip.h"), flags=re.S)  # (comments may name a hook; declarations may not)
    assert "cvo_debug_" not in text


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} for arguments it had to refuse")


class FakeCloud:
    n, handle = 3, None


class FakeGPU:
    L, ctx = NoLibrary(), None


def _map(gpu):
    m = SemanticMap.__new__(SemanticMap)
    m.gpu, m.config, m.L, m.handle = gpu, MapConfig(), NoLibrary(), None
    return m


def test_wrapper_refuses_a_call_without_pose_and_origin():
    with pytest.raises(ValueError, match="the origin or the pose"):
        _map(FakeGPU()).insert_cloud(FakeCloud())


@pytest.mark.parametrize("shape", [(12,), (3, 3), (4, 3), (2, 3, 4)])
def test_wrapper_refuses_a_pose_of_the_wrong_shape(shape):
    with pytest.raises(ValueError, match="3x4 or 4x4"):
        _map(FakeGPU()).insert_cloud(FakeCloud(), pose=np.zeros(shape))


def test_wrapper_refuses_a_host_map():
    m = _map(None)
    with pytest.raises(ValueError, match="host map"):
        m.insert_cloud(FakeCloud(), pose=np.eye(4))
    with pytest.raises(ValueError, match="host map"):
        m.insert_cloud(FakeCloud(), origin=[0, 0, 0])
    with pytest.raises(ValueError, match="host map"):
        m.resident_cloud()
