"""The surface of "merge posed resident clouds on the device and read clouds back" without a GPU: both entry points are
declared in the boundary header, bound and exported by the library; no test hook is in the boundary header; the Python
wrapper checks the pose count before it touches the library."""
import os
import re
import subprocess

import pytest

import cases
from unified_cvo_amd import CvoGPU, _capi

NEW = ("cvo_cloud_merge", "cvo_cloud_download")


def _header(name):
    return open(os.path.join(cases.ROOT, "include", name)).read()


def test_entry_points_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _header("cvo_hip.h"), flags=re.S)
    for sym in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), sym
        assert sym in _capi.EXPORTED, sym
    for bit in ("CVO_CLOUD_HAS_FEAT 1", "CVO_CLOUD_HAS_LABEL 2", "CVO_CLOUD_HAS_GEOTYPE 4"):
        assert bit in text, bit


def test_library_exports_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    for sym in NEW:
        assert sym in exported, sym


def test_bindings_have_argument_types():
    L = _capi.lib()
    assert len(L.cvo_cloud_merge.argtypes) == 8 and len(L.cvo_cloud_download.argtypes) == 7


def test_no_debug_hook_in_the_boundary_header():
    text = re.sub(r"/\*.*?\*/", "", _header("cvo_hip.h"), flags=re.S)  # (comments may name a hook; declarations may not)
    assert "cvo_debug_" not in text


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} for arguments it had to refuse")


class FakeCloud:
    n, handle = 3, None


def test_wrapper_refuses_a_wrong_pose_count():
    g = CvoGPU.__new__(CvoGPU)
    g.L, g.ctx, g.device = NoLibrary(), None, 0
    with pytest.raises(ValueError, match="12 entries per cloud"):
        g.merge_clouds([FakeCloud(), FakeCloud()], poses=[0.0] * 12)
