"""The surface of "query the semantic map: points, rays, a rendered view" without a GPU: the seven entry points are declared in
the boundary header, bound and exported by the library; no test hook is in the boundary header; the kernels are part of the
kernel set; the Python wrapper refuses wrong shapes, unknown stops and host-map / resident-cloud mixes before it touches the
library."""
import os
import re
import subprocess

import numpy as np
import pytest

import cases
from unified_cvo_amd import DeviceCloud, MapConfig, SemanticMap, _capi

NEW = ("cvo_map_query", "cvo_map_query_cloud", "cvo_map_query_host", "cvo_map_raycast", "cvo_map_raycast_host", "cvo_map_render",
       "cvo_map_render_host")


def _read(*path):
    return open(os.path.join(cases.ROOT, *path)).read()


def test_entry_points_are_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", _read("include", "cvo_hip.h"), flags=re.S)
    for sym in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), sym
        assert sym in _capi.EXPORTED, sym
    for struct in ("cvo_map_query_out_t", "cvo_map_ray_out_t", "cvo_map_render_out_t"):
        assert re.search(r"\}\s*%s;" % struct, text), struct


def test_library_exports_them():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    for sym in NEW:
        assert sym in exported, sym


def test_bindings_have_argument_types():
    L = _capi.lib()
    want = dict(cvo_map_query=4, cvo_map_query_cloud=4, cvo_map_query_host=4, cvo_map_raycast=7, cvo_map_raycast_host=7, cvo_map_render=11,
                cvo_map_render_host=11)
    for sym, n in want.items():
        assert len(getattr(L, sym).argtypes) == n, sym
    assert [f for f, _ in _capi.cvo_map_query_out_t._fields_] == ["found", "state", "semantics", "probs", "vars", "feat", "centre"]
    assert [f for f, _ in _capi.cvo_map_ray_out_t._fields_] == ["status", "key", "centre", "t", "steps", "state", "semantics"]
    assert [f for f, _ in _capi.cvo_map_render_out_t._fields_] == ["depth", "semantics", "feat", "label"]


def test_struct_fields_follow_the_header():
    text = _read("include", "cvo_hip.h")
    for struct, cls in (("cvo_map_query_out_t", _capi.cvo_map_query_out_t), ("cvo_map_ray_out_t", _capi.cvo_map_ray_out_t),
                        ("cvo_map_render_out_t", _capi.cvo_map_render_out_t)):
        body = re.search(r"typedef struct %s \{(.*?)\}" % struct, text, flags=re.S).group(1)
        assert re.findall(r"\*\s*(\w+);", body) == [f for f, _ in cls._fields_], struct


def test_no_debug_hook_in_the_boundary_header():
    text = re.sub(r"/\*.*?\*/", "", _read("include", "cvo_hip.h"), flags=re.S)  # (comments may name a hook; declarations may not)
    assert "cvo_debug_" not in text


def test_kernels_are_part_of_the_kernel_set():
    assert '#include "cvo_k_bki_query.h"' in _read("unified_cvo_amd", "csrc", "cvo_kernels.h")
    text = _read("unified_cvo_amd", "csrc", "cvo_k_bki_query.h")
    for k in ("k_bki_query", "k_bki_raycast", "k_bki_render"):
        assert re.search(r"__global__ __launch_bounds__\(\w+\) void %s\(" % k, text), k
    assert "table_find" in _read("unified_cvo_amd", "csrc", "cvo_k_prims.h")


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} for arguments it had to refuse")


class FakeGPU:
    L, ctx = NoLibrary(), None


def fake_cloud():
    c = DeviceCloud.__new__(DeviceCloud)
    c.gpu, c.n, c._keep, c.handle = None, 3, None, None
    return c


def _map(gpu):
    m = SemanticMap.__new__(SemanticMap)
    m.gpu, m.config, m.L, m.handle = gpu, MapConfig(num_classes=3), NoLibrary(), None
    return m


@pytest.mark.parametrize("shape", [(3,), (4, 2), (2, 3, 3), (5, 4)])
def test_query_refuses_points_of_the_wrong_shape(shape):
    for gpu in (FakeGPU(), None):
        with pytest.raises(ValueError, match=r"\(n, 3\)"):
            _map(gpu).query(np.zeros(shape))


def test_query_refuses_the_mixes():
    with pytest.raises(ValueError, match="host map"):
        _map(None).query(fake_cloud())
    with pytest.raises(ValueError, match="host map"):
        _map(None).query(fake_cloud(), pose=np.eye(4))
    with pytest.raises(ValueError, match="map frame"):
        _map(FakeGPU()).query(np.zeros((4, 3)), pose=np.eye(4))
    for shape in ((12,), (3, 3), (4, 3)):
        with pytest.raises(ValueError, match="3x4 or 4x4"):
            _map(FakeGPU()).query(fake_cloud(), pose=np.zeros(shape))


def test_raycast_refusals():
    for gpu in (FakeGPU(), None):
        m = _map(gpu)
        with pytest.raises(ValueError, match=r"\(n, 3\)"):
            m.raycast(np.zeros(3), np.zeros(3))
        with pytest.raises(ValueError, match="differ in shape"):
            m.raycast(np.zeros((2, 3)), np.zeros((4, 3)))
        with pytest.raises(ValueError, match="a stop is one of"):
            m.raycast(np.zeros((4, 3)), np.zeros((4, 3)), stop=("occupied", "solid"))
        with pytest.raises(ValueError, match="0 .. 15"):
            m.raycast(np.zeros((4, 3)), np.zeros((4, 3)), stop=16)
        for steps in (0, -5, (1 << 20) + 1):
            with pytest.raises(ValueError, match="max_steps"):
                m.raycast(np.zeros((4, 3)), np.zeros((4, 3)), max_steps=steps)


def test_stop_masks():
    assert SemanticMap.stop_mask(("occupied",)) == 2 and SemanticMap.stop_mask("unknown") == 4 and SemanticMap.stop_mask(()) == 0
    assert SemanticMap.stop_mask(("free", "occupied", "unknown", "absent")) == 15 and SemanticMap.stop_mask(10) == 10 and SemanticMap.stop_mask(0) == 0


def test_render_refusals():
    kw = dict(fx=8.0, fy=8.0, cx=3.5, cy=3.5, rows=8, cols=8, z_far=3.0)
    for gpu in (FakeGPU(), None):
        m = _map(gpu)
        for shape in ((12,), (3, 3), (4, 3)):
            with pytest.raises(ValueError, match="3x4 or 4x4"):
                m.render(np.zeros(shape), **kw)
        with pytest.raises(ValueError, match="at least 1"):
            m.render(np.eye(4), **dict(kw, rows=0))
        with pytest.raises(ValueError, match="2\\^24 pixels"):
            m.render(np.eye(4), **dict(kw, rows=4097, cols=4096))
        with pytest.raises(ValueError, match="a plane is one of"):
            m.render(np.eye(4), planes=("depth", "colour"), **kw)
        with pytest.raises(ValueError, match="a stop is one of"):
            m.render(np.eye(4), stop=("wall",), **kw)
