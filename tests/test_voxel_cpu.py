"""Voxel-grid downsampling without a GPU: cvo_voxel_select_host (the CPU twin of the kernels, part of the library) against
the numpy statement in np_voxel.py, bit for bit; its refusals; the VoxelMap drop-in header through host/cvo_voxel_check."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_voxel
from unified_cvo_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345


def select_host(xyz, s, n=None):
    """(rc, kept buffer, n_kept): the buffers start as SENTINEL so that a refusal can be seen to write nothing."""
    L = _capi.lib()
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0] if n is None else n
    kept = np.full(max(xyz.shape[0], 1), SENTINEL, np.int32)
    nk = C.c_int(SENTINEL)
    rc = L.cvo_voxel_select_host(n, xyz.ctypes.data_as(C.POINTER(C.c_float)), C.c_float(s),
                                 kept.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nk))
    return rc, kept, nk.value


CASES = np_voxel.cpu_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_twin_equals_numpy(case):
    _, xyz, s = case
    want = np_voxel.reference(xyz, s)
    rc, kept, nk = select_host(xyz, s)
    assert rc == _capi.CVO_OK
    assert nk == want.shape[0]
    assert np.array_equal(kept[:nk], want)
    assert np.all(kept[nk:] == SENTINEL)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_packed_reference_equals_the_row_wise_one(case):
    """np_voxel.reference_packed (one np.unique over 63-bit keys: what the 2^24-point test can afford) against reference."""
    _, xyz, s = case
    assert np.array_equal(np_voxel.reference_packed(xyz, s), np_voxel.reference(xyz, s))


def test_reference_rounds_ties_to_even_and_divides():
    assert np_voxel.voxel_keys([[0.375, 0.625, -0.375]], 0.25).tolist() == [[2, 2, -2]]
    rc, kept, nk = select_host([[0.375, 0.625, -0.375], [0.5, 0.5, -0.5], [0.25, 0.75, -0.25]], 0.25)
    assert (rc, nk, kept[:nk].tolist()) == (0, 2, [0, 2])  # 1.5 and 2.5 meet in voxel 2; 1 and 3 do not
    x = np_voxel.division_cloud(0.1)
    a = np.rint(x / np.float32(0.1))
    b = np.rint(x * (np.float32(1.0) / np.float32(0.1)))
    assert np.any(a != b)  # (the cloud tells a division from a multiply by the reciprocal)


def test_known_counts():
    copies = {c[0]: c for c in CASES}["copies"]
    rc, kept, nk = select_host(copies[1], copies[2])
    assert (rc, nk, kept[0]) == (0, 1, 0)
    own = np_voxel.own_voxel_cloud()
    rc, kept, nk = select_host(own, 0.5)
    assert nk == own.shape[0] and np.array_equal(kept, np.arange(own.shape[0]))


def _refused(xyz, s, code=_capi.CVO_E_INVALID, n=None):
    rc, kept, nk = select_host(xyz, s, n)
    assert rc == code
    assert nk == SENTINEL and np.all(kept == SENTINEL)


@pytest.mark.parametrize("s", [0.0, -0.1, float("nan"), float("inf"), -float("inf")])
def test_refuses_bad_voxel_size(s):
    _refused(np_voxel.scene(100), s)


@pytest.mark.parametrize("where", [0, 500, 999])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
def test_refuses_non_finite_coordinate(where, value):
    x = np_voxel.scene(1000).copy()
    x[where, where % 3] = value
    _refused(x, 0.25)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_refuses_voxel_index_beyond_2_to_20(axis):
    x = np_voxel.scene(1000).copy()
    x[321, axis] = -(2.0 ** 20) * 0.25
    _refused(x, 0.25)
    x[321, axis] = (2.0 ** 20 - 0.5) * 0.25  # the tie rounds to the even 2^20
    _refused(x, 0.25)
    x[321, axis] = (2.0 ** 20 - 1) * 0.25  # the largest voxel index there is
    rc, kept, nk = select_host(x, 0.25)
    assert rc == 0 and np.array_equal(kept[:nk], np_voxel.reference(x, 0.25))
    x[321, axis] = 3.0e38  # the quotient overflows
    _refused(x, 0.25)


def test_refuses_more_than_2_to_24_points():
    x = np.zeros((2 ** 24 + 1, 3), np.float32)
    _refused(x[:1], 0.25, _capi.CVO_E_UNSUPPORTED, n=2 ** 24 + 1)  # (refused on its size: the rows are never read)
    _refused(np_voxel.scene(10), 0.25, n=-1)


def test_voxelmap_header_through_cvo_voxel_check(tmp_path):
    exe = os.path.join(ROOT, "host", "cvo_voxel_check")
    assert os.path.exists(exe), "host/cvo_voxel_check is missing: run `make -C host`"
    for name, xyz, s in (("scene", np_voxel.scene(10000), 0.25), ("duplicates", np_voxel.duplicates_cloud(), 0.1),
                         ("half", np_voxel.half_boundary_cloud(0.25), 0.25)):
        src = tmp_path / f"{name}.f32"
        np.ascontiguousarray(xyz, np.float32).tofile(src)
        out = subprocess.run([exe, str(src), repr(float(s))], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.strip().splitlines()
        want = np_voxel.reference(xyz, s)
        head = dict(kv.split("=") for kv in lines[0].split())
        assert int(head["points"]) == xyz.shape[0] and int(head["voxels"]) == want.shape[0]
        assert np.array_equal(np.array(lines[1].split(), np.int64), want)  # sample_points(): first members, insertion order
        # query_point finds every point's voxel, its first member is the kept one; a second insert of a pointer is refused;
        # deleting a voxel's last member removes the voxel
        assert lines[2] == "queries ok" and lines[3] == "double insert refused" and lines[4] == "delete ok", lines[2:]
