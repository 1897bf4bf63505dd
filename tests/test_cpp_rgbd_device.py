"""Device RGB-D frames through the C++ veneer: tests/cpp/rgbd_device_headers_check.cpp compiles against cvo/CvoGPU.hpp with a
host compiler; host/cvo_rgbd_device_check runs the CPU twin of the rows on its own (no GPU) and, under -m gpu,
CvoGPU::upload_rgbd_points_device / upload_rgbd_device on planes it copies to the device - both against the Python results."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import np_rgbd_device as nd
import rgbd_cases as rc
from unified_cvo_amd import rgbd_points_host
from unified_cvo_amd.api import DSO_EDGES, FULL

CHECK = os.path.join(cases.ROOT, "host", "cvo_rgbd_device_check")


def test_veneer_header_compiles_with_the_device_frame_statements(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    inc = [os.path.join(cases.ROOT, "include"), os.path.join(cases.ROOT, "include", "UnifiedCvo")]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-c"] + [f"-I{p}" for p in inc] +
                          ["-o", str(tmp_path / "rgbd_device_headers_check.o"), os.path.join(cases.ROOT, "tests", "cpp", "rgbd_device_headers_check.cpp")])


def _fnv(xyz, feat, label, geo):
    """FNV-1a over xyz, 5 features, the 19 class scores (when the cloud holds them) and the geometric type, point by point."""
    cols = [np.asarray(xyz, np.float32), nd.pad(feat, nd.FEATURES)] + ([] if label is None else [nd.pad(label, nd.CLASSES)]) + [np.asarray(geo, np.float32).reshape(-1, 2)]
    h = 14695981039346656037
    for b in np.concatenate(cols, axis=1).astype(np.float32).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _write(tmp_path, f):
    (tmp_path / "calib.txt").write_text(f"{f.fx!r} {f.fy!r} {f.cx!r} {f.cy!r} {f.scaling_factor!r}\n")
    np.save(tmp_path / "image.npy", f.image)
    np.save(tmp_path / "depth.npy", f.depth)
    args = [str(tmp_path / "image.npy"), str(tmp_path / "depth.npy"), str(tmp_path / "calib.txt")]
    if f.semantic is None:
        return args, []
    np.save(tmp_path / "scores.npy", f.semantic)
    return args, ["--semantic", str(tmp_path / "scores.npy")]


def _run(args):
    assert os.path.exists(CHECK), "build the host tools first (make -C host)"
    out = subprocess.check_output([CHECK] + args, text=True, timeout=300).splitlines()
    n = int(out[0].split()[1])
    pixel = np.array(out[1].split(), np.int32)
    assert len(pixel) == n
    return n, pixel, out[2]


@pytest.mark.parametrize("name,depth", [("tiny", "u16"), ("small", "f32"), ("semantic", "u16")])
def test_twin_through_the_driver_matches_python(tmp_path, name, depth):
    f = rc.frame(name, depth)
    args, sem = _write(tmp_path, f)
    for method, text in ((DSO_EDGES, "DSO_EDGES"), (FULL, "FULL")):
        want = rgbd_points_host(f, method)
        n, pixel, rows = _run(args + [text] + sem)
        assert np.array_equal(pixel, want.pixel), (name, text)
        assert rows == "rows " + _fnv(want.positions(), want.features(), None if f.semantic is None else want.labels(), want.geometric_types_), (name, text)


def test_driver_refuses_what_the_library_refuses(tmp_path):
    args, _ = _write(tmp_path, rc.frame("tiny"))
    r = subprocess.run([CHECK] + args + ["CANNY_EDGES"], capture_output=True, text=True)
    assert r.returncode == 1 and "cvo_rgbd_device_check:" in r.stderr


@pytest.mark.gpu
def test_veneer_matches_python(tmp_path):
    from unified_cvo_amd import CvoGPU
    yaml = os.path.join(cases.CONFIGS, "geometric_gpu.yaml")
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    try:
        g.set_option("RGBD_HOST", 0)
        for name, depth in (("small", "f32"), ("semantic", "u16")):
            f = rc.frame(name, depth)
            d = tmp_path / f"{name}-{depth}"
            d.mkdir()
            args, sem = _write(d, f)
            for method, text in ((DSO_EDGES, "DSO_EDGES"), (FULL, "FULL")):
                want = g.rgbd_points(f, method)
                n, pixel, rows = _run(args + [text, "--device", yaml] + sem)
                assert np.array_equal(pixel, want.pixel), (name, text)
                assert rows == "rows " + _fnv(want.positions(), want.features(), None if f.semantic is None else want.labels(), want.geometric_types_), (name, text)
            want = g.upload_rgbd(f, 0.25, 5)
            n, pixel, rows = _run(args + ["RECIPE", "--device", yaml, "--leaf", "0.25", "--divisor", "5"] + sem)
            got = want.download()
            assert n == want.n and np.array_equal(pixel, want.pixel)
            assert rows == "rows " + _fnv(got.positions_, got.features_, None, got.geometric_types_), name
            want.free()
    finally:
        g.close()
