"""The RGB-D front end through the C++ veneer: host/cvo_rgbd_check (CvoPointCloud's image constructor on the host;
CvoGPU::rgbd_points / upload_rgbd under -m gpu) against the Python results, and the new headers through a host compiler
next to tests/mock_include like the interop headers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import rgbd_cases as rc
from unified_cvo_amd import rgbd_points_host
from unified_cvo_amd.api import DSO_EDGES, FULL

CHECK = os.path.join(cases.ROOT, "host", "cvo_rgbd_check")
INC = [os.path.join(cases.ROOT, "tests", "mock_include"), os.path.join(cases.ROOT, "include"), os.path.join(cases.ROOT, "include", "UnifiedCvo")]
CXX = shutil.which("g++") or shutil.which("c++")


def _fnv(pc):
    """FNV-1a over xyz, features and geometric type of every point, as cvo_rgbd_check prints it."""
    rows = np.concatenate([pc.positions(), pc.features(), pc.geometric_types_.reshape(-1, 2)], axis=1).astype(np.float32)
    h = 14695981039346656037
    for b in rows.tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _write(tmp_path, f, raw=False):
    calib = tmp_path / "calib.txt"
    calib.write_text(f"{f.fx!r} {f.fy!r} {f.cx!r} {f.cy!r} {f.scaling_factor!r}\n")
    if raw:
        f.image.tofile(tmp_path / "image.u8")
        f.depth.tofile(tmp_path / "depth.raw")
        shape = f"{f.rows}:{f.cols}"
        return [f"{tmp_path / 'image.u8'}:{shape}" + (":3" if f.channels == 3 else ""),
                f"{tmp_path / 'depth.raw'}:{shape}:" + ("u16" if f.depth.dtype == np.uint16 else "f32"), str(calib)]
    np.save(tmp_path / "image.npy", f.image)
    np.save(tmp_path / "depth.npy", f.depth)
    return [str(tmp_path / "image.npy"), str(tmp_path / "depth.npy"), str(calib)]


def _run(args):
    assert os.path.exists(CHECK), "build the host tools first (make -C host)"
    out = subprocess.check_output([CHECK] + args, text=True, timeout=300).splitlines()
    n = int(out[0].split()[1])
    pixel = np.array(out[1].split(), np.int32)
    assert len(pixel) == n
    return n, pixel, out[2:]


@pytest.mark.parametrize("name,depth,raw", [("small", "u16", False), ("small", "f32", True), ("mono", "u16", True), ("tiny", "f32", False)])
def test_image_constructor_matches_python(tmp_path, name, depth, raw):
    f = rc.frame(name, depth)
    args = _write(tmp_path, f, raw)
    for method, text in ((DSO_EDGES, "DSO_EDGES"), (FULL, "FULL")):
        want = rgbd_points_host(f, method)
        n, pixel, rest = _run(args + [text])
        assert n == want.num_points() and np.array_equal(pixel, want.pixel), (name, text)
        assert rest[0] == "rows " + _fnv(want), (name, text)


def test_caller_gray_plane_through_the_driver(tmp_path):
    f = rc.own_gray(rc.frame("small"))
    args = _write(tmp_path, f)
    np.save(tmp_path / "gray.npy", f.gray)
    want = rgbd_points_host(f, DSO_EDGES)
    n, pixel, rest = _run(args + ["DSO_EDGES", "--gray", str(tmp_path / "gray.npy")])
    assert np.array_equal(pixel, want.pixel) and rest[0] == "rows " + _fnv(want)


def test_driver_refuses_what_the_library_refuses(tmp_path):
    f = rc.frame("tiny")
    args = _write(tmp_path, f)
    for method in ("CANNY_EDGES", "RECIPE"):
        r = subprocess.run([CHECK] + args + [method], capture_output=True, text=True)
        assert r.returncode == 1 and "cvo_rgbd_check:" in r.stderr


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_rgbd_headers_compile_on_their_own(tmp_path):
    exe = tmp_path / "rgbd_headers_check"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + [f"-I{p}" for p in INC] +
                          ["-o", str(exe), os.path.join(cases.ROOT, "tests", "cpp", "rgbd_headers_check.cpp")])
    (tmp_path / "rgbd.txt").write_text("525.0 525.5 319.5 239.5 5000\n640 480\n")
    (tmp_path / "stereo.txt").write_text("707.09 707.09 601.88 183.11 0.54\n")
    out = subprocess.check_output([str(exe), str(tmp_path / "rgbd.txt"), str(tmp_path / "stereo.txt")], text=True).splitlines()
    assert out[0] == "rgbd 525 525.5 319.5 239.5 5000 640 480"
    assert out[1] == "stereo 707.09 707.09 601.88 183.11 0.54 1 0"
    assert out[2] == "headers ok"


@pytest.mark.gpu
def test_device_route_matches_python(tmp_path):
    from unified_cvo_amd import CvoGPU
    yaml = os.path.join(cases.CONFIGS, "geometric_gpu.yaml")
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    try:
        for name, depth in (("textured", "u16"), ("small", "f32")):
            f = rc.frame(name, depth)
            d = tmp_path / f"{name}-{depth}"
            d.mkdir()
            args = _write(d, f)
            for method, text in ((DSO_EDGES, "DSO_EDGES"), (FULL, "FULL")):
                want = g.rgbd_points(f, method)
                n, pixel, rest = _run(args + [text, "--device", yaml])
                assert np.array_equal(pixel, want.pixel) and rest[0] == "rows " + _fnv(want), (name, text)
            for leaf, div in ((0.0, 4), (0.25, 5)):
                want = g.upload_rgbd(f, None if leaf == 0.0 else leaf, div)
                n, pixel, rest = _run(args + ["RECIPE", "--device", yaml, "--leaf", str(leaf), "--divisor", str(div)])
                assert n == want.n and np.array_equal(pixel, want.pixel)
                assert np.array_equal(np.array(rest[0].split(), np.int32).astype(bool), want.is_edge)
                want.free()
    finally:
        g.close()
