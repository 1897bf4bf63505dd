"""The LiDAR front end through the C++ veneer: host/cvo_lidar_check (CvoPointCloud's LiDAR constructors on the host;
CvoGPU::upload_lidar under -m gpu) against the Python results, and the PCL-typed overloads of pcl_interop.hpp through a
host compiler next to tests/mock_include."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cases
import lidar_cases as lc
from unified_cvo_amd import LidarConfig, LidarRand, LidarScan, lidar_select_host

CHECK = os.path.join(cases.ROOT, "host", "cvo_lidar_check")
INC = [os.path.join(cases.ROOT, "tests", "mock_include"), os.path.join(cases.ROOT, "include"), os.path.join(cases.ROOT, "include", "UnifiedCvo")]
CXX = shutil.which("g++") or shutil.which("c++")


def _fnv(xyzi, index):
    """FNV-1a over xyz, the intensity and the type (1, 0) of every point, as cvo_lidar_check prints it."""
    rows = np.concatenate([xyzi[index], np.tile(np.array([1, 0], np.float32), (len(index), 1))], axis=1).astype(np.float32)
    h = 14695981039346656037
    for b in rows.tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _run(args):
    assert os.path.exists(CHECK), "build the host tools first (make -C host)"
    out = subprocess.check_output([CHECK] + args, text=True, timeout=300).splitlines()
    frames = []
    while out:
        n, index = int(out[0].split()[1]), np.array(out[1].split(), np.int32)
        assert len(index) == n
        rest = out[2] if len(out) > 2 and out[2].startswith("rows") else None
        frames.append((index, rest))
        out = out[3 if rest else 2:]
    return frames


def test_lidar_constructors_match_python(tmp_path):
    """Two chained frames of the HDL-64 scan, then the labelled small scan."""
    scan, _ = lc.case("hdl64")
    np.save(tmp_path / "scan.npy", scan.xyzi)
    rand, cfg = LidarRand(12345), LidarConfig()
    frames = _run([str(tmp_path / "scan.npy"), "--seed", "12345", "--frames", "2"])
    assert len(frames) == 2
    for index, rows in frames:
        want, _ = lidar_select_host(scan, cfg, rand)
        assert len(want) > 5000 and np.array_equal(index, want) and rows == "rows " + _fnv(scan.xyzi, want)
    assert not np.array_equal(frames[0][0], frames[1][0])  # the stream went on
    sem, _ = lc.case("semantic")
    np.save(tmp_path / "sem.npy", sem.xyzi)
    np.save(tmp_path / "labels.npy", sem.semantic)
    cfg = LidarConfig(semantic=True, beam_num=16)
    want, _ = lidar_select_host(sem, cfg, LidarRand(1))
    (index, rows), = _run([str(tmp_path / "sem.npy"), "--semantic", str(tmp_path / "labels.npy"), str(sem.num_classes), "--beams", "16", "--seed", "1"])
    assert len(want) > 100 and np.array_equal(index, want) and rows == "rows " + _fnv(sem.xyzi, want)


def test_driver_refuses_what_the_library_refuses(tmp_path):
    scan, _ = lc.case("cap")
    bad = scan.xyzi.copy()
    bad[7, 1] = np.nan
    np.save(tmp_path / "nan.npy", bad)
    np.save(tmp_path / "short.npy", scan.xyzi[:, :3].copy())
    for args in ([str(tmp_path / "nan.npy")], [str(tmp_path / "short.npy")], [str(tmp_path / "nan.npy"), "--what"]):
        r = subprocess.run([CHECK] + args, capture_output=True, text=True)
        assert r.returncode == 1 and "cvo_lidar_check:" in r.stderr


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_pcl_typed_overloads(tmp_path):
    lib = os.path.join(cases.ROOT, "host")
    assert os.path.exists(os.path.join(lib, "libcvo_gpu_img_lib.so")), "build the host tools first (make -C host)"
    exe = tmp_path / "lidar_pcl_check"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + [f"-I{p}" for p in INC] +
                          ["-o", str(exe), os.path.join(cases.ROOT, "tests", "cpp", "lidar_pcl_check.cpp"), f"-L{lib}", "-lcvo_gpu_img_lib", f"-Wl,-rpath,{lib}"])
    scan, _ = lc.case("hdl64")
    with open(tmp_path / "scan.txt", "w") as f:
        f.write(f"{scan.n}\n")
        for row in scan.xyzi:
            f.write(" ".join(repr(float(v)) for v in row) + "\n")
    out = subprocess.check_output([str(exe), str(tmp_path / "scan.txt")], text=True).splitlines()
    want, _ = lidar_select_host(scan, LidarConfig(), LidarRand(1))
    labelled, _ = lidar_select_host(LidarScan(scan.xyzi, np.full(scan.n, 2, np.int32), 4), LidarConfig(semantic=True), LidarRand(1))
    assert out[0] == f"n {len(want)} F 1 last {float(scan.xyzi[want[-1], 3]):.9g}"
    assert out[1] == f"n {len(labelled)} C 4"


@pytest.mark.gpu
def test_device_route_matches_python(tmp_path):
    from unified_cvo_amd import CvoGPU
    yaml = os.path.join(cases.CONFIGS, "geometric_gpu.yaml")
    g = CvoGPU(params=cases.load_params("geometric_gpu"))
    try:
        scan, cfg = lc.case("hdl64")
        np.save(tmp_path / "scan.npy", scan.xyzi)
        want = g.upload_lidar(scan, cfg, LidarRand(9))
        assert g.debug_lidar_stats()["on_device"]
        (index, _), = _run([str(tmp_path / "scan.npy"), "--seed", "9", "--device", yaml])
        assert len(index) == want.n and np.array_equal(index, want.pixel)
        want.free()
    finally:
        g.close()
