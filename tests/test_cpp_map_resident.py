"""Resident clouds into and out of the semantic voxel map through the C++ side: host/cvo_map_resident_check builds
semantic_bki::SemanticBKIOctoMap on a context, inserts every frame from where it is on the device
(insert_pointcloud_csm(const ResidentClouds&, k, pose12, ...)) and reads the map out as a resident cloud (resident_cloud()) -
under -m gpu against the tables and rows the Python route gives for the same frames.  Without a GPU: the driver is built,
refuses what it cannot read before it opens a device, and the mapping header compiles on its own with the new statements."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bki_cases as bc
import cases

CHECK = os.path.join(cases.ROOT, "host", "cvo_map_resident_check")
YAML = os.path.join(cases.CONFIGS, "geometric_gpu.yaml")


def _fnv(parts):
    h = 14695981039346656037
    for a in parts:
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _pose(f):
    a = 0.1 * f
    return np.array([[np.cos(a), -np.sin(a), 0, 0.1 * f], [np.sin(a), np.cos(a), 0, 0.2], [0, 0, 1, 0.3]], np.float32)


def _case_file(path, name="three_inserts"):
    """the case's frames, each under a pose of its own -> the driver's arguments behind its name"""
    cfg, frames = bc.all_cases()[name]
    C = cfg.num_classes
    rows = []
    for f, (xyz, feat, label, _) in enumerate(frames):
        n = xyz.shape[0]
        lab = label if C else np.zeros((n, 0), np.float32)
        rows.append(np.concatenate([np.full((n, 1), f, np.float32), np.tile(_pose(f).reshape(1, 12), (n, 1)), xyz, feat, lab], axis=1))
    np.save(path, np.concatenate(rows).astype(np.float32))
    return [str(path), str(C)] + [repr(float(v)) for v in (cfg.resolution, cfg.prior, cfg.free_thresh, cfg.occupied_thresh, cfg.free_resolution, cfg.max_range)]


def test_driver_is_built_and_states_its_arguments():
    assert os.path.exists(CHECK), "build the host tools first (make -C host)"
    res = subprocess.run([CHECK], capture_output=True, text=True)
    assert res.returncode == 2 and "usage:" in res.stderr and "params.yaml" in res.stderr


def test_driver_refuses_a_case_it_cannot_read(tmp_path):
    args = _case_file(tmp_path / "case.npy")
    # a missing file, and a class count the rows do not have: refused before any device is opened
    for bad in ([str(tmp_path / "none.npy")] + args[1:], [args[0], "3"] + args[2:]):
        res = subprocess.run([CHECK] + bad + [YAML], capture_output=True, text=True)
        assert res.returncode == 1 and "cvo_map_resident_check:" in res.stderr, bad


def test_mapping_header_compiles_with_the_resident_statements(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    inc = [os.path.join(cases.ROOT, "include"), os.path.join(cases.ROOT, "include", "UnifiedCvo")]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-c"] + [f"-I{p}" for p in inc] +
                          ["-o", str(tmp_path / "map_resident_headers_check.o"), os.path.join(cases.ROOT, "tests", "cpp", "map_resident_headers_check.cpp")])


@pytest.mark.gpu
def test_veneer_equals_the_python_route(tmp_path):
    import unified_cvo_amd as u
    from unified_cvo_amd import CvoGPU, CvoPointCloud
    args = _case_file(tmp_path / "case.npy")
    out = subprocess.check_output([CHECK] + args + [YAML], text=True, timeout=300, env=dict(os.environ, CVO_BKI_HOST="0")).splitlines()
    cfg, frames = bc.all_cases()["three_inserts"]
    gpu = CvoGPU(params=cases.load_params("geometric_gpu"))
    gpu.set_option("BKI_HOST", 0)
    m = gpu.map_open(u.MapConfig(**cfg.kwargs()))
    for f, (xyz, feat, label, _) in enumerate(frames):
        cloud = gpu.upload(CvoPointCloud.from_arrays(xyz, feat, label))
        m.insert_cloud(cloud, pose=_pose(f))
        cloud.free()
    d = m.resident_cloud().download()
    s = m.debug_stats(readback=True)
    rows = [np.concatenate([d.positions_[i], d.features_[i], d.labels_[i]]).astype(np.float32) for i in range(d.num_points())]
    table = []
    for v in range(len(s["keys"])):
        table += [s["keys"][v:v + 1], s["ms"][v], s["fs"][v]]
    assert d.num_points() > 20 and len(s["keys"]) > 300
    assert out == [f"cloud {d.num_points()}", "rows " + _fnv(rows), f"table {len(s['keys'])} " + _fnv(table), "on_device 1"]
    m.close()
    gpu.close()
