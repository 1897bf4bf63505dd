"""The semantic voxel map through the C++ side: host/cvo_bki_check builds semantic_bki::SemanticBKIOctoMap and
cvo::CvoPointCloud(&map, num_class) with the statements of upstream's driver (mapping/bkioctomap.h) - the CPU twin, and the
device under -m gpu - against the numpy statement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bki_cases as bc
import cases

CHECK = os.path.join(cases.ROOT, "host", "cvo_bki_check")
NAMES = ("three_inserts", "hits257")


def _fnv(parts):
    h = 14695981039346656037
    for a in parts:
        for b in np.ascontiguousarray(a, np.float32).tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _case_file(path, name):
    cfg, frames = bc.all_cases()[name]
    C = cfg.num_classes
    rows = []
    for f, (xyz, feat, label, origin) in enumerate(frames):
        n = xyz.shape[0]
        lab = label if C else np.zeros((n, 0), np.float32)
        rows.append(np.concatenate([np.full((n, 1), f, np.float32), np.tile(origin, (n, 1)), xyz, feat, lab], axis=1))
    np.save(path, np.concatenate(rows).astype(np.float32))
    return [path, C] + [repr(float(v)) for v in (cfg.resolution, cfg.prior, cfg.free_thresh, cfg.occupied_thresh, cfg.free_resolution, cfg.max_range)]


def _check(tmp_path, extra=(), env=None, on_device=0):
    assert os.path.exists(CHECK), "build the host tools first (make -C host)"
    for name in NAMES:
        args = _case_file(tmp_path / "case.npy", name)
        out = subprocess.check_output([CHECK] + [str(a) for a in args] + list(extra), text=True, timeout=300, env=env).splitlines()
        xyz, feat, label = bc.statement_of(name)[-1][1]
        rows = [np.concatenate([xyz[i], feat[i], label[i]]) for i in range(len(xyz))]
        assert len(xyz) > 20 and out == [f"cloud {len(xyz)}", "rows " + _fnv(rows), f"on_device {on_device}"], name


def test_twin_through_the_drivers_statements(tmp_path):
    _check(tmp_path)


def test_driver_refuses_what_the_library_refuses(tmp_path):
    args = [str(a) for a in _case_file(tmp_path / "case.npy", "hits257")]
    for bad in (args[:2] + ["-0.5"] + args[3:], args[:6] + ["0"] + args[7:], args + ["--what"]):
        res = subprocess.run([CHECK] + bad, capture_output=True, text=True)
        assert res.returncode == 1 and "cvo_bki_check:" in res.stderr, bad


def test_mapping_header_compiles_on_its_own_through_the_drivers_statements(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    inc = [os.path.join(cases.ROOT, "include"), os.path.join(cases.ROOT, "include", "UnifiedCvo")]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-c"] + [f"-I{p}" for p in inc] +
                          ["-o", str(tmp_path / "bki_headers_check.o"), os.path.join(cases.ROOT, "tests", "cpp", "bki_headers_check.cpp")])


@pytest.mark.gpu
def test_device_through_the_drivers_statements(tmp_path):
    yaml = os.path.join(cases.CONFIGS, "geometric_gpu.yaml")
    _check(tmp_path, ["--device", yaml], dict(os.environ, CVO_BKI_HOST="0"), on_device=1)
