"""The sparse kernel through the C++ side: host/cvo_bki_sparse_check builds semantic_bki::SemanticBKIOctoMap and inserts frame
by frame with insert_pointcloud (the signature upstream's header keeps commented out) or insert_pointcloud_csm - the CPU twin,
and the device under -m gpu - against the numpy statement (np_bki_sparse.py): the rows of the cloud and the whole table."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bki_sparse_cases as sc
import cases

CHECK = os.path.join(cases.ROOT, "host", "cvo_bki_sparse_check")
NAMES = ("three_inserts", "csm_sparse_csm", "run65_beside")


def _fnv(parts):
    h = 14695981039346656037
    for a in parts:
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _case_args(path, name):
    cfg, frames = sc.all_cases()[name]
    C = cfg.num_classes
    rows = []
    for f, (_, (xyz, feat, label, origin)) in enumerate(frames):
        n = xyz.shape[0]
        lab = label if C else np.zeros((n, 0), np.float32)
        rows.append(np.concatenate([np.full((n, 1), f, np.float32), np.tile(origin, (n, 1)), xyz, feat, lab], axis=1))
    np.save(path, np.concatenate(rows).astype(np.float32))
    kernels = "".join("s" if k == sc.SPARSE else "c" for k, _ in frames)
    values = (cfg.resolution, cfg.prior, cfg.free_thresh, cfg.occupied_thresh, cfg.free_resolution, cfg.max_range, np.float32(cfg.sf2), np.float32(cfg.ell))
    return [str(path), str(C)] + [repr(float(v)) for v in values] + [kernels]


def _check(tmp_path, extra=(), env=None, on_device=0):
    assert os.path.exists(CHECK), "build the host tools first (make -C host)"
    for name in NAMES:
        args = _case_args(tmp_path / "case.npy", name)
        out = subprocess.check_output([CHECK] + args + list(extra), text=True, timeout=300, env=env).splitlines()
        (keys, ms, fs), (xyz, feat, label), _ = sc.statement_of(name)[-1]
        rows = [np.concatenate([xyz[i], feat[i], label[i]]).astype(np.float32) for i in range(len(xyz))]
        table = []
        for v in range(len(keys)):
            table += [keys[v:v + 1], ms[v], fs[v]]
        assert len(xyz) > 3 and len(keys) > 30
        assert out == [f"cloud {len(xyz)}", "rows " + _fnv(rows), f"table {len(keys)} " + _fnv(table), f"on_device {on_device}"], name


def test_twin_through_the_veneer(tmp_path):
    _check(tmp_path)


def test_driver_refuses_what_the_library_refuses(tmp_path):
    args = _case_args(tmp_path / "case.npy", "run65_beside")
    for bad in (args[:8] + ["0.0"] + args[9:], args[:9] + ["nan"] + args[10:], args[:10] + ["x"], args + ["--what"]):
        res = subprocess.run([CHECK] + bad, capture_output=True, text=True)
        assert res.returncode == 1 and "cvo_bki_sparse_check:" in res.stderr, bad
    res = subprocess.run([CHECK] + args[:8] + ["0.0"] + args[9:10] + ["c"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr  # (the counting kernel never looks at sf2)


def test_mapping_header_compiles_on_its_own_with_the_sparse_inserts(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    inc = [os.path.join(cases.ROOT, "include"), os.path.join(cases.ROOT, "include", "UnifiedCvo")]
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-c"] + [f"-I{p}" for p in inc] +
                          ["-o", str(tmp_path / "bki_sparse_headers_check.o"), os.path.join(cases.ROOT, "tests", "cpp", "bki_sparse_headers_check.cpp")])


@pytest.mark.gpu
def test_device_through_the_veneer(tmp_path):
    yaml = os.path.join(cases.CONFIGS, "geometric_gpu.yaml")
    _check(tmp_path, ["--device", yaml], dict(os.environ, CVO_BKI_HOST="0"), on_device=1)
