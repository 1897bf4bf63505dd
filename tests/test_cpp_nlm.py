"""The denoising through the C++ side: host/cvo_nlm_check (the C-ABI's CPU twin from a C++ program; CvoGPU::nlm_denoise /
nlm_denoise_lab under -m gpu) against the numpy statement."""
import os
import subprocess

import numpy as np
import pytest

import cases
import nlm_cases as nc

CHECK = os.path.join(cases.ROOT, "host", "cvo_nlm_check")


def _fnv(a):
    h = 14695981039346656037
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _run(args, env=None):
    assert os.path.exists(CHECK), "build the host tools first (make -C host)"
    shape, digest = subprocess.check_output([CHECK] + [str(a) for a in args], text=True, timeout=300, env=env).splitlines()
    return tuple(int(v) for v in shape.split()[1:]), digest.split()[1]


def _cases(tmp_path):
    """(arguments, the statement's image)"""
    gray, bgr = nc.image("steps", 20, 31), nc.image("steps", 20, 31, 3)
    np.save(tmp_path / "gray.npy", gray)
    np.save(tmp_path / "bgr.npy", bgr)
    g, b = tmp_path / "gray.npy", tmp_path / "bgr.npy"
    return [([g], nc.statement("steps", 20, 31)), ([g, "--in-place"], nc.statement("steps", 20, 31)),
            ([g, "--h", 3, "--windows", 3, 5], nc.statement("steps", 20, 31, 1, 3, (3, 5))),
            ([b], nc.statement("steps", 20, 31, 3)), ([b, "--lab", 7], nc.statement_lab("steps", 20, 31, 10, 7)),
            ([b, "--lab", 7, "--in-place"], nc.statement_lab("steps", 20, 31, 10, 7))]


def test_twin_from_cpp_matches_the_statement(tmp_path):
    for args, want in _cases(tmp_path):
        shape, digest = _run(args)
        assert shape == (20, 31, 1 if want.ndim == 2 else 3) and digest == _fnv(want), args
    assert _fnv(nc.statement("steps", 20, 31)) != _fnv(nc.image("steps", 20, 31))


def test_driver_refuses_what_the_library_refuses(tmp_path):
    np.save(tmp_path / "gray.npy", nc.image("steps", 6, 7))
    np.save(tmp_path / "f32.npy", np.zeros((6, 7), np.float32))
    g = str(tmp_path / "gray.npy")
    for args in ([g, "--h", "0"], [g, "--windows", "9", "21"], [g, "--lab", "10"], [str(tmp_path / "f32.npy")], [g, "--what"]):
        r = subprocess.run([CHECK] + args, capture_output=True, text=True)
        assert r.returncode == 1 and "cvo_nlm_check:" in r.stderr, args


@pytest.mark.gpu
def test_device_route_matches_the_statement(tmp_path):
    yaml = os.path.join(cases.CONFIGS, "geometric_gpu.yaml")
    for args, want in _cases(tmp_path):
        shape, digest = _run(args + ["--device", yaml], dict(os.environ, CVO_NLM_HOST="0"))  # the kernel, whatever the size
        assert digest == _fnv(want), args
    r = subprocess.run([CHECK, str(tmp_path / "gray.npy"), "--windows", "9", "21", "--device", yaml], capture_output=True, text=True)
    assert r.returncode == 1 and "cvo_nlm_denoise" in r.stderr
