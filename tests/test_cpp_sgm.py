"""The stereo matcher through the C++ side: host/cvo_sgm_check (the C-ABI's CPU twin from a C++ program, and
cvo::ImageStereo's (left, right) constructor; CvoGPU::stereo_disparity under -m gpu) against the numpy statement and against
the five-argument ImageStereo constructor given the statement's map (host/cvo_stereo_check)."""
import os
import subprocess

import numpy as np
import pytest

import cases
import np_sgm
import sgm_cases as sc

CHECK = os.path.join(cases.ROOT, "host", "cvo_sgm_check")
STEREO_CHECK = os.path.join(cases.ROOT, "host", "cvo_stereo_check")
ROWS, COLS, D0 = 150, 96, 12  # (the stereo front end keeps rows 100 .. rows - 30 only)
CONFIGS = ({}, dict(max_disparity=64, p1=7, p2=60, uniqueness=10, lr_max_diff=0, paths=4))


def _fnv(a):
    h = 14695981039346656037
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _config_args(config):
    c = {**dict(max_disparity=128, p1=10, p2=120, uniqueness=5, lr_max_diff=1, paths=8), **config}
    return ["--config"] + [str(c[k]) for k in ("max_disparity", "p1", "p2", "uniqueness", "lr_max_diff", "paths")] if config else []


def _run(args, env=None):
    assert os.path.exists(CHECK), "build the host tools first (make -C host)"
    return subprocess.check_output([CHECK] + [str(a) for a in args], text=True, timeout=300, env=env).splitlines()


def _planes(tmp_path, rows, cols, d0, seed=0):
    left, right = sc.shift(rows, cols, d0, seed)
    np.save(tmp_path / "left.npy", left)
    np.save(tmp_path / "right.npy", right)
    return left, right, [tmp_path / "left.npy", tmp_path / "right.npy"]


def test_twin_from_cpp_matches_the_statement(tmp_path):
    for rows, cols, d0 in ((24, 100, 17), (7, 63, 3), (1, 1, 0)):
        _, _, files = _planes(tmp_path, rows, cols, d0)
        for config in CONFIGS:
            want = sc.statement("shift", rows, cols, 0, d0, **config)["disparity"]
            out = _run(files + _config_args(config))
            assert out == [f"shape {rows} {cols}", "disparity " + _fnv(want)], (rows, cols, config)
    want = sc.statement("shift", 24, 100, 0, 17)
    assert want["valid"].mean() > 0.5 and _fnv(want["disparity"]) != _fnv(np.zeros((24, 100), np.float32))


def _frame_lines(tmp_path, files, config, extra=(), env=None):
    """What the (left, right) constructor's frame gives, and what the five-argument one gives with the statement's map."""
    calib = tmp_path / "calib.txt"
    calib.write_text("707.09 707.09 48.0 75.0 0.54\n")
    want_map = sc.statement("shift", ROWS, COLS, 0, D0, **config)["disparity"]
    np.save(tmp_path / "disparity.npy", want_map)
    out = {}
    for method in ("FULL", "CV_FAST", "DSO_EDGES"):
        got = _run(files + _config_args(config) + ["--points", calib, method] + list(extra), env)
        assert got[:2] == [f"shape {ROWS} {COLS}", "disparity " + _fnv(want_map)], method
        want = subprocess.check_output([STEREO_CHECK, str(files[0]), str(tmp_path / "disparity.npy"), str(calib), method], text=True, timeout=300).splitlines()
        assert got[2:] == want, method
        out[method] = int(want[0].split()[1])
    return out


def test_the_left_right_constructor_yields_the_frame_of_the_statements_map(tmp_path):
    _, _, files = _planes(tmp_path, ROWS, COLS, D0)
    n = _frame_lines(tmp_path, files, {})
    assert n["FULL"] > 500  # (the frame does yield points: the comparison is not of two empty clouds)
    _frame_lines(tmp_path, files, CONFIGS[1])


def test_a_bgr_pair_goes_to_gray_by_the_front_ends_formula(tmp_path):
    rng = np.random.default_rng(5)
    right = rng.integers(0, 256, (ROWS, COLS, 3), dtype=np.uint8)
    left = rng.integers(0, 256, (ROWS, COLS, 3), dtype=np.uint8)
    left[:, D0:] = right[:, :COLS - D0]
    np.save(tmp_path / "l.npy", left)
    np.save(tmp_path / "r.npy", right)
    gray = lambda a: ((a.astype(np.int64) @ np.array([1868, 9617, 4899]) + 8192) >> 14).astype(np.uint8)
    want = np_sgm.disparity(gray(left), gray(right))
    calib = tmp_path / "calib.txt"
    calib.write_text("707.09 707.09 48.0 75.0 0.54\n")
    out = _run([tmp_path / "l.npy", tmp_path / "r.npy", "--points", calib, "FULL"])
    assert out[1] == "disparity " + _fnv(want) and int(out[2].split()[1]) > 500


def test_driver_refuses_what_the_library_refuses(tmp_path):
    _, _, files = _planes(tmp_path, 6, 7, 1)
    np.save(tmp_path / "f32.npy", np.zeros((6, 7), np.float32))
    np.save(tmp_path / "other.npy", np.zeros((6, 8), np.uint8))
    l, r = str(files[0]), str(files[1])
    for args in ([l, r, "--config", "96", "10", "120", "5", "1", "8"], [l, r, "--config", "64", "10", "120", "5", "1", "5"], [l, str(tmp_path / "f32.npy")],
                 [l, str(tmp_path / "other.npy")], [l, r, "--what"]):
        res = subprocess.run([CHECK] + args, capture_output=True, text=True)
        assert res.returncode == 1 and "cvo_sgm_check:" in res.stderr, args


@pytest.mark.gpu
def test_device_route_matches_the_statement(tmp_path):
    yaml = os.path.join(cases.CONFIGS, "geometric_gpu.yaml")
    env = dict(os.environ, CVO_SGM_HOST="0")  # the kernels, whatever the size
    _, _, files = _planes(tmp_path, 24, 100, 17)
    for config in CONFIGS:
        want = sc.statement("shift", 24, 100, 0, 17, **config)["disparity"]
        assert _run(files + _config_args(config) + ["--device", yaml], env)[1] == "disparity " + _fnv(want), config
    _, _, files = _planes(tmp_path, ROWS, COLS, D0)
    _frame_lines(tmp_path, files, {}, ["--device", yaml], env)
    res = subprocess.run([CHECK, str(files[0]), str(files[1]), "--config", "96", "10", "120", "5", "1", "8", "--device", yaml], capture_output=True, text=True, env=env)
    assert res.returncode == 1 and "cvo_stereo_disparity" in res.stderr
