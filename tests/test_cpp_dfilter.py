"""The disparity post-filter through the C++ side: host/cvo_dfilter_check (the C-ABI's CPU twin from a C++ program, in place;
cvo::ImageStereo's (left, right, ..., dfilter) constructor; CvoGPU::disparity_filter and the filtered CvoGPU::stereo_disparity
under -m gpu) against the numpy statement."""
import os
import subprocess

import numpy as np
import pytest

import cases
import dfilter_cases as dc
import np_dfilter
import sgm_cases as sc

CHECK = os.path.join(cases.ROOT, "host", "cvo_dfilter_check")
NAMES = ("golden", "blobs", "blobs sim 0", "gap 5000 columns 129", "mean 9x16", "1x1 removed")
PAIR = (64, 200, 3, 64)  # rows, cols, seed, max_disparity of the two_planes pair


def _fnv(a):
    h = 14695981039346656037
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def _config_args(cfg):
    return ["--config", repr(cfg.speckle_sim_threshold), cfg.speckle_size, cfg.ipol_gap_width, cfg.adaptive_mean]


def _run(args, env=None):
    assert os.path.exists(CHECK), "build the host tools first (make -C host)"
    return subprocess.check_output([CHECK] + [str(a) for a in args], text=True, timeout=300, env=env).splitlines()


def _maps(tmp_path, extra=(), env=None):
    for name in NAMES:
        d, cfg = dc.cases()[name]
        np.save(tmp_path / "map.npy", d)
        want = dc.statement(name)["out"]
        assert _run([tmp_path / "map.npy"] + _config_args(cfg) + list(extra), env) == [f"shape {d.shape[0]} {d.shape[1]}", "filtered " + _fnv(want)], name
    d = dc.golden_input()
    np.save(tmp_path / "map.npy", d)
    assert _run([tmp_path / "map.npy"] + list(extra), env)[1] == "filtered " + _fnv(dc.statement("golden")["out"])  # the default configuration
    assert _fnv(dc.statement("golden")["out"]) != _fnv(d)


def _pair(tmp_path, extra=(), env=None):
    rows, cols, seed, D = PAIR
    left, right, _ = sc.two_planes(rows, cols, seed)
    np.save(tmp_path / "left.npy", left)
    np.save(tmp_path / "right.npy", right)
    raw = sc.statement("two_planes", rows, cols, seed, max_disparity=D)["disparity"]
    for cfg in (np_dfilter.Config(), np_dfilter.Config(1.0, 30, 2, 0)):
        want = np_dfilter.dfilter(raw, cfg)
        out = _run(["--pair", tmp_path / "left.npy", tmp_path / "right.npy", D] + _config_args(cfg) + list(extra), env)
        assert out == [f"shape {rows} {cols}", "filtered " + _fnv(want)], vars(cfg)
        assert _fnv(want) != _fnv(raw)


def test_twin_from_cpp_matches_the_statement(tmp_path):
    _maps(tmp_path)


def test_the_left_right_constructor_with_a_filter(tmp_path):
    _pair(tmp_path)


def test_driver_refuses_what_the_library_refuses(tmp_path):
    np.save(tmp_path / "map.npy", dc.golden_input())
    np.save(tmp_path / "u8.npy", np.zeros((6, 7), np.uint8))
    bad = dc.golden_input()
    bad[3, 3] = np.nan
    np.save(tmp_path / "nan.npy", bad)
    m = str(tmp_path / "map.npy")
    for args in ([m, "--config", "-1", "200", "3", "1"], [m, "--config", "1", "-5", "3", "1"], [m, "--config", "1", "200", "-1", "1"], [str(tmp_path / "u8.npy")],
                 [str(tmp_path / "nan.npy")], [m, "--what"], ["--config", "1", "200", "3", "1"]):
        res = subprocess.run([CHECK] + args, capture_output=True, text=True)
        assert res.returncode == 1 and "cvo_dfilter_check:" in res.stderr, args


@pytest.mark.gpu
def test_device_route_matches_the_statement(tmp_path):
    yaml = os.path.join(cases.CONFIGS, "geometric_gpu.yaml")
    env = dict(os.environ, CVO_DFILTER_HOST="0", CVO_SGM_HOST="0")  # the kernels, whatever the size
    _maps(tmp_path, ["--device", yaml], env)
    _pair(tmp_path, ["--device", yaml], env)
    np.save(tmp_path / "map.npy", dc.golden_input())
    res = subprocess.run([CHECK, str(tmp_path / "map.npy"), "--config", "-1", "200", "3", "1", "--device", yaml], capture_output=True, text=True, env=env)
    assert res.returncode == 1 and "cvo_disparity_filter" in res.stderr
