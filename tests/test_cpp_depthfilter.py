"""The C++ veneer of the keyframe depth filter: host/cvo_depth_filter_check runs CvoGPU::depth_filter, with host clouds (the
driver's kf_filtered) and with resident clouds, against the driver's loops written out on the host over
compute_association_gpu."""
import os
import subprocess

import pytest

import cases

DRV = os.path.join(cases.ROOT, "host", "cvo_depth_filter_check")


def test_check_program_is_built_and_registered():
    assert os.path.exists(DRV), "python __graft_entry__.py builds host/ (make -C host)"
    assert "cvo_depth_filter_check" in open(os.path.join(cases.ROOT, "host", "Makefile")).read()
    assert "host/cvo_depth_filter_check.cpp" in open(os.path.join(cases.ROOT, "CMakeLists.txt")).read()
    out = subprocess.run([DRV], capture_output=True, text=True, timeout=60)   # no arguments: the usage line, no device touched
    assert out.returncode == 2 and "usage" in out.stderr


@pytest.mark.gpu
def test_cpp_veneer_filters_a_keyframe():
    """Rows 0 .. 9 of the 60 see three observations and are dropped, the others four or five: 50 points, in both forms;
    coordinates bit for bit the host loops', indices and attributes equal."""
    out = subprocess.run([DRV, os.path.join(cases.CONFIGS, "outdoor.yaml")], capture_output=True, text=True, timeout=120)
    print(out.stdout + out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = {w[0]: w for w in (line.split() for line in out.stdout.strip().splitlines()) if len(w) == 7}
    assert set(lines) == {"clouds", "resident"}, out.stdout
    for name in ("clouds", "resident"):
        w = lines[name]
        assert int(w[2]) == 50 and int(w[4]) == 0 and w[6] == "equal", out.stdout
