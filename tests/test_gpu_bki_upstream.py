"""The semantic voxel map on the device (BKI_HOST=0) against upstream's OWN compiled code: the kernels of cvo_k_bki.h on the
frames of tests/golden/bki_upstream.npz (scripts/make_bki_upstream_golden.py), compared directly with what upstream's R-tree,
key functions and Semantics made of them - keys, ms and fs after every frame, and the cloud's rows for exactly upstream's
OCCUPIED voxels - and on the threshold sequences.  Bit patterns and integers, no tolerance; reads nothing but tests/golden/."""
import pytest

import bki_cases as bc
import bki_upstream as bu
import cases
import np_bki
import test_bki_upstream as ups
import test_gpu_bki as dev
from unified_cvo_amd import CvoGPU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    g = CvoGPU(params=cases.load_params("geometric_gpu"))  # one context across the cases
    g.set_option("BKI_HOST", 0)
    yield g
    g.close()


@pytest.mark.parametrize("i", range(len(ups.CASES)))
def test_device_inserts(gpu, i):
    C, par, frames = ups.CASES[i]
    got = dev.run_device(gpu, (ups.config_of(C, par), frames))  # (asserts on_device == 1 after every frame)
    for f, (stats, cloud, size) in enumerate(got):
        ups.against_upstream(i, f, (stats["keys"], stats["ms"], stats["fs"]), cloud, "device")
        assert size == (len(ups.FX[f"ins{i}_{f}_key"]), int((ups.FX[f"ins{i}_{f}_state"] == np_bki.OCCUPIED).sum()))
        assert ups.LONGEST[i][f] in (None, stats["longest_run"])
    # the runs of 17, 65 and 300 hits in one voxel are summed by the wave kernel (k_bki_long), each the longest of its frame
    assert ups.LONGEST[0] == [17, 65, 300] and 17 > bc.SHORT_RUN == ups.LONGEST[2][0]


@pytest.mark.parametrize("row", range(len(bc.THRESHOLDS)))
def test_device_thresholds(gpu, row):
    ups.threshold_run_agrees(lambda case: dev.run_device(gpu, case), row)
    assert bu.node_steps(ups.FX)[row][-1]["state"] == bc.THRESHOLDS[row][3]
