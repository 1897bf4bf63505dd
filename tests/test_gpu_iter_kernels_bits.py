"""The per-iteration kernels (k_assoc, k_coeff) bit for bit: short aligns must end on exactly the pose bytes and iteration
counts recorded in tests/golden/iter_kernels_bits.json (scripts/make_iter_bits_fixture.py).  Three ways through the
kernels per case: a traced run (the update never speculates), an untraced run (the speculative update is adopted) and
a run with CVO_SKIN=0 (a candidate scan every iteration, no list reuse); on the 10k geometric pair of the headline
workload and on the colour config."""
import json
import os

import numpy as np
import pytest

import cases
from unified_cvo_amd import CvoGPU

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(cases.GOLDEN, "iter_kernels_bits.json")
N_IT = 200
CASES = {"config2_n10000": lambda: cases.config2(n=10000), "config3_n2000": lambda: cases.config3(n=2000)}
VARIANTS = ("traced", "speculative", "skin0")


def run(name, variant):
    P, src, tgt, init = CASES[name]()
    old = os.environ.get("CVO_SKIN")
    if variant == "skin0":
        os.environ["CVO_SKIN"] = "0"
    try:
        gpu = CvoGPU(params=P)
        kw = dict(trace_capacity=N_IT, trace_dense=N_IT) if variant == "traced" else {}
        r = gpu.align(src, tgt, init, max_iterations=N_IT, **kw)
    finally:
        if variant == "skin0":
            if old is None:
                os.environ.pop("CVO_SKIN", None)
            else:
                os.environ["CVO_SKIN"] = old
    return {"iterations": int(r.iterations), "transform": np.ascontiguousarray(r.transform, np.float32).tobytes().hex()}


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_iteration_kernels_reproduce_recorded_bits(name, variant):
    want = _fixture()[name][variant]
    got = run(name, variant)
    assert got["iterations"] == want["iterations"], (name, variant, got["iterations"], want["iterations"])
    assert got["transform"] == want["transform"], (name, variant)
