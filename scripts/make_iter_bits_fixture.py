#!/usr/bin/env python
"""Records tests/golden/iter_kernels_bits.json (GPU box): the exact final pose bytes and iteration counts of short aligns
through the per-iteration kernels - a traced run (no speculation), an untraced run (the speculative update adopts) and a
CVO_SKIN=0 run (a candidate scan every iteration) - on the 10k geometric pair of the headline workload and on the colour
config.  tests/test_gpu_iter_kernels_bits.py holds every later build of the kernels to these bits.
usage: python scripts/make_iter_bits_fixture.py [OUT.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_iter_kernels_bits as T  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
rec = {"generator": "scripts/make_iter_bits_fixture.py",
       "note": "final transform as float32 bytes (hex, column order of AlignResult.transform) and iterations per run",
       "cases": {}}
for name in T.CASES:
    rec["cases"][name] = {v: T.run(name, v) for v in T.VARIANTS}
    print(name, rec["cases"][name], flush=True)
with open(out, "w") as f:
    json.dump(rec, f, indent=1)
print("written", out)
