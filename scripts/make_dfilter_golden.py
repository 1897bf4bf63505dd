#!/usr/bin/env python
"""Makes tests/golden/dfilter_elas.npz: what libelas's OWN compiled removeSmallSegments, gapInterpolation and adaptiveMean
leave of a generated map, so that tests/np_dfilter.py is pinned against the reference's code and not against a reading of it.

    python scripts/make_dfilter_golden.py /path/to/libelas/libelas        (the directory that holds elas.h and elas.cpp)

The script writes a small driver of its own into a temporary directory (it includes elas.h with the members made reachable,
sets width / height / bpl and calls the three passes on a map read from a file), compiles it together with libelas's sources
(g++ -O2 -msse3) and runs it under several MALLOC_PERTURB_ values: adaptiveMean reads parts of a malloc'ed buffer it never
wrote, so its output depends on what malloc hands out in column 3, rows 4-6 and rows H-6 .. H-4.  One of the values makes
fresh memory read as small positive floats (a negative result is never stored, so patterns that read as negative floats hide
column 3).  The script asserts that the runs agree after the first two passes everywhere and after the mean outside that
band, and stores the input, the map after each pass (first run), the mask `agree` of pixels on which all runs agree and the
mask `pinned` = agree outside the band: inside the band runs can agree merely because every pattern tried took weight 0,
while the statement, which reads the map's own values there, legitimately differs.

Nothing of libelas, source or compiled, is kept: the temporary directory is removed, the .npz holds arrays only."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dfilter_cases  # noqa: E402

DRIVER = r"""
#define private public
#define protected public
#include "elas.h"
#undef private
#undef protected
@USING@
#include <cstdio>
#include <cstdlib>
#include <vector>

static void dump(const char* path, const std::vector<float>& d) {
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(d.data(), sizeof(float), d.size(), f) != d.size()) exit(2);
  fclose(f);
}

int main(int argc, char** argv) {
  if (argc != 7) return 1;
  const int rows = atoi(argv[1]), cols = atoi(argv[2]);
  std::vector<float> d((size_t)rows * cols);
  FILE* f = fopen(argv[3], "rb");
  if (!f || fread(d.data(), sizeof(float), d.size(), f) != d.size()) return 2;
  fclose(f);
  Elas::parameters param;  // ROBOTICS, what StaticStereo uses
  Elas elas(param);
  elas.width = cols;
  elas.height = rows;
  elas.bpl = cols + 15 - (cols - 1) % 16;
  elas.removeSmallSegments(d.data());
  dump(argv[4], d);
  elas.gapInterpolation(d.data());
  dump(argv[5], d);
  elas.adaptiveMean(d.data());
  dump(argv[6], d);
  return 0;
}
"""

# fresh memory reads as 0xAAAAAAAA (tiny negative), 0x3F3F3F3F (0.747), 0x41414141 (12.08: inside the map's range, so it takes
# weight in the windows that reach rows 0-2) and 0xFEFEFEFE (huge negative)
PERTURB = (85, 192, 190, 1)


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "elas.cpp")):
        sys.exit(__doc__)
    src = os.path.abspath(sys.argv[1])
    d = dfilter_cases.golden_input()
    rows, cols = d.shape
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        # (some copies of libelas wrap the class in a namespace)
        using = "using namespace elas;" if "namespace elas" in open(os.path.join(src, "elas.h")).read() else ""
        open(os.path.join(tmp, "driver.cpp"), "w").write(DRIVER.replace("@USING@", using))
        exe = os.path.join(tmp, "driver")
        sources = [os.path.join(src, f) for f in sorted(os.listdir(src)) if f.endswith(".cpp") and f != "main.cpp"]
        subprocess.check_call(["g++", "-O2", "-msse3", "-I", src, "-o", exe, os.path.join(tmp, "driver.cpp")] + sources)
        d.tofile(os.path.join(tmp, "in.bin"))
        for perturb in PERTURB:
            names = [os.path.join(tmp, f"{s}_{perturb}.bin") for s in ("speckle", "gap", "mean")]
            subprocess.check_call([exe, str(rows), str(cols), os.path.join(tmp, "in.bin")] + names, env=dict(os.environ, MALLOC_PERTURB_=str(perturb)))
            runs.append([np.fromfile(n, np.float32).reshape(rows, cols) for n in names])
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1]), "speckle / gap depend on the heap"
    agree = np.ones((rows, cols), bool)
    for r in runs[1:]:
        agree &= r[2].view(np.uint32) == runs[0][2].view(np.uint32)
    band = np.zeros((rows, cols), bool)
    band[:, 3] = True
    band[4:7, :] = True
    band[rows - 6:rows - 3, :] = True
    assert not (~agree & ~band).any(), "the runs differ outside column 3, rows 4-6 and rows H-6 .. H-4"
    assert (~agree).any(), "no run showed the dependence on the heap: choose other MALLOC_PERTURB_ values"
    out = os.path.join(ROOT, "tests", "golden", "dfilter_elas.npz")
    np.savez_compressed(out, input=d, speckle=runs[0][0], gap=runs[0][1], mean=runs[0][2], agree=agree, pinned=agree & ~band)
    rows_only = ~agree.copy()
    rows_only[:, 3] = False
    print(f"{out}: {rows} x {cols}, {int((~agree).sum())} pixels differ between the runs "
          f"(column 3: {int((~agree)[:, 3].sum())}, the row bands elsewhere: {int(rows_only.sum())}), {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
