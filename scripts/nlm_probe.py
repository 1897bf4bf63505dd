"""Non-local-means denoising (RawImage's first statement): what a frame costs on the kernel and on the CPU twin.

  python scripts/nlm_probe.py [--out DIR] [--reps N]     wall times at 640 x 480 and 1241 x 376, DIR/nlm_probe.{json,txt}
  python scripts/nlm_probe.py --crossover                small square frames (the NLM_HOST default), DIR/crossover.{json,txt}
  rocprofv3 --kernel-trace --stats -d DIR/trace -o nlm --output-format csv -- python scripts/nlm_probe.py --kernels
                                                          the launches a profiler should see, nothing else

Frames: the noisy two-level steps of tests/nlm_cases.py, one channel (cv::fastNlMeansDenoising) and three channels through
the Lab route (the middle of cv::fastNlMeansDenoisingColored), h = h_color = 10, windows 7 / 21: RawImage's call.  Routes,
alternated call by call in ONE process (other work shares the machine):
  device  NLM_HOST=0: upload, k_nlm (two launches for Lab), download, one synchronisation;
  twin    NLM_HOST=1: the same call on one CPU thread.  The twin is the baseline because it is the only other
          implementation here: OpenCV is not available to this script, so OpenCV's own time is not measured.
Wall time is a host clock around the call, which returns after the upload stream has been synchronised: the median and the
spread of --reps calls after two warm-up calls per route.  The routes' images are compared.  A size where the device loses
is reported like any other.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nlm_cases as nc  # noqa: E402
from unified_cvo_amd import CvoGPU  # noqa: E402

FRAMES = ((480, 640), (376, 1241))
CROSSOVER_SIDES = (8, 12, 16, 24, 32, 48, 64, 96, 128)


def routes(gpu, img, lab):
    call = gpu.nlm_denoise_lab if lab else gpu.nlm_denoise

    def with_host(route):
        def run():
            gpu.set_option("NLM_HOST", route)
            try:
                return call(img)
            finally:
                gpu.set_option("NLM_HOST", None)
        return run

    return {"device": with_host(0), "twin": with_host(1)}


def measure(fns, reps):
    ts, out = {k: [] for k in fns}, {}
    for rep in range(reps + 2):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            out[name] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= 2:
                ts[name].append(dt)
    first = next(iter(out.values()))
    assert all(np.array_equal(first, p) for p in out.values())
    return {k: [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nlm"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--kernels", action="store_true", help="only the launches, for a kernel trace")
    ap.add_argument("--crossover", action="store_true", help="small frames: where the kernel overtakes the CPU twin")
    a = ap.parse_args()
    shapes = tuple((s, s) for s in CROSSOVER_SIDES) if a.crossover else FRAMES
    gpu = CvoGPU()
    if a.kernels:
        gpu.set_option("NLM_HOST", 0)
        for rows, cols in FRAMES:
            for _ in range(5):
                gpu.nlm_denoise(nc.image("steps", rows, cols))
            for _ in range(5):
                gpu.nlm_denoise_lab(nc.image("steps", rows, cols, 3))
        print(gpu.debug_nlm_stats(), flush=True)
        gpu.close()
        return
    os.makedirs(a.out, exist_ok=True)
    rows_out, lines = [], []
    for rows, cols in shapes:
        for lab in (False, True):
            img = nc.image("steps", rows, cols, 3 if lab else 1)
            ms = measure(routes(gpu, img, lab), a.reps)
            rows_out.append({"rows": rows, "cols": cols, "pixels": rows * cols, "image": "lab" if lab else "gray", "ms": ms})
            line = (f"{cols:4d} x {rows:3d} ({rows * cols:6d} pixels) {'Lab ' if lab else 'gray'} | ms "
                    + "  ".join(f"{k} {v[0]:.3f} [{v[1]:.3f}..{v[2]:.3f}]" for k, v in ms.items()))
            print(line, flush=True)
            lines.append(line)
    gpu.close()
    name = "crossover" if a.crossover else "nlm_probe"
    with open(os.path.join(a.out, name + ".json"), "w") as fo:
        json.dump({"reps": a.reps, "ms": "median [min, max] of a host clock around the call", "rows": rows_out}, fo, indent=1)
    with open(os.path.join(a.out, name + ".txt"), "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
