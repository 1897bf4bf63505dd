"""The stereo matcher (cvo_stereo_disparity: semi-global matching over a census cost): what a frame costs on the kernels and on
the CPU twin.

  python scripts/sgm_probe.py [--out DIR] [--reps N] [--twin-reps M]   wall times at 1241 x 376 and 640 x 480, D = 128, 8 and
                                                                       4 paths, DIR/sgm_probe.{json,txt}
  python scripts/sgm_probe.py --crossover                              small frames (the SGM_HOST default), DIR/crossover.{json,txt}
  rocprofv3 --kernel-trace --stats -d DIR/trace -o sgm --output-format csv -- python scripts/sgm_probe.py --kernels
                                                                       the launches a profiler should see, nothing else

Frames: the two-plane pair of tests/sgm_cases.py (box-filtered noise, the upper half shifted by 10, the lower by 30).  Routes,
alternated call by call in ONE process (other work shares the machine):
  device  SGM_HOST=0: upload of both planes, census, one launch per direction, the selection, download, one synchronisation;
  twin    SGM_HOST=1: the same call on one CPU thread.  The twin is the baseline because it is the only other implementation
          here: neither libelas nor OpenCV's StereoSGBM is available to this script, and neither is measured or claimed.
and, for the composite, upload_stereo_pair (matcher on the device, then the stereo front end) against what a caller without it
runs: stereo_disparity_host, then upload_stereo.
Wall time is a host clock around the call, which returns after the upload stream has been synchronised: the median and the
spread of --reps calls (the twin: --twin-reps, it takes seconds) after two warm-up calls (the twin: one).  The routes' maps
are compared.  A size where the device loses is reported like any other.
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

import sgm_cases as sc  # noqa: E402
from unified_cvo_amd import CvoGPU, SGMConfig, StereoFrame, stereo_disparity_host  # noqa: E402
from unified_cvo_amd.api import CV_FAST  # noqa: E402

FRAMES = ((376, 1241), (480, 640))
CROSSOVER = ((2, 4), (4, 8), (8, 8), (8, 16), (8, 32), (16, 32), (16, 64), (32, 64), (32, 128), (64, 128), (96, 320))
CALIB = dict(fx=707.09, fy=707.09, cx=601.88, cy=183.11, baseline=0.54)


def with_host(gpu, route, fn):
    def run():
        gpu.set_option("SGM_HOST", route)
        try:
            return fn()
        finally:
            gpu.set_option("SGM_HOST", None)
    return run


def measure(fns, reps, slow=(), slow_reps=3, same=lambda a, b: np.array_equal(a, b)):
    """fns: name -> call.  Routes alternate call by call; the names in `slow` run slow_reps times after one warm-up call."""
    ts, out = {k: [] for k in fns}, {}
    for rep in range(reps + 2):
        for name, fn in fns.items():
            if name in slow and rep > slow_reps:
                continue
            t0 = time.perf_counter()
            out[name] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= (1 if name in slow else 2):
                ts[name].append(dt)
    first = next(iter(out.values()))
    assert all(same(first, p) for p in out.values())
    return {k: [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3), len(v)] for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgm"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--twin-reps", type=int, default=3)
    ap.add_argument("--kernels", action="store_true", help="only the launches, for a kernel trace")
    ap.add_argument("--crossover", action="store_true", help="small frames: where the kernels overtake the CPU twin")
    a = ap.parse_args()
    gpu = CvoGPU()
    if a.kernels:
        gpu.set_option("SGM_HOST", 0)
        for rows, cols in FRAMES:
            left, right, _ = sc.two_planes(rows, cols)
            for paths in (8, 4):
                for _ in range(5):
                    gpu.stereo_disparity(left, right, SGMConfig(paths=paths))
        print(gpu.debug_sgm_stats(), flush=True)
        gpu.close()
        return
    os.makedirs(a.out, exist_ok=True)
    rows_out, lines = [], []

    def report(rows, cols, what, ms):
        rows_out.append({"rows": rows, "cols": cols, "pixels": rows * cols, "what": what, "ms": ms})
        line = (f"{cols:4d} x {rows:3d} ({rows * cols:6d} pixels) {what:<22} | ms "
                + "  ".join(f"{k} {v[0]:.3f} [{v[1]:.3f}..{v[2]:.3f}] n={v[3]}" for k, v in ms.items()))
        print(line, flush=True)
        lines.append(line)

    if a.crossover:
        for rows, cols in CROSSOVER:
            left, right, _ = sc.two_planes(rows, cols)
            for D in (64, 128):
                cfg = SGMConfig(max_disparity=D)
                call = lambda: gpu.stereo_disparity(left, right, cfg)
                report(rows, cols, f"D {D} 8 paths", measure({"device": with_host(gpu, 0, call), "twin": with_host(gpu, 1, call)}, a.reps))
    else:
        for rows, cols in FRAMES:
            left, right, _ = sc.two_planes(rows, cols)
            for paths in (8, 4):
                cfg = SGMConfig(paths=paths)
                call = lambda: gpu.stereo_disparity(left, right, cfg)
                report(rows, cols, f"D 128 {paths} paths", measure({"device": with_host(gpu, 0, call), "twin": with_host(gpu, 1, call)}, a.reps,
                                                                    slow=("twin",), slow_reps=a.twin_reps))
            frame = StereoFrame(left, None, **CALIB)

            def pair():
                c = gpu.upload_stereo_pair(frame, right, method=CV_FAST)
                px = c.pixel
                c.free()
                return px

            def twin_then_upload():
                c = gpu.upload_stereo(StereoFrame(left, stereo_disparity_host(left, right), **CALIB), CV_FAST)
                px = c.pixel
                c.free()
                return px

            report(rows, cols, "pair -> cloud (CV_FAST)", measure({"upload_stereo_pair": with_host(gpu, 0, pair), "twin, upload_stereo": twin_then_upload},
                                                                 a.reps, slow=("twin, upload_stereo",), slow_reps=a.twin_reps))
    gpu.close()
    name = "crossover" if a.crossover else "sgm_probe"
    with open(os.path.join(a.out, name + ".json"), "w") as fo:
        json.dump({"reps": a.reps, "twin_reps": a.twin_reps, "ms": "median [min, max, calls] of a host clock around the call", "rows": rows_out}, fo, indent=1)
    with open(os.path.join(a.out, name + ".txt"), "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
