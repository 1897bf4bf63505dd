"""Stereo front end: what a left frame + disparity costs on its way to CV_FAST points and to a resident cloud.

  python scripts/stereo_probe.py [--out DIR] [--reps N]     wall times, written to DIR/stereo_probe.{json,txt}
  python scripts/stereo_probe.py --crossover                route times of small frames (the STEREO_HOST default), DIR/crossover.{json,txt}
  rocprofv3 --kernel-trace --stats -d DIR/trace -o stereo --output-format csv -- python scripts/stereo_probe.py --kernels
                                                            the launches a profiler should see, nothing else

Frames: synth.stereo_frame("textured") at 376 x 1241 and 480 x 640, no NaN disparities, leaf 0.5, edge divisor 5.
Stages, each on routes alternated call by call in ONE process (other work shares the machine):
  points   stereo_points(CV_FAST): device (STEREO_HOST=0, the kernels of cvo_k_fast.h / cvo_k_stereo.h) against twin
           (STEREO_HOST=1: the same selection on one CPU thread - the only route a caller could take before);
  upload   upload_stereo(CV_FAST): device against before = cvo_stereo_points_host into preallocated arrays + the ordinary upload;
  recipe   upload_stereo_recipe: device against twin (STEREO_HOST=1) and before = cvo_stereo_points_host twice, the rows
           turned into colour clouds with numpy, two upload_voxel calls (two resident clouds, not one);
  select   fast_select alone with FAST_TILE=1 and 0 (the LDS tile against ring reads through the cache) and the twin.
Wall time is a host clock around the call, which returns after the upload stream has been synchronised: the median and
the spread of --reps calls after two warm-up calls per route.  The pixels of the routes are compared.  A stage where
the device loses is reported like any other.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from unified_cvo_amd import CvoGPU, CvoPointCloud, StereoFrame, synth  # noqa: E402
from unified_cvo_amd.api import CV_FAST, DSO_EDGES, FAST_STEREO, FULL, _fptr  # noqa: E402

SHAPES = ((376, 1241), (480, 640))
CROSSOVER_SHAPES = ((140, 72), (140, 100), (140, 140), (160, 200), (200, 320), (240, 400))
LEAF, DIVISOR = 0.5, 5.0


def gray_of(f):
    b, g, r = (f.image[..., k].astype(np.int64) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


class Before:
    """The routes of a caller without the device front end, buffers allocated once."""

    def __init__(self, gpu, frame):
        self.gpu, self.f, self.fs = gpu, frame, frame.c_struct()
        n = frame.rows * frame.cols
        self.pixel = np.zeros(n, np.int32)
        self.xyz, self.feat = np.zeros((n, 3), np.float32), np.zeros((n, frame.channels + 2), np.float32)
        self.geo = np.zeros((n, 2), np.float32)
        self.n = C.c_int()

    def points(self, method):
        rc = self.gpu.L.cvo_stereo_points_host(C.byref(self.fs), method, self.pixel.ctypes.data_as(C.POINTER(C.c_int)), C.byref(self.n),
                                               _fptr(self.xyz), _fptr(self.feat), None, _fptr(self.geo))
        assert rc == 0
        return self.n.value

    def upload(self):
        k = self.points(CV_FAST)
        d = self.gpu.upload(CvoPointCloud.from_arrays(self.xyz[:k], self.feat[:k], None, self.geo[:k]))
        d.free()
        return self.pixel[:k].copy()

    def recipe(self):
        out = []
        for method, s, gt in ((DSO_EDGES, np.float32(LEAF) / np.float32(DIVISOR), (1.0, 0.0)), (FULL, LEAF, (0.0, 1.0))):
            k = self.points(method)
            feat = np.zeros((k, 5), np.float32)
            feat[:, :3] = self.feat[:k, :3]  # (the byte round trip is the identity on 3-channel frames)
            pc = CvoPointCloud.from_arrays(self.xyz[:k], feat, None, np.tile(np.array([gt], np.float32), (k, 1)))
            d = self.gpu.upload_voxel(pc, float(s))
            out.append(self.pixel[:k][d.kept])
            d.free()
        return np.concatenate(out)


def stages(gpu, f):
    """stage -> {route -> callable returning the pixels}; a route sets its own switches."""
    before, gray = Before(gpu, f), gray_of(f)

    def with_opts(opts, fn):
        def run():
            for k, v in opts.items():
                gpu.set_option(k, v)
            try:
                return fn()
            finally:
                for k in opts:
                    gpu.set_option(k, None)
        return run

    def resident(call):
        d = call()
        p = d.pixel
        d.free()
        return p

    return {
        "points": {"device": with_opts({"STEREO_HOST": 0}, lambda: gpu.stereo_points(f, CV_FAST).pixel),
                   "twin": with_opts({"STEREO_HOST": 1}, lambda: gpu.stereo_points(f, CV_FAST).pixel)},
        "upload": {"device": with_opts({"STEREO_HOST": 0}, lambda: resident(lambda: gpu.upload_stereo(f, CV_FAST))),
                   "before": before.upload},
        "recipe": {"device": with_opts({"STEREO_HOST": 0}, lambda: resident(lambda: gpu.upload_stereo_recipe(f, LEAF, DIVISOR))),
                   "twin": with_opts({"STEREO_HOST": 1}, lambda: resident(lambda: gpu.upload_stereo_recipe(f, LEAF, DIVISOR))),
                   "before": before.recipe},
        "select": {"device": with_opts({"STEREO_HOST": 0, "FAST_TILE": 1}, lambda: gpu.fast_select(gray, FAST_STEREO)[0]),
                   "cache": with_opts({"STEREO_HOST": 0, "FAST_TILE": 0}, lambda: gpu.fast_select(gray, FAST_STEREO)[0]),
                   "twin": with_opts({"STEREO_HOST": 1}, lambda: gpu.fast_select(gray, FAST_STEREO)[0])},
    }


def measure(routes, reps):
    ts, pix = {k: [] for k in routes}, {}
    for rep in range(reps + 2):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            pix[name] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= 2:
                ts[name].append(dt)
    first = next(iter(pix.values()))
    assert all(np.array_equal(first, p) for p in pix.values())
    return {k: [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for k, v in ts.items()}, int(len(first))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--kernels", action="store_true", help="only the launches, for a kernel trace")
    ap.add_argument("--crossover", action="store_true", help="small frames: where the kernels overtake the CPU twin")
    ap.add_argument("--shapes", nargs="+", default=None, help="frame sizes, ROWSxCOLS")
    a = ap.parse_args()
    shapes = [tuple(map(int, s.split("x"))) for s in a.shapes] if a.shapes else (CROSSOVER_SHAPES if a.crossover else SHAPES)
    gpu = CvoGPU()
    frames = [StereoFrame(**synth.stereo_frame("textured", rows, cols, nan_pixels=False)) for rows, cols in shapes]
    if a.kernels:
        gpu.set_option("STEREO_HOST", 0)
        for f in frames:
            for tile in (1, 0):
                gpu.set_option("FAST_TILE", tile)
                for _ in range(5):
                    gpu.upload_stereo(f, CV_FAST).free()
                print(f"{f.cols}x{f.rows} FAST_TILE={tile}: {gpu.debug_stereo_stats()['tried']}", flush=True)
            gpu.set_option("FAST_TILE", None)
            for _ in range(5):
                gpu.upload_stereo_recipe(f, LEAF, DIVISOR).free()
        gpu.close()
        return
    os.makedirs(a.out, exist_ok=True)
    rows, lines = [], []
    for f in frames:
        for stage, routes in stages(gpu, f).items():
            if a.crossover and stage == "select":
                continue
            ms, points = measure(routes, a.reps)
            rows.append({"cols": f.cols, "rows": f.rows, "pixels": f.rows * f.cols, "stage": stage, "points": points, "ms": ms})
            line = (f"{f.cols:5d} x {f.rows:4d} {stage:7s} points {points:6d} | ms "
                    + "  ".join(f"{k} {v[0]:.2f} [{v[1]:.2f}..{v[2]:.2f}]" for k, v in ms.items()))
            print(line, flush=True)
            lines.append(line)
    gpu.close()
    name = "crossover" if a.crossover else "stereo_probe"
    with open(os.path.join(a.out, name + ".json"), "w") as fo:
        json.dump({"reps": a.reps, "leaf": LEAF, "edge_divisor": DIVISOR, "ms": "median [min, max] of a host clock around the call", "rows": rows}, fo, indent=1)
    with open(os.path.join(a.out, name + ".txt"), "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
