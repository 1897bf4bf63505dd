"""LiDAR front end: what a raw scan costs on its way to the LOAM selection's indices and to a resident cloud.

  python scripts/lidar_probe.py [--out DIR] [--reps N]     wall times at the HDL-64 shape, written to DIR/lidar_probe.{json,txt}
  python scripts/lidar_probe.py --crossover                route times of smaller scans (the LIDAR_HOST default), DIR/crossover.{json,txt}
  rocprofv3 --kernel-trace --stats -d DIR/trace -o lidar --output-format csv -- python scripts/lidar_probe.py --kernels
                                                            the launches a profiler should see, nothing else

Scans: the synthetic room of tests/lidar_cases.py (64 x 1800 at the default configuration: `hdl64`; smaller images with
their own angular resolution for the crossover).  Stages, each on routes alternated call by call in ONE process (other
work shares the machine):
  select   lidar_select: device (LIDAR_HOST=0, the kernels of cvo_k_lidar.h; edge_detection on the calling thread
           meanwhile) against twin (LIDAR_HOST=1: the same selection on one CPU thread - the only route a caller had);
  upload   upload_lidar: device against before = cvo_lidar_select_host into preallocated arrays, the rows gathered
           with numpy, the ordinary upload.
Wall time is a host clock around the call, which returns after the upload stream has been synchronised: the median and
the spread of --reps calls after two warm-up calls per route, every call from the same generator state.  The indices of
the routes are compared.  A stage where the device loses is reported like any other.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import lidar_cases as lc  # noqa: E402
from unified_cvo_amd import CvoGPU, CvoPointCloud, LidarConfig, LidarRand, LidarScan  # noqa: E402

CROSSOVER_SHAPES = ((16, 256), (16, 512), (16, 1024), (32, 1024), (32, 1800), (64, 1024))


def scan_of(R, H):
    """-> (LidarScan, LidarConfig) of the synthetic room on an R x H image."""
    if (R, H) == (64, 1800):
        return lc.case("hdl64")
    im = lc.Image(R, H, seed=2)
    cfg = LidarConfig(n_scan=R, horizon_scan=H, ang_res_x=360.0 / H, ground_scan_ind=(3 * R) // 4, beam_num=R,
                      segment_alpha_x=float(np.radians(360.0 / H)), segment_alpha_y=float(np.radians(im.elev_step)))
    return LidarScan(im.points()[0]), cfg


def stages(gpu, scan, cfg):
    index, n, s = np.zeros(2 * scan.n, np.int32), C.c_int(), scan.c_struct()

    def with_host(route, fn):
        def run():
            gpu.set_option("LIDAR_HOST", route)
            try:
                return fn()
            finally:
                gpu.set_option("LIDAR_HOST", None)
        return run

    def resident(d):
        p = d.pixel
        d.free()
        return p

    def before():
        rand = LidarRand(1)
        rc = gpu.L.cvo_lidar_select_host(C.byref(s), C.byref(cfg.c), C.byref(rand.c), index.ctypes.data_as(C.POINTER(C.c_int)), None, C.byref(n))
        assert rc == 0
        k = index[:n.value]
        rows = scan.xyzi[k]
        d = gpu.upload(CvoPointCloud.from_arrays(rows[:, :3], rows[:, 3:4], None, np.tile(np.array([1, 0], np.float32), (len(k), 1))))
        d.free()
        return k.copy()

    return {
        "select": {"device": with_host(0, lambda: gpu.lidar_select(scan, cfg, LidarRand(1))[0]),
                   "twin": with_host(1, lambda: gpu.lidar_select(scan, cfg, LidarRand(1))[0])},
        "upload": {"device": with_host(0, lambda: resident(gpu.upload_lidar(scan, cfg, LidarRand(1)))),
                   "before": before},
    }


def measure(routes, reps):
    ts, out = {k: [] for k in routes}, {}
    for rep in range(reps + 2):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            out[name] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= 2:
                ts[name].append(dt)
    first = next(iter(out.values()))
    assert all(np.array_equal(first, p) for p in out.values())
    return {k: [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for k, v in ts.items()}, int(len(first))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--kernels", action="store_true", help="only the launches, for a kernel trace")
    ap.add_argument("--crossover", action="store_true", help="smaller scans: where the kernels overtake the CPU twin")
    a = ap.parse_args()
    shapes = CROSSOVER_SHAPES if a.crossover else ((64, 1800),)
    gpu = CvoGPU()
    if a.kernels:
        scan, cfg = scan_of(64, 1800)
        gpu.set_option("LIDAR_HOST", 0)
        for _ in range(5):
            gpu.lidar_select(scan, cfg, LidarRand(1))
        print(gpu.debug_lidar_stats(), flush=True)
        gpu.close()
        return
    os.makedirs(a.out, exist_ok=True)
    rows, lines = [], []
    for R, H in shapes:
        scan, cfg = scan_of(R, H)
        for stage, routes in stages(gpu, scan, cfg).items():
            ms, points = measure(routes, a.reps)
            rows.append({"n_scan": R, "horizon_scan": H, "scan_points": scan.n, "stage": stage, "selected": points, "ms": ms})
            line = (f"{R:3d} x {H:4d} ({scan.n:6d} points) {stage:6s} selected {points:6d} | ms "
                    + "  ".join(f"{k} {v[0]:.2f} [{v[1]:.2f}..{v[2]:.2f}]" for k, v in ms.items()))
            print(line, flush=True)
            lines.append(line)
    gpu.close()
    name = "crossover" if a.crossover else "lidar_probe"
    with open(os.path.join(a.out, name + ".json"), "w") as fo:
        json.dump({"reps": a.reps, "ms": "median [min, max] of a host clock around the call", "rows": rows}, fo, indent=1)
    with open(os.path.join(a.out, name + ".txt"), "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
