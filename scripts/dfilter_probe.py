"""The disparity post-filter (cvo_disparity_filter: libelas's speckle, gap and adaptive-mean passes): what a map costs on the
kernels and on the CPU twin, and what the filter adds to the matcher.

  python scripts/dfilter_probe.py [--out DIR] [--reps N]      wall times at 1241 x 376 and 640 x 480, DIR/dfilter_probe.{json,txt}
  python scripts/dfilter_probe.py --crossover                 small maps (the DFILTER_HOST default), DIR/crossover.{json,txt}
  rocprofv3 --kernel-trace --stats -d DIR/trace -o dfilter --output-format csv -- python scripts/dfilter_probe.py --kernels
                                                              the launches a profiler should see, nothing else

Maps: the matcher's own (stereo_disparity, D = 128, 8 paths, on the device) of the two-plane pair of tests/sgm_cases.py, so
the filter sees the speckles and pin-holes it exists for; the crossover's small maps are top-left crops of the 480 x 640 one.
Routes, alternated call by call in ONE process (other work shares the machine):
  device  DFILTER_HOST=0: upload, the speckle pass's four launches, the gap pass's two, the mean's two, one download with the
          counters, one synchronisation;
  twin    DFILTER_HOST=1: the same call on one CPU thread;
and for the matcher: stereo_disparity (the call the parent commit has, its kernels untouched), stereo_disparity with the filter
(the map stays on the device in between), and the unfiltered call followed by disparity_filter (a download and an upload more).
Wall time is a host clock around the call, which returns after the upload stream has been synchronised: the median and the
spread of --reps calls after two warm-up calls.  The routes' maps are compared.  A size where the device loses is reported
like any other."""
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
from unified_cvo_amd import CvoGPU, DFilterConfig, SGMConfig  # noqa: E402

FRAMES = ((376, 1241), (480, 640))
CROSSOVER = ((4, 8), (8, 16), (16, 32), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (480, 640))


def with_host(gpu, route, fn):
    def run():
        gpu.set_option("DFILTER_HOST", route)
        try:
            return fn()
        finally:
            gpu.set_option("DFILTER_HOST", None)
    return run


def measure(fns, reps, same=True):
    """fns: name -> call.  Routes alternate call by call."""
    ts, out = {k: [] for k in fns}, {}
    for rep in range(reps + 2):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            out[name] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= 2:
                ts[name].append(dt)
    if same:
        first = next(iter(out.values()))
        assert all(np.array_equal(first.view(np.uint32), p.view(np.uint32)) for p in out.values())
    return {k: [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3), len(v)] for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dfilter"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--kernels", action="store_true", help="only the launches, for a kernel trace")
    ap.add_argument("--crossover", action="store_true", help="small maps: where the kernels overtake the CPU twin")
    a = ap.parse_args()
    gpu = CvoGPU()
    gpu.set_option("SGM_HOST", 0)
    if a.kernels:
        gpu.set_option("DFILTER_HOST", 0)
        for rows, cols in FRAMES:
            left, right, _ = sc.two_planes(rows, cols)
            raw = gpu.stereo_disparity(left, right)
            for _ in range(5):
                gpu.disparity_filter(raw)
            print(gpu.debug_dfilter_stats(), flush=True)
        gpu.close()
        return
    os.makedirs(a.out, exist_ok=True)
    rows_out, lines = [], []

    def report(rows, cols, what, ms, note=""):
        rows_out.append({"rows": rows, "cols": cols, "pixels": rows * cols, "what": what, "ms": ms, "note": note})
        line = (f"{cols:4d} x {rows:3d} ({rows * cols:6d} pixels) {what:<18} | ms "
                + "  ".join(f"{k} {v[0]:.3f} [{v[1]:.3f}..{v[2]:.3f}] n={v[3]}" for k, v in ms.items()) + (f" | {note}" if note else ""))
        print(line, flush=True)
        lines.append(line)

    if a.crossover:
        left, right, _ = sc.two_planes(480, 640)
        big = gpu.stereo_disparity(left, right)
        for rows, cols in CROSSOVER:
            raw = np.ascontiguousarray(big[:rows, 40:40 + cols] if cols <= 600 else big[:rows, :cols])
            call = lambda: gpu.disparity_filter(raw)
            report(rows, cols, "filter", measure({"device": with_host(gpu, 0, call), "twin": with_host(gpu, 1, call)}, a.reps))
    else:
        for rows, cols in FRAMES:
            left, right, truth = sc.two_planes(rows, cols)
            raw = gpu.stereo_disparity(left, right)
            call = lambda: gpu.disparity_filter(raw)
            ms = measure({"device": with_host(gpu, 0, call), "twin": with_host(gpu, 1, call)}, a.reps)
            gpu.set_option("DFILTER_HOST", 0)
            out = gpu.disparity_filter(raw)
            st = gpu.debug_dfilter_stats()
            gpu.set_option("DFILTER_HOST", None)
            share = lambda m: float((np.abs(m[m >= 0] - truth[m >= 0]) > 1).mean())
            note = (f"segments {st['segments']} removed {st['removed']} filled {st['filled']}; valid {int((raw >= 0).sum())} -> {int((out >= 0).sum())}, "
                    f"more than 1 from the truth {100 * share(raw):.2f} % -> {100 * share(out):.2f} %")
            report(rows, cols, "filter", ms, note)
            dcfg = DFilterConfig()
            gpu.set_option("DFILTER_HOST", 0)
            report(rows, cols, "matcher, D 128", measure({"stereo_disparity": lambda: gpu.stereo_disparity(left, right),
                                                          "with dfilter": lambda: gpu.stereo_disparity(left, right, SGMConfig(), dfilter=dcfg),
                                                          "then disparity_filter": lambda: gpu.disparity_filter(gpu.stereo_disparity(left, right), dcfg)},
                                                         a.reps, same=False))
            gpu.set_option("DFILTER_HOST", None)
    gpu.close()
    name = "crossover" if a.crossover else "dfilter_probe"
    with open(os.path.join(a.out, name + ".json"), "w") as fo:
        json.dump({"reps": a.reps, "ms": "median [min, max, calls] of a host clock around the call", "rows": rows_out}, fo, indent=1)
    with open(os.path.join(a.out, name + ".txt"), "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
