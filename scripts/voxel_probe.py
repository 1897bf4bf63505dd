"""Voxel-grid downsampling: what a raw frame costs on its way to a resident cloud.

  python scripts/voxel_probe.py [--out DIR] [--reps N]     wall times, written to DIR/voxel_probe.{json,txt}
  rocprofv3 --kernel-trace --stats -d DIR/trace -o voxel --output-format csv -- python scripts/voxel_probe.py --kernels
                                                            the launches a profiler should see, nothing else
  python scripts/voxel_probe.py --trace-summary DIR/trace/voxel_kernel_trace.csv     (any machine) that trace per frame,
                                                            leaf size and form of k_voxel_insert

Frames: the street scene of synth.scene_pair at 307 200 (an RGB-D frame) and 1 000 000 points, shuffled (as synth
makes it) and in scan order (tests/np_voxel.scan_order: image rows, then columns), xyz only and with colour, leaf sizes
0.1 and 0.25.  Routes, alternated call by call in ONE process: the kernels with the block-local pre-pass
(VOXEL_PREPASS=1), without it (=0), and the CPU twin (VOXEL_HOST=1) - the route a caller had before.  Wall time is a host clock
around upload_voxel, which returns after the stream has been synchronised; the median and the spread of --reps calls
after two warm-up calls per route.  voxel_select alone (coordinates up, indices back) is timed the same way.
--kernels runs every (frame, leaf, pre-pass) once more than it warms up, so that the per-kernel statistics of the trace
(k_voxel_insert<true> / <false>, k_compact_count<VoxelFirst>, k_voxel_scan, k_compact_write<VoxelFirst>) average over equal
numbers of both forms.
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

import np_voxel  # noqa: E402
from unified_cvo_amd import CvoGPU, CvoPointCloud, synth  # noqa: E402

ROUTES = (("prepass", {"VOXEL_HOST": 0, "VOXEL_PREPASS": 1}), ("plain", {"VOXEL_HOST": 0, "VOXEL_PREPASS": 0}),
          ("host", {"VOXEL_HOST": 1, "VOXEL_PREPASS": None}))


def frames(sizes):
    for n in sizes:
        x = synth.scene_pair(n)[0]
        for order, xyz in (("shuffled", x), ("scan", np_voxel.scan_order(x))):
            yield n, order, xyz


def set_route(gpu, switches):
    for k, v in switches.items():
        gpu.set_option(k, v)


def wall(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def trace_summary(path, sizes):
    """Per (frame, leaf, route) of a --kernels run: the five k_voxel_insert launches and the mean of the three small
    kernels, in microseconds, in launch order (the order --kernels issues them in)."""
    import csv
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    names = {"insert": "k_voxel_insert", "count": "k_compact_count", "scan": "k_voxel_scan", "write": "k_compact_write"}
    by = {k: [us(r) for r in rows if name in r["Kernel_Name"]] for k, name in names.items()}
    forms = ["<true>" in r["Kernel_Name"] for r in rows if "k_voxel_insert" in r["Kernel_Name"]]
    i = 0
    for n in sizes:
        for order in ("shuffled", "scan"):
            for s in (0.1, 0.25):
                for name, _ in ROUTES[:2]:
                    sl = slice(5 * i, 5 * i + 5)
                    assert all(f == (name == "prepass") for f in forms[sl]), "not a --kernels trace of these sizes"
                    rest = sum(sum(by[k][sl]) / 5 for k in ("count", "scan", "write"))
                    print(f"{n:8d} {order:8s} leaf {s:<4} {name:8s} k_voxel_insert us " + " ".join(f"{v:6.1f}" for v in by["insert"][sl])
                          + f" | count + scan + write {rest:5.1f}")
                    i += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", type=int, nargs="+", default=[307200, 1000000])
    ap.add_argument("--kernels", action="store_true", help="only the launches, for a kernel trace")
    ap.add_argument("--trace-summary", metavar="CSV", help="summarise the kernel trace of a --kernels run; no GPU needed")
    a = ap.parse_args()
    if a.trace_summary:
        trace_summary(a.trace_summary, a.sizes)
        return
    gpu = CvoGPU()
    if a.kernels:
        for n, order, xyz in frames(a.sizes):
            for s in (0.1, 0.25):
                for name, sw in ROUTES[:2]:
                    set_route(gpu, sw)
                    for _ in range(5):
                        gpu.voxel_select(xyz, s)
                    print(f"{n} {order} {s} {name}: {gpu.debug_voxel_stats()}", flush=True)
        gpu.close()
        return
    os.makedirs(a.out, exist_ok=True)
    rows, lines = [], []
    for n, order, xyz in frames(a.sizes):
        rng = np.random.default_rng(1)
        clouds = {"xyz": CvoPointCloud.from_xyz(xyz),
                  "colour": CvoPointCloud.from_arrays(xyz, synth.colour_features(xyz, rng).astype(np.float32), None,
                                                      np.tile(np.array([[0.0, 1.0]], np.float32), (n, 1)))}
        for s in (0.1, 0.25):
            want = np_voxel.reference(xyz, s)
            # alternate the routes call by call: other work shares the machine
            sel = {name: [] for name, _ in ROUTES}
            up = {(name, kind): [] for name, _ in ROUTES for kind in clouds}
            stats = {}
            for rep in range(a.reps + 2):
                for name, sw in ROUTES:
                    set_route(gpu, sw)
                    t0 = time.perf_counter()
                    kept = gpu.voxel_select(xyz, s)
                    dt = (time.perf_counter() - t0) * 1e3
                    assert np.array_equal(kept, want), (n, order, s, name)
                    if name != "host":
                        stats[name] = gpu.debug_voxel_stats()
                    if rep >= 2:
                        sel[name].append(dt)
                    for kind, pc in clouds.items():
                        t0 = time.perf_counter()
                        d = gpu.upload_voxel(pc, s)
                        dt = (time.perf_counter() - t0) * 1e3
                        d.free()
                        if rep >= 2:
                            up[(name, kind)].append(dt)
            # the ordinary upload of the kept rows alone (what follows the selection on every route)
            sub = clouds["colour"].select(want)
            plain_up = wall(lambda: gpu.upload(sub).free(), a.reps)
            row = {"points": n, "order": order, "leaf": s, "kept": int(want.shape[0]),
                   "entered_prepass": stats["prepass"]["entered"], "probes_plain": stats["plain"]["probes_total"],
                   "longest_probe": stats["plain"]["probe_longest"],
                   "select_ms": {k: [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for k, v in sel.items()},
                   "upload_voxel_ms": {f"{k[0]}/{k[1]}": [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)]
                                       for k, v in up.items()},
                   "upload_kept_rows_colour_ms": round(float(np.median(plain_up)), 3)}
            rows.append(row)
            line = (f"{n:8d} {order:8s} leaf {s:<4} kept {row['kept']:7d} entered(prepass) {row['entered_prepass']:7d} | select ms "
                    + "  ".join(f"{k} {v[0]:.2f} [{v[1]:.2f}..{v[2]:.2f}]" for k, v in row["select_ms"].items())
                    + " | upload_voxel ms " + "  ".join(f"{k} {v[0]:.2f}" for k, v in row["upload_voxel_ms"].items()))
            print(line, flush=True)
            lines.append(line)
    gpu.close()
    with open(os.path.join(a.out, "voxel_probe.json"), "w") as f:
        json.dump({"reps": a.reps, "ms": "median [min, max] of a host clock around the call", "rows": rows}, f, indent=1)
    with open(os.path.join(a.out, "voxel_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
