"""Times the semantic voxel map's SPARSE kernel (cvo_map_set_kernel, cvo_k_bki_sparse.h) on the device (BKI_HOST=0) against its
CPU twin on one thread, next to the counting insert of the same frames.  The workloads are scripts/bki_probe.py's - a 9 284-point
RGB-D-like cloud and a 16 686-point LiDAR-like cloud at resolution 0.05 and free_resolution 1 - with ell at 2 x and 4 x the
resolution.  For each: the first insert into a fresh map, the tenth into the grown map, the read-out.  Then a sweep of frame sizes
for the sparse crossover: the training points of a frame from which ten sparse inserts and a read-out take the device less time
than the twin.  Before anything is timed the device's table after two inserts is checked equal to the twin's, bit for bit.

    python scripts/bki_sparse_probe.py [--out profiles/bki_sparse/bki_sparse_probe.txt] [--json ...] [--profile]

--profile: one pass of both workloads on the device and nothing else, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python scripts/bki_sparse_probe.py --profile)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unified_cvo_amd as u  # noqa: E402
from unified_cvo_amd import CvoGPU  # noqa: E402
from bki_probe import frames, lidar_like, rgbd_like  # noqa: E402

RESOLUTION = 0.05


def life(open_map, kernel, fr):
    """ten inserts and a read-out -> dict of milliseconds and counts"""
    m = open_map()
    m.set_kernel(kernel)
    t = []
    for xyz, feat, label, origin in fr:
        t0 = time.perf_counter()
        m.insert((xyz, feat, label), origin=origin)
        t.append((time.perf_counter() - t0) * 1e3)
    stats = m.debug_stats()
    t0 = time.perf_counter()
    cloud = m.cloud()
    read = (time.perf_counter() - t0) * 1e3
    voxels, _ = m.size()
    m.close()
    return dict(first_ms=t[0], tenth_ms=t[-1], inserts_ms=sum(t), readout_ms=read, total_ms=sum(t) + read, training=stats["training"],
                members=stats["members"], longest_run=stats["longest_run"], voxels=voxels, occupied=len(cloud[0]), capacity=stats["capacity"],
                growths=stats["growths"], on_device=stats["on_device"])


def median_life(open_map, kernel, fr, repeats):
    runs = [life(open_map, kernel, fr) for _ in range(repeats)]
    out = dict(runs[0])
    for k in ("first_ms", "tenth_ms", "inserts_ms", "readout_ms", "total_ms"):
        out[k] = float(np.median([r[k] for r in runs]))
    return out


def check_equal(device, twin, fr):
    """two sparse inserts on either side: the tables equal bit for bit"""
    tables = []
    for opener in (device, twin):
        m = opener()
        m.set_kernel("sparse")
        for xyz, feat, label, origin in fr[:2]:
            m.insert((xyz, feat, label), origin=origin)
        s = m.debug_stats(readback=True)
        tables.append(s)
        m.close()
    a, b = tables
    assert a["on_device"] == 1 and b["on_device"] == 0
    for k in ("keys", "ms", "fs"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"the device's {k} differ from the twin's"
    return len(a["keys"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    gpu = CvoGPU()
    gpu.set_option("BKI_HOST", 0)
    workloads = {"rgbd_9284": frames(rgbd_like, 9284, 1), "lidar_16686": frames(lidar_like, 16686, 2)}
    configs = {f"ell{f}x": u.MapConfig(resolution=RESOLUTION, free_resolution=1.0, num_classes=19, sf2=1.0, ell=f * RESOLUTION) for f in (2, 4)}
    openers = {name: (lambda c=c: gpu.map_open(c), lambda c=c: u.map_open_host(c)) for name, c in configs.items()}
    device2, twin2 = openers["ell2x"]
    life(device2, "sparse", frames(rgbd_like, 2000, 3, count=2))  # (warm-up: the code objects, the first allocations)
    if args.profile:
        for fr in workloads.values():
            life(device2, "sparse", fr)
        return
    result = {"workloads": {}, "sweep": [], "checked_voxels": {}}

    class Lines(list):
        def append(self, line):  # (every line as it is measured: the twin's LiDAR lives take a minute each)
            print(line, flush=True)
            super().append(line)

    lines = Lines()
    for name, fr in workloads.items():
        result["checked_voxels"][name] = check_equal(device2, twin2, fr)
    lines.append("sparse kernel of the semantic voxel map: device (MI355X) against the CPU twin on one thread, milliseconds, medians of %d "
                 "lives of ten inserts; tables checked equal first (%s voxels)" % (args.repeats, result["checked_voxels"]))
    lines.append("workload      kernel        route   first    tenth   readout  ten+read  training/frame  members  longest  voxels   capacity growths")
    for name, fr in workloads.items():
        rows = [("sparse " + cname, "sparse", dev, tw) for cname, (dev, tw) in openers.items()] + [("counting", "csm", device2, twin2)]
        for label, kernel, dev, tw in rows:
            for route, opener in (("device", dev), ("twin", tw)):
                r = median_life(opener, kernel, fr, args.repeats if route == "device" else 1)
                assert r["on_device"] == (route == "device")
                result["workloads"][f"{name}/{label}/{route}"] = r
                lines.append(f"{name:13s} {label:13s} {route:6s} {r['first_ms']:8.2f} {r['tenth_ms']:8.2f} {r['readout_ms']:8.2f} {r['total_ms']:9.2f} "
                             f"{r['training']:10d} {r['members']:10d} {r['longest_run']:7d} {r['voxels']:9d} {r['capacity']:9d} {r['growths']:4d}")
    lines.append("")
    lines.append("sparse crossover sweep (RGB-D-like frames, ell 2 x resolution): hits  training/frame  device ten+read  twin ten+read")
    crossover = None
    for n in (8, 32, 128, 512, 2048):
        fr = frames(rgbd_like, n, 10 + n)
        d, t = median_life(device2, "sparse", fr, args.repeats), median_life(twin2, "sparse", fr, args.repeats)
        result["sweep"].append(dict(hits=n, training=d["training"], device_ms=d["total_ms"], twin_ms=t["total_ms"]))
        lines.append(f"  {n:6d} {d['training']:10d} {d['total_ms']:12.3f} {t['total_ms']:12.3f}")
        if crossover is None and d["total_ms"] < t["total_ms"]:
            crossover = d["training"]
        elif d["total_ms"] >= t["total_ms"]:
            crossover = None
    result["crossover_training"] = crossover
    lines.append(f"sparse crossover: {crossover} training points per frame (None: the device never stays ahead)")
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    if args.json:
        json.dump(result, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
