"""Times the semantic voxel map (cvo_map_*) on the device against its CPU twin on one thread - the same arithmetic; neither
upstream's OpenMP build nor PCL is measured.  Two workloads at resolution 0.05 and free_resolution 1: a 9 284-point RGB-D-like
cloud (the README's RGB-D figure) and a 16 686-point LiDAR-like cloud with 5 - 60 m rays.  For each: the first insert into a
fresh map, the tenth insert into the grown map (the sensor moves 0.1 m per frame), the read-out.  Then a sweep of cloud sizes
for the crossover: the training points of a frame from which ten inserts and a read-out take the device less time than the twin.

    python scripts/bki_probe.py [--out profiles/bki/bki_probe.txt] [--json ...] [--profile]

--profile: one pass of both workloads on the device and nothing else, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python scripts/bki_probe.py --profile)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import unified_cvo_amd as u  # noqa: E402
from unified_cvo_amd import CvoGPU  # noqa: E402

F32 = np.float32


def rgbd_like(rng, n):
    """points on surfaces 1 - 4 m in front of a camera with a 60 x 45 degree view"""
    z = rng.uniform(1.0, 4.0, n)
    return np.stack([z * np.tan(rng.uniform(-0.52, 0.52, n)), z * np.tan(rng.uniform(-0.39, 0.39, n)), z], 1).astype(F32)


def lidar_like(rng, n):
    """points 5 - 60 m around a spinning sensor, +-15 degrees of elevation"""
    r, az, el = rng.uniform(5.0, 60.0, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-0.26, 0.26, n)
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(F32)


def frames(make, n, seed, count=10, C=19):
    rng = np.random.default_rng(seed)
    out = []
    for f in range(count):
        origin = np.array([0.1 * f, 0.0, 0.0], F32)
        xyz = make(rng, n) + origin
        label = rng.uniform(0, 1, (n, C)).astype(F32)
        out.append((xyz, rng.uniform(0, 1, (n, 5)).astype(F32), label, origin))
    return out


def life(open_map, fr):
    """ten inserts and a read-out -> dict of milliseconds and counts"""
    m = open_map()
    t = []
    for xyz, feat, label, origin in fr:
        t0 = time.perf_counter()
        m.insert((xyz, feat, label), origin=origin)
        t.append((time.perf_counter() - t0) * 1e3)
    stats = m.debug_stats()
    t0 = time.perf_counter()
    cloud = m.cloud()
    read = (time.perf_counter() - t0) * 1e3
    voxels, occupied = m.size()
    m.close()
    return dict(first_ms=t[0], tenth_ms=t[-1], inserts_ms=sum(t), readout_ms=read, total_ms=sum(t) + read, training=stats["training"],
                members=stats["members"], voxels=voxels, occupied=len(cloud[0]), capacity=stats["capacity"], growths=stats["growths"],
                longest_probe=stats["longest_probe"], on_device=stats["on_device"])


def median_life(open_map, fr, repeats):
    runs = [life(open_map, fr) for _ in range(repeats)]
    out = dict(runs[0])
    for k in ("first_ms", "tenth_ms", "inserts_ms", "readout_ms", "total_ms"):
        out[k] = float(np.median([r[k] for r in runs]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    gpu = CvoGPU()
    gpu.set_option("BKI_HOST", 0)
    cfg = u.MapConfig(resolution=0.05, free_resolution=1.0, num_classes=19)
    device = lambda: gpu.map_open(cfg)  # noqa: E731
    twin = lambda: u.map_open_host(cfg)  # noqa: E731
    workloads = {"rgbd_9284": frames(rgbd_like, 9284, 1), "lidar_16686": frames(lidar_like, 16686, 2)}
    life(device, frames(rgbd_like, 2000, 3, count=2))  # (warm-up: the code objects, the first allocations)
    if args.profile:
        for fr in workloads.values():
            life(device, fr)
        return
    lines, result = [], {"workloads": {}, "sweep": []}
    lines.append("semantic voxel map: device (MI355X) against the CPU twin on one thread, milliseconds, medians of %d lives of ten inserts" % args.repeats)
    lines.append("workload         route   first    tenth   readout  ten+read  training/frame  voxels   occupied  capacity growths")
    for name, fr in workloads.items():
        for route, opener in (("device", device), ("twin", twin)):
            r = median_life(opener, fr, args.repeats)
            assert r["on_device"] == (route == "device")
            result["workloads"][f"{name}/{route}"] = r
            lines.append(f"{name:16s} {route:6s} {r['first_ms']:8.2f} {r['tenth_ms']:8.2f} {r['readout_ms']:8.2f} {r['total_ms']:9.2f} "
                         f"{r['training']:10d} {r['voxels']:12d} {r['occupied']:9d} {r['capacity']:9d} {r['growths']:4d}")
    lines.append("")
    lines.append("crossover sweep (RGB-D-like frames): hits  training/frame  device ten+read  twin ten+read")
    crossover = None
    for n in (8, 32, 128, 512, 2048, 9284):
        fr = frames(rgbd_like, n, 10 + n)
        d, t = median_life(device, fr, args.repeats), median_life(twin, fr, args.repeats)
        result["sweep"].append(dict(hits=n, training=d["training"], device_ms=d["total_ms"], twin_ms=t["total_ms"]))
        lines.append(f"  {n:6d} {d['training']:10d} {d['total_ms']:12.3f} {t['total_ms']:12.3f}")
        if crossover is None and d["total_ms"] < t["total_ms"]:
            crossover = d["training"]
        elif d["total_ms"] >= t["total_ms"]:
            crossover = None
    result["crossover_training"] = crossover
    lines.append(f"crossover: {crossover} training points per frame (None: the device never stays ahead)")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    if args.json:
        json.dump(result, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
