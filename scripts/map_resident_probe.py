"""Resident clouds into the semantic voxel map and out of it: what cvo_map_insert_cloud and cvo_map_cloud_resident cost next
to the routes a caller had before.

    python scripts/map_resident_probe.py [--out profiles/map_resident/map_resident_probe.txt] [--reps N]
    rocprofv3 --kernel-trace --stats -- python scripts/map_resident_probe.py --kernels     the new routes' launches alone

Workloads (scripts/bki_probe.py's): a 9 284-point RGB-D-like cloud and a 16 686-point LiDAR-like cloud with 5 - 60 m rays, 19
classes, resolution 0.05, free_resolution 1, ten frames, the sensor moving 0.1 m and turning 0.02 rad per frame.  The frames
are resident clouds before anything is timed (a front end or cvo_cloud_from_device made them).  Routes, alternated call by
call in ONE process, each on a map of its own, after the two maps and the two clouds have been checked equal:
  insert     (a) insert_cloud(cloud, pose)             (b) cloud.download(), then insert(rows, pose)       per frame
  read-out   (a) resident_cloud()                      (b) cloud(resident=True)                            of the ten-frame map
the read-out by default and under ORDER=wide.  Wall time is a host clock around a call that ends in a device
synchronisation: the first frame, and the median [min .. max] of frames 2 - 10 over --reps lives of a map; for the
read-out the median [min .. max] of --reps calls after three warm-up calls per route."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import unified_cvo_amd as u  # noqa: E402
from bki_probe import lidar_like, rgbd_like  # noqa: E402
from unified_cvo_amd import CvoGPU, CvoPointCloud  # noqa: E402

F32 = np.float32
WARM = 3
FRAMES = 10


def pose(f):
    a = 0.02 * f
    return np.array([[np.cos(a), -np.sin(a), 0, 0.1 * f], [np.sin(a), np.cos(a), 0, 0], [0, 0, 1, 0]], F32)


def frames(make, n, seed, C=19):
    rng = np.random.default_rng(seed)
    return [CvoPointCloud.from_arrays(make(rng, n), rng.uniform(0, 1, (n, 5)).astype(F32), rng.uniform(0, 1, (n, C)).astype(F32))
            for _ in range(FRAMES)]


def rows_of(cloud, C):
    d = cloud.download()
    return d.positions_, d.features_, d.labels_[:, :C]


def life(gpu, cfg, clouds):
    """ten frames into two maps, the routes alternated frame by frame -> (map a, map b, ms per frame of a, of b)"""
    a, b = gpu.map_open(cfg), gpu.map_open(cfg)
    ta, tb = [], []
    for f, c in enumerate(clouds):
        T = pose(f)
        t0 = time.perf_counter()
        a.insert_cloud(c, pose=T)
        ta.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        b.insert(rows_of(c, cfg.num_classes), pose=T)
        tb.append((time.perf_counter() - t0) * 1e3)
    return a, b, ta, tb


def same_tables(a, b):
    sa, sb = a.debug_stats(readback=True), b.debug_stats(readback=True)
    assert sa["on_device"] == sb["on_device"] == 1
    for k in ("keys", "ms", "fs"):
        assert sa[k].tobytes() == sb[k].tobytes(), k
    return sa


def same_clouds(x, y):
    dx, dy = x.download(), y.download()
    assert x.n == y.n and dx.present == dy.present and np.array_equal(x.debug_order(), y.debug_order())
    for k in ("positions_", "features_", "labels_"):
        assert getattr(dx, k).tobytes() == getattr(dy, k).tobytes(), k


def spread(v):
    return f"{np.median(v):8.3f} [{np.min(v):7.3f} .. {np.max(v):7.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_resident", "map_resident_probe.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels", action="store_true", help="one life of each workload on the new routes only, for a kernel trace")
    args = ap.parse_args()
    gpu = CvoGPU()
    gpu.set_option("BKI_HOST", 0)
    cfg = u.MapConfig(resolution=0.05, free_resolution=1.0, num_classes=19)
    lines = ["resident clouds into and out of the semantic voxel map (MI355X), milliseconds of wall time per call",
             f"insert: first frame (median of {args.reps} lives), frames 2-10 median [min .. max]; read-out: median [min .. max] of {args.reps * 4} calls", ""]
    for name, make, n, seed in (("rgbd_9284", rgbd_like, 9284, 1), ("lidar_16686", lidar_like, 16686, 2)):
        clouds = [gpu.upload(pc) for pc in frames(make, n, seed)]
        if args.kernels:
            m = gpu.map_open(cfg)
            for f, c in enumerate(clouds):
                m.insert_cloud(c, pose=pose(f))
            m.resident_cloud().free()
            m.close()
            continue
        a, b, _, _ = life(gpu, cfg, clouds)  # (warm-up, and the check that the routes agree)
        stats = same_tables(a, b)
        b.close()
        first, rest = {"a": [], "b": []}, {"a": [], "b": []}
        for _ in range(args.reps):
            x, y, ta, tb = life(gpu, cfg, clouds)
            x.close()
            y.close()
            for k, t in (("a", ta), ("b", tb)):
                first[k].append(t[0])
                rest[k] += t[1:]
        lines.append(f"{name}: {n} points per frame, {stats['training']} training points in the tenth frame, {stats['voxels']} voxels stored")
        lines.append(f"  insert   insert_cloud(cloud, pose)        first {np.median(first['a']):8.3f}   later {spread(rest['a'])}")
        lines.append(f"  insert   download + insert(rows, pose)    first {np.median(first['b']):8.3f}   later {spread(rest['b'])}")
        for order in (None, "wide"):
            gpu.set_option("ORDER", order)
            new, old = a.resident_cloud(), a.cloud(resident=True)[3]
            same_clouds(new, old)
            occupied, route = new.n, new.debug_order_route()
            new.free()
            old.free()
            ts = {"new": [], "old": []}
            for rep in range(args.reps * 4 + WARM):
                for key, fn in (("new", a.resident_cloud), ("old", lambda: a.cloud(resident=True)[3])):
                    t0 = time.perf_counter()
                    c = fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    c.free()
                    if rep >= WARM:
                        ts[key].append(dt)
            tag = f"{occupied} occupied voxels, ORDER={'wide' if order else 'default'} (ordered by route {route})"
            lines.append(f"  read-out resident_cloud()                 {spread(ts['new'])}   {tag}")
            lines.append(f"  read-out cloud(resident=True)             {spread(ts['old'])}")
        gpu.set_option("ORDER", None)
        a.close()
        for c in clouds:
            c.free()
        lines.append("")
    gpu.close()
    if args.kernels:
        return
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
