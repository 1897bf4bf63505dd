"""Times the read side of the semantic voxel map (cvo_map_query / _query_cloud / _raycast / _render, cvo_k_bki_query.h) on the
device (BKI_HOST=0) against its CPU twin on one thread.  The maps are README's two ten-frame maps - scripts/bki_probe.py's
9 284-point RGB-D-like and 16 686-point LiDAR-like frames at resolution 0.05, free_resolution 1 - under the counting kernel and
under the sparse one (ell 2 x resolution).  Per map:
  query      9 284 and 16 686 points (hits of the frames, a tenth of them moved off the map) from host rows, and the same points
             as a resident cloud under a pose; the resident query also against the only route a caller had before -
             cvo_map_cloud of the whole map, then a host dictionary lookup of the points' keys
  raycast    16 686 segments of 5 - 60 m from the last origin in random directions, stopping at OCCUPIED
  render     640 x 480, fx = fy = 525, z_far 10 m, from the last origin (the RGB-D-like map along the frames' own view, the LiDAR-like one along x)
What a time includes: the whole call as a caller sees it - the upload of points or rays, the launch, the copy of every output
array back, the synchronisation; the wrapper's allocation of the numpy outputs too (both routes pay it).  Not included: building
the maps, uploading the resident cloud.  Every result is first checked equal, byte for byte, between the two routes; then the
routes alternate, one warm-up call each, medians of --repeats device calls and --twin-repeats twin calls.

    python scripts/map_query_probe.py [--out profiles/map_query/map_query_probe.txt] [--json ...] [--profile]

--profile: the device calls of every map once and nothing else, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python scripts/map_query_probe.py --profile)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unified_cvo_amd as u  # noqa: E402
from unified_cvo_amd import CvoGPU, CvoPointCloud  # noqa: E402
from bki_probe import frames, lidar_like, rgbd_like  # noqa: E402

RESOLUTION = 0.05
F32 = np.float32
VIEW = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, rows=480, cols=640, z_far=10.0)


def filled(opener, kernel, fr):
    m = opener()
    m.set_kernel(kernel)
    for xyz, feat, label, origin in fr:
        m.insert((xyz, feat, label), origin=origin)
    return m


def timed(fn, repeats):
    fn()  # (warm-up)
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def same(a, b, what):
    for name, x, y in zip(a._fields, a, b):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), f"{what}: the device's {name} differs from the twin's"


def key_of(xyz):
    q = xyz.astype(np.float64) / np.float64(F32(RESOLUTION)) + 524288.5
    ok = np.isfinite(q).all(axis=1) & (q >= 1).all(axis=1) & (q < 1048575).all(axis=1)
    k = np.where(ok[:, None], q, 0).astype(np.int64)
    return ok, (k[:, 0] << 40) | (k[:, 1] << 20) | k[:, 2]


def old_route(m, pts):
    """what a caller did before: the whole map's OCCUPIED cloud down, a dictionary of its keys, a lookup per point"""
    xyz, _, label = m.cloud()
    _, keys = key_of(xyz)
    table = dict(zip(keys.tolist(), range(len(keys))))
    ok, want = key_of(pts)
    return np.array([table.get(k, -1) if o else -1 for k, o in zip(want.tolist(), ok)]), label


def look_from(origin, along_x):
    """the camera at `origin`: the RGB-D-like frames already look along the map's z; the LiDAR-like map is seen along its x"""
    R = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]] if along_x else [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    return np.concatenate([np.array(R, F32), np.asarray(origin, F32).reshape(3, 1)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--twin-repeats", type=int, default=1)
    args = ap.parse_args()
    gpu = CvoGPU()
    gpu.set_option("BKI_HOST", 0)
    cfg = u.MapConfig(resolution=RESOLUTION, free_resolution=1.0, num_classes=19, sf2=1.0, ell=2 * RESOLUTION)
    workloads = {"rgbd_9284": frames(rgbd_like, 9284, 1), "lidar_16686": frames(lidar_like, 16686, 2)}
    pose = np.array([[np.cos(0.01), -np.sin(0.01), 0, 0.02], [np.sin(0.01), np.cos(0.01), 0, -0.01], [0, 0, 1, 0.005]], F32)
    result, lines = {}, []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say("read side of the semantic voxel map: device (MI355X) against the CPU twin on one thread; milliseconds per call (upload, launch, every "
        "output copied back), medians of %d device and %d twin calls behind one warm-up; results checked equal first" % (args.repeats, args.twin_repeats))
    say("map                      call                 n        device ms   twin ms   device ns/item  twin ns/item   other")
    for wname, fr in workloads.items():
        for kernel in ("csm", "sparse"):
            name = f"{wname}/{kernel}"
            dev = filled(lambda: gpu.map_open(cfg), kernel, fr)
            assert dev.debug_stats()["on_device"] == 1
            rng = np.random.default_rng(7)
            hits = np.concatenate([f[0] for f in fr[-2:]])
            origin = fr[-1][3]
            d = rng.normal(size=(16686, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            ends = (origin + d * rng.uniform(5, 60, (16686, 1))).astype(F32)
            T = look_from(origin, wname.startswith("lidar"))
            sets = {}
            for n in (9284, 16686):
                pts = hits[rng.permutation(len(hits))[:n]].copy()
                pts[::10] += F32(3.0)
                sets[n] = (pts, gpu.upload(CvoPointCloud.from_arrays(pts)))
            if args.profile:
                for pts, cloud in sets.values():
                    dev.query(pts)
                    dev.query(cloud, pose=pose)
                dev.raycast(origin, ends)
                dev.render(T, **VIEW)
                dev.close()
                continue
            twin = filled(lambda: u.map_open_host(cfg), kernel, fr)
            voxels = dev.size()[0]
            calls = []
            for n, (pts, cloud) in sets.items():
                moved = dev.query(cloud, pose=pose)
                same(dev.query(pts), twin.query(pts), f"{name} query {n}")
                calls.append((f"query host rows", n, lambda p=pts: dev.query(p), lambda p=pts: twin.query(p), ""))
                t_old = timed(lambda p=pts: old_route(dev, p), 1)
                calls.append((f"query resident cloud", n, lambda c=cloud: dev.query(c, pose=pose), None, f"old route (cvo_map_cloud + dictionary) {t_old:.1f} ms"))
                assert (moved.found <= 2).all()
            same(dev.raycast(origin, ends), twin.raycast(origin, ends), f"{name} raycast")
            calls.append(("raycast 5-60 m", 16686, lambda: dev.raycast(origin, ends), lambda: twin.raycast(origin, ends), ""))
            a, b = dev.render(T, **VIEW), twin.render(T, **VIEW)
            same(a, b, f"{name} render")
            steps = int(dev.raycast(origin, ends, stop=0).steps.sum())
            calls.append(("render 640x480", 640 * 480, lambda: dev.render(T, **VIEW), lambda: twin.render(T, **VIEW),
                          f"{float((a.depth > 0).mean()) * 100:.0f} % of the pixels stop; the 16 686 rays cross {steps} voxels unstopped"))
            for what, n, on_dev, on_twin, other in calls:
                td = timed(on_dev, args.repeats)  # (the routes alternate: device, twin, device ...)
                tt = timed(on_twin, args.twin_repeats) if on_twin else float("nan")
                result[f"{name}/{what}/{n}"] = dict(n=n, device_ms=td, twin_ms=tt, voxels=voxels, other=other)
                say(f"{name:24s} {what:20s} {n:7d} {td:10.3f} {tt:10.3f} {td * 1e6 / n:12.1f} {tt * 1e6 / n:12.1f}   {other}")
            for _, cloud in sets.values():
                cloud.free()
            say(f"{name:24s} voxels {voxels}")
            dev.close()
            twin.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    if args.json:
        json.dump(result, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
