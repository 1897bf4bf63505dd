"""Posed resident clouds merged on the device: what cvo_cloud_merge costs next to the route a caller had before.

  python scripts/merge_probe.py [--out DIR] [--reps N]      wall times, written to DIR/merge_probe.{json,txt}
  rocprofv3 --kernel-trace --stats -d DIR/trace -o merge --output-format csv -- python scripts/merge_probe.py --kernels
                                                             the launches a profiler should see, nothing else

Shapes: 8 frames of 10 000 colour points, and 16 frames of 21 429 points with colour and one-hot labels; every frame under a
rigid pose of its own; leaves 0.05 and 0.1.  Routes, alternated call by call in ONE process:
  (a) merge        CvoGPU.merge_clouds of the resident frames
  (b) host route   what a caller had before: a host copy of every frame at hand, moved in numpy with the pose's float
                   arithmetic (fma(T0, x, T1 y) + fma(T2, z, T3) rounded as the device rounds it), concatenated, upload_voxel
The two results are checked equal first (kept indices, spatial order, downloaded rows).  Wall time is a host clock around a
call that ends in a device synchronisation; the median, minimum and maximum of --reps calls after three warm-up calls per
route.
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

from unified_cvo_amd import CvoGPU, synth  # noqa: E402

WARM = 3
SHAPES = (("8 x 10000 colour", 8, 10000, False), ("16 x 21429 colour+labels", 16, 21429, True))
LEAVES = (0.05, 0.1)


def fptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def frame(n, k, labels):
    src, fsrc, lsrc = synth.semantic_pair(n, k)[:3]
    return [np.ascontiguousarray(src, np.float32), np.ascontiguousarray(fsrc, np.float32),
            np.ascontiguousarray(lsrc, np.float32) if labels else None, None]


def pose(rs):
    w = rs.normal(size=3)
    w *= rs.uniform(0.02, 0.2) / np.linalg.norm(w)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    return np.concatenate([R, rs.uniform(-0.5, 0.5, (3, 1))], axis=1).reshape(12)


def move(pose12, xyz):
    T = np.asarray(pose12, np.float64).astype(np.float32).reshape(3, 4)
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    out = np.empty_like(xyz)
    for r in range(3):
        p1 = (T[r, 1] * xyz[:, 1]).astype(np.float64)
        out[:, r] = (np.float64(T[r, 0]) * x + p1).astype(np.float32) + (np.float64(T[r, 2]) * z + np.float64(T[r, 3])).astype(np.float32)
    return out


def upload(gpu, arrs):
    h = C.c_void_p()
    gpu._check(gpu.L.cvo_cloud_upload(gpu.ctx, arrs[0].shape[0], *[fptr(a) for a in arrs], C.byref(h)))
    return gpu._adopt(h, arrs[0].shape[0])


def host_route(gpu, frames, poses, leaf):
    xyz = np.concatenate([move(p, f[0]) for p, f in zip(poses, frames)])
    cols = [np.concatenate([f[k] for f in frames]) if frames[0][k] is not None else None for k in (1, 2, 3)]
    n = xyz.shape[0]
    kept, nk, h = np.zeros(n, np.int32), C.c_int(), C.c_void_p()
    gpu._check(gpu.L.cvo_cloud_upload_voxel(gpu.ctx, n, fptr(xyz), *[fptr(a) for a in cols], float(leaf), C.byref(h),
                                            kept.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nk)))
    c = gpu._adopt(h, nk.value)
    c.kept = kept[:nk.value]
    return c


def stat(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernels", action="store_true", help="only the merge launches, for a kernel trace")
    a = ap.parse_args()
    gpu = CvoGPU()
    rs = np.random.default_rng(1)
    rows, lines = [], []
    for name, F, n, labels in SHAPES:
        frames = [frame(n, k, labels) for k in range(F)]
        poses = np.stack([pose(rs) for _ in range(F)])
        clouds = [upload(gpu, f) for f in frames]
        for leaf in LEAVES:
            if a.kernels:
                for _ in range(5):
                    gpu.merge_clouds(clouds, poses, leaf).free()
                continue
            m, kept = gpu.merge_clouds(clouds, poses, leaf, return_kept=True)
            h = host_route(gpu, frames, poses, leaf)
            assert np.array_equal(kept, h.kept) and np.array_equal(m.debug_order(), h.debug_order()), (name, leaf)
            dm, dh = m.download(), h.download()
            assert dm.positions_.tobytes() == dh.positions_.tobytes() and dm.features_.tobytes() == dh.features_.tobytes(), (name, leaf)
            assert dm.labels_.tobytes() == dh.labels_.tobytes() and dm.present == dh.present
            n_kept = m.n
            m.free()
            h.free()
            routes = {"merge": lambda: gpu.merge_clouds(clouds, poses, leaf), "host route": lambda: host_route(gpu, frames, poses, leaf)}
            ts = {k: [] for k in routes}
            for rep in range(a.reps + WARM):
                for key, fn in routes.items():
                    t0 = time.perf_counter()
                    out = fn()
                    dt = (time.perf_counter() - t0) * 1e3
                    out.free()
                    if rep >= WARM:
                        ts[key].append(dt)
            row = {"case": name, "leaf": leaf, "rows": F * n, "kept": n_kept, "ms": {k: stat(v) for k, v in ts.items()}}
            rows.append(row)
            line = f"{name:26s} leaf {leaf:<5} kept {n_kept:7d}  " + "  ".join(
                f"{k} {v[0]:.3f} ms [{v[1]:.3f}..{v[2]:.3f}]" for k, v in row["ms"].items())
            print(line, flush=True)
            lines.append(line)
        for c in clouds:
            c.free()
    gpu.close()
    if a.kernels:
        return
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "merge_probe.json"), "w") as f:
        json.dump({"reps": a.reps, "warm_up": WARM, "ms": "median [min, max] of a host clock around the call", "rows": rows}, f, indent=1)
    with open(os.path.join(a.out, "merge_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
