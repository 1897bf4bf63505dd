"""Keyframe depth filtering on the device: what cvo_depth_filter costs next to the route a caller had before it.

  python scripts/depthfilter_probe.py [--out DIR] [--reps N]     wall times, written to DIR/depthfilter_probe.{json,txt}
  rocprofv3 --kernel-trace --stats -d DIR/trace -o depth --output-format csv -- python scripts/depthfilter_probe.py --kernels
                                                                  the launches a profiler should see, nothing else

Shapes: a keyframe of 9 284 points (the size of the RGB-D recipe's cloud in the README) against 4 and 8 frames of 21 429 and
of 307 200 points, geometry only, every frame under matrices of its own; the driver's kernel diag(n, n, d), d >> n; the
default nearest_neighbors_max.  Routes, alternated call by call in ONE process:
  (a) device       open, add for every frame, finish (CvoGPU.depth_filter_open ...), timed whole and per stage
  (b) host route   what a caller had before, per frame: compute_association_gpu_non_isotropic to a host CSR, download of the
                   frame, the twin's arithmetic on one thread (depth_filter_accumulate_host); then depth_filter_finish_host and
                   cvo_cloud_upload of the kept rows
The two results are checked equal first (kept indices, depths, downloaded rows, spatial order).  Wall time is a host clock
around calls that end in a device synchronisation; the median, minimum and maximum of --reps rounds after two warm-up rounds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from unified_cvo_amd import (CvoGPU, CvoPointCloud, depth_filter_accumulate_host, depth_filter_finish_host,  # noqa: E402
                             synth)

WARM = 2
KF = 9284
SHAPES = ((4, 21429), (8, 21429), (4, 307200), (8, 307200))
KERNEL = np.diag([0.01, 0.01, 0.25]).astype(np.float32)  # (two to three associated points per row and frame at these densities)


def rigid(rs, scale):
    w = rs.normal(size=3)
    w *= scale * rs.uniform(0.2, 1.0) / np.linalg.norm(w)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = rs.uniform(-1, 1, 3) * scale
    return T.astype(np.float32)


def stat(v):
    return [round(float(np.median(v)), 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)]


def device_route(gpu, kf, frames, Ts, Tds, stages=None):
    t0 = time.perf_counter()
    df = gpu.depth_filter_open(kf)
    t1 = time.perf_counter()
    for f, T, Td in zip(frames, Ts, Tds):
        df.add(f, T, KERNEL, Td)
    t2 = time.perf_counter()
    out = df.finish(return_kept=True)
    t3 = time.perf_counter()
    df.close()
    if stages is not None:
        stages["open"].append((t1 - t0) * 1e3)
        stages["adds (association + k_depth_accumulate)"].append((t2 - t1) * 1e3)
        stages["finish + ingest"].append((t3 - t2) * 1e3)
    return out


def host_route(gpu, kf, kf_xyz, frames, Ts, Tds, stages=None):
    state = None
    ta = td = tt = 0.0
    for f, T, Td in zip(frames, Ts, Tds):
        t0 = time.perf_counter()
        rp, col, val = gpu.compute_association_gpu_non_isotropic(kf, f, T, KERNEL)
        t1 = time.perf_counter()
        y = f.download().positions()
        t2 = time.perf_counter()
        state = depth_filter_accumulate_host(rp, col, val, y, Td, state)
        t3 = time.perf_counter()
        ta, td, tt = ta + t1 - t0, td + t2 - t1, tt + t3 - t2
    if stages is not None:
        stages["entries"] = int(state[2].sum())
    t0 = time.perf_counter()
    xyz, kept, depth, nf = depth_filter_finish_host(kf_xyz, state)
    t1 = time.perf_counter()
    out = gpu.upload(CvoPointCloud.from_xyz(xyz))
    t2 = time.perf_counter()
    if stages is not None:
        for k, v in (("association to a host CSR", ta), ("download of the frames", td), ("twin accumulate", tt + t1 - t0), ("upload", t2 - t1)):
            stages[k].append(v * 1e3)
    return out, kept, depth, nf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_filter"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernels", action="store_true", help="only the device route's launches, for a kernel trace")
    a = ap.parse_args()
    gpu = CvoGPU()
    rs = np.random.default_rng(3)
    rows, lines = [], []
    for F, m in SHAPES:
        src, tgt, _ = synth.geometric_pair(KF, 0, m=m)
        kf_xyz = np.ascontiguousarray(src, np.float32)
        kf = gpu.upload(CvoPointCloud.from_xyz(kf_xyz))
        frames, Ts, Tds = [], [], []
        for k in range(F):
            shift = rs.normal(0.0, 0.01, tgt.shape).astype(np.float32)
            frames.append(gpu.upload(CvoPointCloud.from_xyz(tgt + shift)))
            Ts.append((synth.gt_motion() @ rigid(rs, 0.003)).astype(np.float32))
            Tds.append(rigid(rs, 0.05))
        if a.kernels:
            for _ in range(3):
                device_route(gpu, kf, frames, Ts, Tds)[0].free()
            continue
        d, dk, dd, dn = device_route(gpu, kf, frames, Ts, Tds)
        h, hk, hd, hn = host_route(gpu, kf, kf_xyz, frames, Ts, Tds)
        assert np.array_equal(dk, hk) and dd.tobytes() == hd.tobytes() and dn == hn, (F, m)
        assert np.array_equal(d.debug_order(), h.debug_order()) and d.download().positions_.tobytes() == h.download().positions_.tobytes()
        n_kept = d.n
        d.free()
        h.free()
        ts = {"device": [], "host route": []}
        st_d = {k: [] for k in ("open", "adds (association + k_depth_accumulate)", "finish + ingest")}
        st_h = {k: [] for k in ("association to a host CSR", "download of the frames", "twin accumulate", "upload")}
        for rep in range(a.reps + WARM):
            keep = rep >= WARM
            t0 = time.perf_counter()
            out = device_route(gpu, kf, frames, Ts, Tds, st_d if keep else None)
            t1 = time.perf_counter()
            out[0].free()
            t2 = time.perf_counter()
            out = host_route(gpu, kf, kf_xyz, frames, Ts, Tds, st_h if keep else None)
            t3 = time.perf_counter()
            out[0].free()
            if keep:
                ts["device"].append((t1 - t0) * 1e3)
                ts["host route"].append((t3 - t2) * 1e3)
        entries = st_h.pop("entries")
        row = {"frames": F, "frame_points": m, "keyframe_points": KF, "kept": n_kept, "nearest_neighbors_max": gpu.params.nearest_neighbors_max,
               "entries_per_row_and_frame": round(entries / (KF * F), 2),
               "ms": {k: stat(v) for k, v in ts.items()}, "device_stages_ms": {k: stat(v) for k, v in st_d.items()},
               "host_stages_ms": {k: stat(v) for k, v in st_h.items()}}
        rows.append(row)
        line = f"{F} x {m:6d}  kept {n_kept:5d}  {row['entries_per_row_and_frame']:.2f} entries per row and frame  " + "  ".join(f"{k} {v[0]:.2f} ms [{v[1]:.2f}..{v[2]:.2f}]" for k, v in row["ms"].items())
        line += "\n    device: " + ", ".join(f"{k} {v[0]:.2f}" for k, v in row["device_stages_ms"].items())
        line += "\n    host route: " + ", ".join(f"{k} {v[0]:.2f}" for k, v in row["host_stages_ms"].items())
        print(line, flush=True)
        lines.append(line)
        for c in frames + [kf]:
            c.free()
    gpu.close()
    if a.kernels:
        return
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "depthfilter_probe.json"), "w") as f:
        json.dump({"reps": a.reps, "warm_up": WARM, "ms": "median [min, max] of a host clock around the calls", "rows": rows}, f, indent=1)
    with open(os.path.join(a.out, "depthfilter_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
