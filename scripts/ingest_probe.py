"""Clouds from rows that are already on the device: what cvo_cloud_from_device costs next to the route a caller had before.

  python scripts/ingest_probe.py [--out DIR] [--reps N]     wall times, written to DIR/ingest_probe.{json,txt}
  rocprofv3 --kernel-trace --stats -d DIR/trace -o ingest --output-format csv -- python scripts/ingest_probe.py --kernels
                                                            the launches a profiler should see, nothing else

Clouds: synth.semantic_pair sources of 10 000 and 16 384 points with colour and one-hot labels, 10 000 points xyz only, and
100 000 points with colour and labels (above KD_MAX_POINTS: ordered on the host, attributes gathered by k_cloud_gather).
The rows live in torch tensors on the device (torch is imported first and the library afterwards, as bench.py does).
Routes, alternated call by call in ONE process:
  (a) d2h+upload   every tensor copied to host memory (tensor.cpu()), then cvo_cloud_upload of the host arrays
  (b) from_device  CvoGPU.upload_device of the tensors
and for 64 clouds of 10 000 points with colour and labels
  (c) upload_many  cvo_cloud_upload_many of host arrays that are already there (no device-to-host copy in it)
      from_device_many  cvo_cloud_from_device_many of the 64 clouds' device rows
Wall time is a host clock around a call that ends in a device synchronisation; the median, minimum and maximum of --reps
calls after three warm-up calls per route.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from unified_cvo_amd import CvoGPU, synth  # noqa: E402

WARM = 3
CASES = (("10k feat+label", 10000, True), ("16384 feat+label", 16384, True), ("10k xyz", 10000, False), ("100k feat+label", 100000, True))


def rows_of(n, attrs, pair_id=0):
    src, fsrc, lsrc = synth.semantic_pair(n, pair_id)[:3]
    a = [np.ascontiguousarray(src, np.float32)]
    if attrs:
        a += [np.ascontiguousarray(fsrc, np.float32), np.ascontiguousarray(lsrc, np.float32)]
    return a


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def host_upload(gpu, arrs):
    h = C.c_void_p()
    p = [fptr(a) for a in arrs] + [None] * (4 - len(arrs))
    gpu._check(gpu.L.cvo_cloud_upload(gpu.ctx, arrs[0].shape[0], *p, C.byref(h)))
    return gpu._adopt(h, arrs[0].shape[0])


def route_a(gpu, tensors):
    return host_upload(gpu, [t.cpu().numpy() for t in tensors])


def route_b(gpu, tensors):
    return gpu.upload_device(*tensors)


def alternate(routes, reps):
    """{name: [ms]} of routes = {name: fn -> cloud or list of clouds}, alternated call by call."""
    ts = {k: [] for k in routes}
    for rep in range(reps + WARM):
        for name, fn in routes.items():
            t0 = time.perf_counter()
            out = fn()
            dt = (time.perf_counter() - t0) * 1e3
            for c in out if isinstance(out, list) else [out]:
                c.free()
            if rep >= WARM:
                ts[name].append(dt)
    return ts


def stat(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def many_routes(gpu, dev, n_clouds=64, n=10000):
    host = [rows_of(n, True, k) for k in range(n_clouds)]
    tens = [[torch.from_numpy(a).to(dev) for a in arrs] for arrs in host]
    fpp = C.POINTER(C.c_float)
    counts = (C.c_int * n_clouds)(*[n] * n_clouds)
    cols = [(fpp * n_clouds)(*[fptr(arrs[i]) for arrs in host]) for i in range(3)]

    def upload_many():
        out = (C.c_void_p * n_clouds)()
        gpu._check(gpu.L.cvo_cloud_upload_many(gpu.ctx, n_clouds, counts, cols[0], cols[1], cols[2], None, 4, out))
        return [gpu._adopt(C.c_void_p(out[i]), n) for i in range(n_clouds)]

    return {"upload_many": upload_many, "from_device_many": lambda: gpu.upload_device_many([tuple(t) for t in tens])}, (host, tens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernels", action="store_true", help="only the launches, for a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_probe: torch sees no device (there is no CPU route to measure)")
    dev = torch.device("cuda", 0)
    gpu = CvoGPU()
    rows, lines = [], []
    for name, n, attrs in CASES:
        tensors = [torch.from_numpy(x).to(dev) for x in rows_of(n, attrs)]
        torch.cuda.synchronize()
        if a.kernels:
            for _ in range(5):
                route_b(gpu, tensors).free()
            continue
        ha, hb = route_a(gpu, tensors), route_b(gpu, tensors)
        assert np.array_equal(ha.debug_order(), hb.debug_order()), name
        ha.free()
        hb.free()
        ts = alternate({"d2h+upload": lambda: route_a(gpu, tensors), "from_device": lambda: route_b(gpu, tensors)}, a.reps)
        row = {"case": name, "points": n, "bytes_in": sum(t.numel() * 4 for t in tensors), "ms": {k: stat(v) for k, v in ts.items()}}
        rows.append(row)
        line = f"{name:18s} " + "  ".join(f"{k} {v[0]:.3f} ms [{v[1]:.3f}..{v[2]:.3f}]" for k, v in row["ms"].items())
        print(line, flush=True)
        lines.append(line)
    routes, keep = many_routes(gpu, dev)
    if a.kernels:
        for _ in range(5):
            for c in routes["from_device_many"]():
                c.free()
        gpu.close()
        return
    ts = alternate(routes, a.reps)
    row = {"case": "64 x 10k feat+label", "points": 64 * 10000, "ms": {k: stat(v) for k, v in ts.items()}}
    rows.append(row)
    line = f"{row['case']:18s} " + "  ".join(f"{k} {v[0]:.3f} ms [{v[1]:.3f}..{v[2]:.3f}]" for k, v in row["ms"].items())
    print(line, flush=True)
    lines.append(line)
    gpu.close()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "ingest_probe.json"), "w") as f:
        json.dump({"reps": a.reps, "warm_up": WARM, "ms": "median [min, max] of a host clock around the call", "rows": rows}, f, indent=1)
    with open(os.path.join(a.out, "ingest_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
