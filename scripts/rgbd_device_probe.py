"""RGB-D frames that are already on the device: what cvo_cloud_from_rgbd_device / _recipe cost next to the route a caller had
before from the same device-resident planes.

  python scripts/rgbd_device_probe.py [--out DIR] [--reps N]     wall times, written to DIR/rgbd_device_probe.{json,txt}
  rocprofv3 --kernel-trace --stats -d DIR/trace -o rgbd_device --output-format csv -- python scripts/rgbd_device_probe.py --kernels
                                                                  the launches a profiler should see, nothing else

The planes live in torch tensors on the device (torch is imported first and the library afterwards, as bench.py does).
Routes, results checked equal first, alternated call by call in ONE process under RGBD_HOST=0:
  old   every plane copied to host memory (tensor.cpu(); C x H x W scores permuted to H x W x C on the host), then
        rgbd_points + upload - for the recipe: upload_rgbd
  new   CvoGPU.upload_rgbd_points_device / upload_rgbd_device of a DeviceRGBDFrame over the tensors (no pixel list asked for)
Cases: 640 x 480 colour without classes; 640 x 480 with 19 classes as H x W x C and as C x H x W; 1280 x 720 with 19 classes
(C x H x W); the recipe at leaf 0.1 and 0.25 on the 640 x 480 colour frame.  Constructor cases use DSO_EDGES.
Wall time is a host clock around a call that ends in a device synchronisation; the median, minimum and maximum of --reps calls
after three warm-up calls per route.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from unified_cvo_amd import CvoGPU, DeviceRGBDFrame, RGBDFrame, synth  # noqa: E402
from unified_cvo_amd.api import DSO_EDGES  # noqa: E402

WARM = 3
# name, rows, cols, classes, layout of the scores on the device, recipe leaf (None: the constructor with DSO_EDGES)
CASES = (("640x480 colour", 480, 640, 0, "hwc", None), ("640x480 19 classes HWC", 480, 640, 19, "hwc", None),
         ("640x480 19 classes CHW", 480, 640, 19, "chw", None), ("1280x720 19 classes CHW", 720, 1280, 19, "chw", None),
         ("640x480 recipe leaf 0.1", 480, 640, 0, "hwc", 0.1), ("640x480 recipe leaf 0.25", 480, 640, 0, "hwc", 0.25))


def tensors_of(f, layout, dev):
    t = dict(image=torch.from_numpy(f.image).to(dev), depth=torch.from_numpy(f.depth.astype(np.int16) if f.depth.dtype == np.uint16 else f.depth).to(dev))
    if f.semantic is not None:
        s = torch.from_numpy(f.semantic).to(dev)
        t["semantic"] = s if layout == "hwc" else s.permute(2, 0, 1).contiguous()
    return t


def old_route(gpu, f, t, layout, leaf):
    image, depth = t["image"].cpu().numpy(), t["depth"].cpu().numpy()
    if depth.dtype == np.int16:
        depth = depth.view(np.uint16)
    sem = None
    if "semantic" in t:
        s = t["semantic"].cpu().numpy()
        sem = s if layout == "hwc" else np.ascontiguousarray(np.moveaxis(s, 0, 2))
    host = RGBDFrame(image, depth, f.fx, f.fy, f.cx, f.cy, f.scaling_factor, semantic=sem)
    return gpu.upload_rgbd(host, leaf) if leaf else gpu.upload(gpu.rgbd_points(host, DSO_EDGES))


def new_route(gpu, frame, leaf):
    return gpu.upload_rgbd_device(frame, leaf) if leaf else gpu.upload_rgbd_points_device(frame, DSO_EDGES)


def stat(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgbd_device"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernels", action="store_true", help="only the new route's launches, for a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rgbd_device_probe: torch sees no device (there is no CPU route to measure)")
    dev = torch.device("cuda", 0)
    gpu = CvoGPU()
    gpu.set_option("RGBD_HOST", 0)
    rows, lines = [], []
    for name, h, w, classes, layout, leaf in CASES:
        f = RGBDFrame(**synth.rgbd_frame(kind="textured", rows=h, cols=w, num_classes=classes))
        t = tensors_of(f, layout, dev)
        torch.cuda.synchronize()
        frame = DeviceRGBDFrame(t["image"], t["depth"], f.fx, f.fy, f.cx, f.cy, f.scaling_factor, semantic=t.get("semantic"), layout=layout)
        if a.kernels:
            for _ in range(5):
                new_route(gpu, frame, leaf).free()
            continue
        old, new = old_route(gpu, f, t, layout, leaf), new_route(gpu, frame, leaf)
        assert old.n == new.n and np.array_equal(old.debug_order(), new.debug_order()), name
        do, dn = old.download(), new.download()
        for x, y in ((do.positions_, dn.positions_), (do.features_, dn.features_), (do.labels_, dn.labels_), (do.geometric_types_, dn.geometric_types_)):
            assert np.array_equal(np.asarray(x, np.float32).view(np.uint32), np.asarray(y, np.float32).view(np.uint32)), name
        n = new.n
        old.free()
        new.free()
        ts = {"old": [], "new": []}
        for rep in range(a.reps + WARM):
            for route, fn in (("old", lambda: old_route(gpu, f, t, layout, leaf)), ("new", lambda: new_route(gpu, frame, leaf))):
                t0 = time.perf_counter()
                c = fn()
                dt = (time.perf_counter() - t0) * 1e3
                c.free()
                if rep >= WARM:
                    ts[route].append(dt)
        row = {"case": name, "points": n, "ms": {k: stat(v) for k, v in ts.items()}}
        rows.append(row)
        line = f"{name:26s} {n:6d} points  " + "  ".join(f"{k} {v[0]:.3f} ms [{v[1]:.3f}..{v[2]:.3f}]" for k, v in row["ms"].items())
        print(line, flush=True)
        lines.append(line)
    gpu.close()
    if a.kernels:
        return
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "rgbd_device_probe.json"), "w") as fh:
        json.dump({"reps": a.reps, "warm_up": WARM, "ms": "median [min, max] of a host clock around the call", "rows": rows}, fh, indent=1)
    with open(os.path.join(a.out, "rgbd_device_probe.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
