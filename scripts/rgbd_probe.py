"""RGB-D front end: what a depth + colour frame costs on its way to a resident cloud.

  python scripts/rgbd_probe.py [--out DIR] [--reps N]     wall times, written to DIR/rgbd_probe.{json,txt}
  python scripts/rgbd_probe.py --shapes 150x200 240x320 --name rgbd_probe_small     other frame sizes (rows x cols)
  rocprofv3 --kernel-trace --stats -d DIR/trace -o rgbd --output-format csv -- python scripts/rgbd_probe.py --kernels
                                                           the launches a profiler should see, nothing else

Frames: synth.rgbd_frame("textured") at 640 x 480 and 1280 x 720, uint16 depth, leaf 0.1 and 0.25, edge divisor 4.
Routes, alternated call by call in ONE process (other work shares the machine):
  device   upload_rgbd with RGBD_HOST=0: the kernels of cvo_k_rgbd.h, voxel selection on the resident coordinates,
           rows of the survivors built on the host, the ordinary upload;
  twin     upload_rgbd with RGBD_HOST=1: the same call with the CPU twin and the CPU voxel selection;
  before   what a caller had before this call existed: both candidate clouds built on one CPU thread
           (cvo_rgbd_points_host into preallocated arrays), their rows turned into colour clouds with numpy, two
           upload_voxel calls, the pixel lists concatenated on the host.  It ends with TWO resident clouds, not one.
Wall time is a host clock around the call, which returns after the upload stream has been synchronised: the median
and the spread of --reps calls after two warm-up calls per route.  The pixels of the three routes are compared.
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

from unified_cvo_amd import CvoGPU, CvoPointCloud, RGBDFrame, synth  # noqa: E402
from unified_cvo_amd.api import DSO_EDGES, FULL, _fptr  # noqa: E402

SHAPES = ((480, 640), (720, 1280))
LEAVES = (0.1, 0.25)


class Before:
    """The route of a caller without upload_rgbd, its buffers allocated once."""

    def __init__(self, gpu, frame):
        self.gpu, self.f, self.fs = gpu, frame, frame.c_struct()
        n = frame.rows * frame.cols
        self.pixel = np.zeros(n, np.int32)
        self.xyz, self.feat = np.zeros((n, 3), np.float32), np.zeros((n, frame.channels + 2), np.float32)
        self.n = C.c_int()

    def run(self, leaf, divisor=4.0):
        out = []
        for method, s, gt in ((DSO_EDGES, np.float32(leaf) / np.float32(divisor), (1.0, 0.0)), (FULL, leaf, (0.0, 1.0))):
            rc = self.gpu.L.cvo_rgbd_points_host(C.byref(self.fs), method, self.pixel.ctypes.data_as(C.POINTER(C.c_int)), C.byref(self.n),
                                                 _fptr(self.xyz), _fptr(self.feat), None, None)
            assert rc == 0
            k = self.n.value
            feat = np.zeros((k, 5), np.float32)
            feat[:, :3] = self.feat[:k, :3]  # (the byte round trip is the identity on 3-channel frames)
            pc = CvoPointCloud.from_arrays(self.xyz[:k], feat, None, np.tile(np.array([gt], np.float32), (k, 1)))
            d = self.gpu.upload_voxel(pc, float(s))
            out.append((d, self.pixel[:k][d.kept]))
        pixel = np.concatenate([out[0][1], out[1][1]])
        for d, _ in out:
            d.free()
        return pixel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgbd"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--kernels", action="store_true", help="only the launches, for a kernel trace")
    ap.add_argument("--shapes", nargs="+", default=[f"{r}x{c}" for r, c in SHAPES], help="frame sizes, ROWSxCOLS")
    ap.add_argument("--name", default="rgbd_probe", help="base name of the two result files")
    a = ap.parse_args()
    gpu = CvoGPU()
    frames = [RGBDFrame(**synth.rgbd_frame("textured", rows, cols)) for rows, cols in (map(int, s.split("x")) for s in a.shapes)]
    if a.kernels:
        gpu.set_option("RGBD_HOST", 0)
        for f in frames:
            for leaf in LEAVES:
                for _ in range(5):
                    gpu.upload_rgbd(f, leaf).free()
                print(f"{f.cols}x{f.rows} leaf {leaf}: {gpu.debug_rgbd_stats()}", flush=True)
        gpu.close()
        return
    os.makedirs(a.out, exist_ok=True)
    rows, lines = [], []
    for f in frames:
        before = Before(gpu, f)
        for leaf in LEAVES:
            ts = {"device": [], "twin": [], "before": []}
            pix = {}
            for rep in range(a.reps + 2):
                for name in ts:
                    gpu.set_option("RGBD_HOST", {"device": 0, "twin": 1}.get(name))
                    t0 = time.perf_counter()
                    if name == "before":
                        p = before.run(leaf)
                    else:
                        d = gpu.upload_rgbd(f, leaf)
                        p = d.pixel
                        d.free()
                    dt = (time.perf_counter() - t0) * 1e3
                    pix[name] = p
                    if rep >= 2:
                        ts[name].append(dt)
            gpu.set_option("RGBD_HOST", None)
            assert np.array_equal(pix["device"], pix["twin"]) and np.array_equal(pix["device"], pix["before"])
            med = {k: float(np.median(v)) for k, v in ts.items()}
            row = {"cols": f.cols, "rows": f.rows, "leaf": leaf, "points": int(len(pix["device"])),
                   "ms": {k: [round(med[k], 3), round(float(np.min(v)), 3), round(float(np.max(v)), 3)] for k, v in ts.items()},
                   "before_over_device": round(med["before"] / med["device"], 2), "twin_over_device": round(med["twin"] / med["device"], 2)}
            rows.append(row)
            line = (f"{f.cols:5d} x {f.rows:4d} leaf {leaf:<4} points {row['points']:6d} | upload_rgbd ms "
                    + "  ".join(f"{k} {v[0]:.2f} [{v[1]:.2f}..{v[2]:.2f}]" for k, v in row["ms"].items())
                    + f" | before / device {row['before_over_device']:.2f}  twin / device {row['twin_over_device']:.2f}")
            print(line, flush=True)
            lines.append(line)
    gpu.close()
    with open(os.path.join(a.out, a.name + ".json"), "w") as fo:
        json.dump({"reps": a.reps, "ms": "median [min, max] of a host clock around the call", "rows": rows}, fo, indent=1)
    with open(os.path.join(a.out, a.name + ".txt"), "w") as fo:
        fo.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
