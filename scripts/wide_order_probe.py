"""Ordering clouds above 16 384 points: what ORDER=wide (the multi-block ordering, cvo_k_kd_wide.h) costs next to a default
context, whose route for these sizes is the host's std::nth_element.

  python scripts/wide_order_probe.py [--out DIR] [--reps N] [--leaf W ...]   wall times, written to DIR/order_probe.{json,txt}
  rocprofv3 --kernel-trace --stats -d DIR/trace -o order --output-format csv -- python scripts/wide_order_probe.py --kernels
                                                            the launches a profiler should see, nothing else

Clouds: synth.semantic_pair sources of 16 686 (the LiDAR front end's default selection), 37 995 (the README's RGB-D map
read-out), 100 000 and 307 200 points (a full 640 x 480 frame), each bare (xyz only) and with colour + labels.
Calls: cvo_cloud_upload of host arrays, and CvoGPU.upload_device of the same rows in torch tensors on the device (torch is
imported first and the library afterwards, as bench.py does).
Routes, alternated call by call in ONE process: a default context, an ORDER=wide context, and one more ORDER=wide context
per --leaf value with WIDE_LEAF set to it (the capacity of a leaf block; the default is the library's).
Wall time is a host clock around a call that ends in a device synchronisation; the median, minimum and maximum of --reps
calls after three warm-up calls per route.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from ingest_probe import alternate, host_upload, rows_of, stat  # noqa: E402
from unified_cvo_amd import CvoGPU, debug_wide_plan  # noqa: E402

SIZES = (16686, 37995, 100000, 307200)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order_wide"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--leaf", type=int, nargs="*", default=[], help="further WIDE_LEAF values to run next to the default")
    ap.add_argument("--kernels", action="store_true", help="only the launches of ORDER=wide, for a kernel trace")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wide_order_probe: torch sees no device (there is no CPU route to measure)")
    dev = torch.device("cuda", 0)
    W = debug_wide_plan(0)[0]
    gpus = {"default": CvoGPU(), f"wide(W={W})": CvoGPU()}
    for leaf in a.leaf:
        gpus[f"wide(W={leaf})"] = CvoGPU()
    for name, g in gpus.items():
        if name != "default":
            g.set_option("ORDER", "wide")
        if name not in ("default", f"wide(W={W})"):
            g.set_option("WIDE_LEAF", name[7:-1])
    rows, lines = [], []
    for n in SIZES:
        for attrs in (False, True):
            arrs = rows_of(n, attrs)
            tensors = [torch.from_numpy(x).to(dev) for x in arrs]
            torch.cuda.synchronize()
            case = f"{n} {'colour+labels' if attrs else 'xyz'}"
            if a.kernels:
                g = gpus[f"wide(W={W})"]
                for _ in range(5):
                    host_upload(g, arrs).free()
                    g.upload_device(*tensors).free()
                continue
            for name, g in gpus.items():
                h, d = host_upload(g, arrs), g.upload_device(*tensors)
                assert h.debug_order_route() == d.debug_order_route() == (0 if name == "default" else 2), (case, name)
                assert np.array_equal(h.debug_order(), d.debug_order()), (case, name)
                h.free()
                d.free()
            for call, fn in (("upload", lambda g: host_upload(g, arrs)), ("upload_device", lambda g: g.upload_device(*tensors))):
                ts = alternate({name: (lambda g=g: fn(g)) for name, g in gpus.items()}, a.reps)
                row = {"case": case, "call": call, "points": n, "ms": {k: stat(v) for k, v in ts.items()}}
                rows.append(row)
                line = f"{case:22s} {call:14s} " + "  ".join(f"{k} {v[0]:.3f} ms [{v[1]:.3f}..{v[2]:.3f}]" for k, v in row["ms"].items())
                print(line, flush=True)
                lines.append(line)
    for g in gpus.values():
        g.close()
    if a.kernels:
        return
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "order_probe.json"), "w") as f:
        json.dump({"reps": a.reps, "warm_up": 3, "ms": "median [min, max] of a host clock around the call", "rows": rows}, f, indent=1)
    with open(os.path.join(a.out, "order_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
