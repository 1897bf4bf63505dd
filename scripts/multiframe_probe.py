"""Times multi-frame align (CvoGPU.align_multiframe) on windows of 4, 8 and 16 frames of the street scene at 10k points
each: frame 0 held, every other frame perturbed by up to 2 deg / 5 cm, edges between frames up to 3 apart.  Prints one
line per window: outer iterations, trust-region steps, ms per step (the whole call divided by the steps: the edge
evaluations of every outer iteration are included), total time.  Usage: python scripts/multiframe_probe.py [n_points]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cases  # noqa: E402
from unified_cvo_amd import CvoGPU, CvoPointCloud, CvoFrameGPU, synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    P = cases.load_params("geometric_gpu")
    P.multiframe_ell_init, P.multiframe_ell_min, P.multiframe_ell_decay_rate = 0.3, 0.1, 0.7
    P.multiframe_num_neighbors, P.multiframe_max_iters = 64, 20
    P.multiframe_iterations_per_ell, P.multiframe_iterations_per_solve, P.multiframe_min_nonzeros = 3, 8, 300
    gpu = CvoGPU(params=P)
    for F in (4, 8, 16):
        xyz, gt = synth.scene_sequence(F, n, seed=F)
        rs = np.random.default_rng(F)
        frames = []
        for f in range(F):
            T = np.eye(4)
            T[:3] = gt[f]
            if f:
                D = np.eye(4)
                D[:3, :3] = synth.rot_axis_angle(rs.normal(size=3), rs.uniform(-2, 2))
                D[:3, 3] = rs.uniform(-0.05, 0.05, 3)
                T = T @ D
            frames.append(CvoFrameGPU(gpu, CvoPointCloud.from_xyz(xyz[f]), T[:3]))
        edges = [(i, j) for i in range(F) for j in range(i + 1, min(F, i + 4))]
        t0 = time.perf_counter()
        info, trace = gpu.align_multiframe(frames, [True] + [False] * (F - 1), edges, trace=True)
        wall = time.perf_counter() - t0
        steps = max(info["steps"], 1)
        print(f"frames {F:2d} x {n} points, {len(edges)} edges: outer iterations {info['outer_iterations']}, "
              f"steps {info['steps']} ({info['accepted_steps']} accepted), {1e3 * info['seconds'] / steps:.3f} ms per step "
              f"(whole call / steps), total {1e3 * info['seconds']:.1f} ms (wall {1e3 * wall:.1f} ms), "
              f"last nonzeros {info['last_total_nonzeros']}", flush=True)


if __name__ == "__main__":
    main()
