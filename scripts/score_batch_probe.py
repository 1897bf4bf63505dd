"""Batched scores against the loop of single calls they replace (GPU box).

Two workloads, each timed as ONE batch call and as the loop of single calls, steady-state wall time (median of REPS
timed repetitions after two warm-up runs; every call ends in a device synchronisation) -> jobs/s:
  pairs  64 frame pairs x exact function_angle at 10k x 10k, configs 2 / 3 / 4 (64 distinct clouds on each side)
  sweep  one 10k pair x 64 poses, exact function_angle (the evaluate-indicator sweep; <X, X>, <Y, Y> once per batch)
Every batch value is checked == the single call's.  usage: score_batch_probe.py [--quick] [--out FILE.json]
(--quick: 8 jobs at 2k points, one config - a rehearsal; under rocprofv3 --kernel-trace use --batch-only: the batch calls
only; --trace-summary DB: per-kernel statistics of that trace's database, on any machine)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import cases  # noqa: E402
from unified_cvo_amd import CvoGPU, synth  # noqa: E402


def med(fn, reps):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def pose(k):
    a = 0.003 * (k - 32)
    c, s = np.cos(a), np.sin(a)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
    T[:3, 3] = (0.004 * (k - 32), 0.002 * (k % 9), 0.0)
    return T


def run(name, gpu, S, D, Ts, ell, reps, batch_only=False):
    n = len(S)
    batch = lambda: gpu.function_angle_batch(S, D, Ts, ell, is_approximate=False)  # noqa: E731
    loop = lambda: [gpu.function_angle(s, d, T, ell, False) for s, d, T in zip(S, D, Ts)]  # noqa: E731
    tb = med(batch, reps)
    ov, ch, launches = gpu.debug_last_score_batch()
    row = dict(workload=name, jobs=n, batch_s=tb[0], batch_min_s=tb[1], batch_max_s=tb[2], batch_jobs_per_s=n / tb[0],
               overlap_evals=ov, chain_evals=ch, launches=launches)
    if not batch_only:
        tl = med(loop, reps)
        got, want = batch(), np.array(loop(), np.float32)
        row.update(loop_s=tl[0], loop_min_s=tl[1], loop_max_s=tl[2], loop_jobs_per_s=n / tl[0], speedup=tl[0] / tb[0],
                   bit_identical=bool(np.array_equal(got, want)))
    print(json.dumps(row), flush=True)
    return row


def trace_summary(db_path):
    """Per-kernel statistics of a rocprofv3 --kernel-trace database (rocpd SQLite) and every k_overlap_table launch."""
    import re
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, duration, grid_x, workgroup_x, lds_size, vgpr_count from kernels order by start").fetchall()
    short = lambda n: (re.search(r"(\w+(<[^>]*>)?)\(", n.replace("(anonymous namespace)::", "")) or re.search(r"(.*)", n)).group(1)  # noqa: E731
    st = {}
    for n, d, *_ in rows:
        st.setdefault(short(n), []).append(d / 1e3)
    print(f"{'kernel':36s} {'calls':>6s} {'total_us':>10s} {'avg_us':>8s} {'min_us':>8s} {'max_us':>8s}")
    for k, v in sorted(st.items(), key=lambda kv: -sum(kv[1])):
        print(f"{k:36s} {len(v):6d} {sum(v):10.1f} {sum(v) / len(v):8.2f} {min(v):8.2f} {max(v):8.2f}")
    print("\nk_overlap_table launches in order:")
    for n, d, gx, wx, lds, vgpr in rows:
        if "k_overlap_table" in n:
            print(f"  {short(n):22s} blocks {gx // wx:6d}  {d / 1e3:8.2f} us  {gx // wx / (d / 1e3):6.1f} blocks/us  LDS {lds} B")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-summary", metavar="DB", help="summarise a rocprofv3 kernel-trace database instead (CPU)")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--batch-only", action="store_true", help="batch calls only (for a rocprofv3 kernel trace)")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.trace_summary:
        trace_summary(a.trace_summary)
        return
    n_pts, n_jobs = (2000, 8) if a.quick else (10000, 64)
    configs = (("config2", cases.config2),) if a.quick else (("config2", cases.config2), ("config3", cases.config3),
                                                             ("config4", cases.config4))
    rows = []
    for cname, builder in configs:
        P = builder(n=64)[0]
        gpu = CvoGPU(params=P)
        S, D = [], []
        for k in range(n_jobs):
            _, s, d, _ = builder(n=n_pts, pair_id=k)
            S.append(gpu.upload(s))
            D.append(gpu.upload(d))
        Ts = [synth.gt_motion().astype(np.float32) if k % 2 else np.eye(4, dtype=np.float32) for k in range(n_jobs)]
        rows.append(run(f"pairs {cname} {n_jobs} x {n_pts}", gpu, S, D, Ts, P.ell_init, a.reps, a.batch_only))
        sweep = [pose(k) for k in range(n_jobs)]
        rows.append(run(f"sweep {cname} 1 pair x {n_jobs} poses", gpu, [S[0]] * n_jobs, [D[0]] * n_jobs, sweep, P.ell_init,
                        a.reps, a.batch_only))
        gpu.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
