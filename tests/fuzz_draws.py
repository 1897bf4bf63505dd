"""The randomised draws of the fuzz tests (test_gpu_parity.py): parameters, clouds and initial guess of one seed.  Shared so
that test_gpu_speculation.py runs exactly the pairs the oracle comparisons run."""
import numpy as np

import cases
from unified_cvo_amd import CvoPointCloud, synth


def trajectory(seed):
    """test_randomised_trajectories: random sizes / parameters / initial guesses over slab clouds of the three feature
    kinds (seed % 3: geometry, colour, semantics).  Returns (P, source, target, init)."""
    rs = np.random.default_rng(100 + seed)
    kind = seed % 3
    n = int(rs.integers(150, 1800))
    m = int(rs.integers(150, 1800))
    if seed % 8 == 7:  # a few at BASELINE scale (up to 10k x 10k, ragged)
        n = int(rs.integers(4000, 10001))
        m = int(rs.integers(4000, 10001))
    if kind == 0:
        P = cases.load_params("geometric_gpu")
        src, tgt, _ = synth.geometric_pair(n, seed, m=m)
        a, b = CvoPointCloud.from_xyz(src), CvoPointCloud.from_xyz(tgt)
    elif kind == 1:
        P = cases.load_params("intensity_gpu")
        src, fsrc, tgt, ftgt, _, _ = synth.colour_pair(max(n, m), seed)
        geo = np.tile(np.array([[0.0, 1.0]], np.float32), (max(n, m), 1))
        a = CvoPointCloud.from_arrays(src[:n], fsrc[:n], None, geo[:n])
        b = CvoPointCloud.from_arrays(tgt[:m], ftgt[:m], None, geo[:m])
    else:
        P = cases.load_params("semantic_img_gpu0")
        k = max(n, m)
        src, fsrc, lsrc, tgt, ftgt, ltgt = synth.semantic_pair(k, seed)
        geo = np.tile(np.array([[0.0, 1.0]], np.float32), (k, 1))
        a = CvoPointCloud.from_arrays(src[:n], fsrc[:n], lsrc[:n], geo[:n])
        b = CvoPointCloud.from_arrays(tgt[:m], ftgt[:m], ltgt[:m], geo[:m])
    P.ell_init = float(rs.choice([0.15, 0.3, 0.6, 1.2]))           # 1.2: dense, rows overflow their lists
    P.nearest_neighbors_max = int(rs.choice([8, 40, 512]))         # 8 / 40: the first-K truncation bites
    P.ell_decay_start = int(rs.choice([5, 30]))
    P.min_step = float(rs.choice([1e-4, 2e-3]))
    P.is_using_range_ell = int(rs.integers(0, 2))
    init = (synth.gt_motion() @ synth.warm_start_delta()).astype(np.float32) if rs.integers(0, 2) else np.eye(4, dtype=np.float32)
    return P, a, b, init


def clustered(seed):
    """test_randomised_clustered_trajectories: clustered clouds (synth.scene_pair: local density varies by more than 100x)
    of random, ragged sizes; seed % 3: geometry only / + colour / + colour and semantics.  Returns (P, source, target, init)."""
    rs = np.random.default_rng(900 + seed)
    n, m = int(rs.integers(1200, 6500)), int(rs.integers(1200, 6500))
    src, tgt, _ = synth.scene_pair(n, 50 + seed, m=m)
    kind = seed % 3   # geometry only / + colour / + colour and semantics (k_assoc, k_assoc_dense: GENERAL instantiations)
    if kind == 0:
        a, b = CvoPointCloud.from_xyz(src), CvoPointCloud.from_xyz(tgt)
        P = cases.load_params("geometric_gpu")
    else:
        T = synth.gt_motion()
        back = (tgt.astype(np.float64) - T[:3, 3]) @ T[:3, :3]          # the target points before the motion (+ noise)
        fs = synth.colour_features(src, np.random.default_rng(7100 + seed)).astype(np.float32)
        ft = synth.colour_features(back, np.random.default_rng(7200 + seed), noise=0.01).astype(np.float32)
        geo = np.tile(np.array([[0.0, 1.0]], np.float32), (max(n, m), 1))
        ls = synth.checkerboard_labels(src) if kind == 2 else None
        lt = synth.checkerboard_labels(back, flip=0.02, rng=np.random.default_rng(7300 + seed)) if kind == 2 else None
        a, b = CvoPointCloud.from_arrays(src, fs, ls, geo[:n]), CvoPointCloud.from_arrays(tgt, ft, lt, geo[:m])
        P = cases.load_params("intensity_gpu" if kind == 1 else "semantic_img_gpu0")
    P.ell_init = float(rs.choice([0.3, 0.6, 0.95, 1.4]))
    P.nearest_neighbors_max = int(rs.choice([40, 200, 512]))
    P.ell_decay_start = int(rs.choice([5, 30]))
    P.is_using_range_ell = int(rs.integers(0, 2))
    init = (synth.gt_motion() @ synth.warm_start_delta()).astype(np.float32) if rs.integers(0, 2) else np.eye(4, dtype=np.float32)
    return P, a, b, init
